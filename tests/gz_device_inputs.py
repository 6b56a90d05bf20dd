"""Helpers of the device inflater's tests (dart_amd/csrc/dg_inflate.h): a BGZF writer over zlib's raw deflate, a deflate bit writer for hand-made streams,
the valid and invalid streams both suites use, Python restatements of the whole-record rule and of fast_fastq.h::gz_reader_sees_the_same, and the driver of
tests/native/inflate_checks.hip.  zlib's own verdict on every stream is asserted here, on the CPU, before the stream is handed out: a typo in this file
cannot pass as a result of the code under test."""
from __future__ import annotations

import os, struct, subprocess, zlib
import numpy as np
import common

BLOCK = 0xff00
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")       # the SAM specification's end-of-file marker
# the INF_E_* rules of dg_inflate.h
(OK, E_BTYPE, E_STORED, E_SYMBOLS, E_CODELEN_SET, E_REPEAT, E_NO_EOB, E_LITLEN_SET, E_DIST_SET, E_LITLEN_CODE, E_DIST_CODE, E_FAR, E_INPUT, E_ISIZE,
 E_CRC) = range(15)
WALKER = -1


# ---- BGZF ----------------------------------------------------------------------------------------------------------------------------------------
def member(raw: bytes, data: bytes | None = None, crc: int | None = None, isize: int | None = None, extra_front: bytes = b"", flg: int = 4, bc: bool = True,
           bsize: int | None = None) -> bytes:
    """one gzip member around a raw deflate stream; data: what it inflates to (for CRC32 and ISIZE, unless given); extra_front: subfields in front of BC"""
    extra = extra_front + (b"BC\x02\x00\x00\x00" if bc else b"")
    total = 12 + len(extra) + len(raw) + 8
    if bc:
        extra = extra[:-2] + struct.pack("<H", (total if bsize is None else bsize) - 1)
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) if isize is None else isize
    return b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff" + struct.pack("<H", len(extra)) + extra + raw + struct.pack("<II", crc & 0xffffffff, isize)


def deflate_raw(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, full_flush_at=()) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, last = b"", 0
    for cut in full_flush_at:
        out += c.compress(data[last:cut]) + c.flush(zlib.Z_FULL_FLUSH); last = cut
    return out + c.compress(data[last:]) + c.flush()


def bgzf(data: bytes, block=BLOCK, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, eof=False, **kw) -> bytes:
    out = b""
    for a in range(0, len(data), block):
        out += member(deflate_raw(data[a:a + block], level, strategy), data[a:a + block], **kw)
    return out + (EOF_MEMBER if eof else b"")


def bgzf_reference(blocks: bytes) -> bytes:
    """zlib on a whole BGZF file, member by member"""
    out = b""
    while blocks:
        d = zlib.decompressobj(31)
        out += d.decompress(blocks)
        assert d.eof
        blocks = d.unused_data
    return out


def fastq_like(n, seed=1) -> bytes:
    rng = np.random.default_rng(seed)
    out = bytearray()
    i = 0
    while len(out) < n:
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 101)].tobytes()
        q = bytes((33 + np.minimum(40, rng.integers(20, 60, 101))).astype(np.uint8))
        out += b"@read%d/1\n" % i + seq + b"\n+\n" + q + b"\n"; i += 1
    return bytes(out[:n])


# ---- a deflate bit writer --------------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):                     # n bits of v, lowest first (header fields, extra bits)
        self.acc |= (v & ((1 << n) - 1)) << self.n; self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255); self.acc >>= 8; self.n -= 8

    def code(self, c, n):                    # a Huffman code: highest bit first
        for k in range(n - 1, -1, -1):
            self.put((c >> k) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self) -> bytes:
        self.align()
        return bytes(self.out)


def canon(lens):
    """RFC 1951 3.2.2: lengths -> {symbol: (code, length)}"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1; nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l); nxt[l] += 1
    return out


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CLC_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CLC_LENS = [4] * 13 + [5] * 6              # a complete code over all 19 symbols: 13 / 16 + 6 / 32 = 1


def len_sym(l):
    s = max(k for k in range(29) if LEN_BASE[k] <= l) if l < 258 else 28
    return 257 + s, LEN_EXTRA[s], l - LEN_BASE[s]


def dist_sym(d):
    s = max(k for k in range(30) if DIST_BASE[k] <= d)
    return s, DIST_EXTRA[s], d - DIST_BASE[s]


def put_tokens(w: Bits, tokens, lit_lens, dist_lens, eob=True):
    """tokens: an int is a literal, (length, distance) a match, ("sym", s) a bare literal / length symbol, ("dsym", length, s) a match with a bare distance symbol"""
    lc, dc = canon(lit_lens), canon(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lc[t])
        elif t[0] == "sym":
            w.code(*lc[t[1]])
        elif t[0] == "dsym":
            s, eb, ev = len_sym(t[1]); w.code(*lc[s]); w.put(ev, eb); w.code(*dc[t[2]])
        else:
            s, eb, ev = len_sym(t[0]); w.code(*lc[s]); w.put(ev, eb)
            s, eb, ev = dist_sym(t[1]); w.code(*dc[s]); w.put(ev, eb)
    if eob:
        w.code(*lc[256])


def fixed_block(w: Bits, tokens, final=True, eob=True):
    w.put(1 if final else 0, 1); w.put(1, 2)
    put_tokens(w, tokens, FIXED_LIT, FIXED_DIST, eob)


def stored_block(w: Bits, data: bytes, final=False, nlen=None):
    w.put(1 if final else 0, 1); w.put(0, 2); w.align()
    w.put(len(data), 16); w.put((~len(data) & 0xffff) if nlen is None else nlen, 16)
    for b in data:
        w.put(b, 8)


def rle_lengths(seq):
    """the code-length symbols of a header, greedily, over the literal / length and distance lengths as ONE sequence -> [(symbol, extra bits, value, start, end)]"""
    out, i = [], 0
    while i < len(seq):
        v = seq[i]; j = i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            k = min(run, 138)
            out.append((18, 7, k - 11, i, i + k) if k >= 11 else (17, 3, k - 3, i, i + k)); i += k
        elif v and run >= 4:
            out.append((v, 0, 0, i, i + 1)); k = min(run - 1, 6); out.append((16, 2, k - 3, i + 1, i + 1 + k)); i += 1 + k
        else:
            out.append((v, 0, 0, i, i + 1)); i += 1
    return out


def dynamic_header(w: Bits, lit_lens, dist_lens, final=True, clc_lens=None, cl_syms=None, hlit=None, hdist=None, hclen=19):
    """cl_syms: the code-length symbols as [(symbol, extra bits, value)] in place of rle_lengths' choice"""
    clc = CLC_LENS if clc_lens is None else clc_lens
    w.put(1 if final else 0, 1); w.put(2, 2)
    w.put(len(lit_lens) - 257 if hlit is None else hlit, 5); w.put(len(dist_lens) - 1 if hdist is None else hdist, 5); w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(clc[CLC_ORDER[k]], 3)
    codes = canon(clc)
    for s in (rle_lengths(list(lit_lens) + list(dist_lens)) if cl_syms is None else cl_syms):
        if s[0] in codes:
            w.code(*codes[s[0]])
        w.put(s[2], s[1])


def dynamic_block(w: Bits, lit_lens, dist_lens, tokens, final=True, eob=True, **kw):
    dynamic_header(w, lit_lens, dist_lens, final, **kw)
    put_tokens(w, tokens, lit_lens, dist_lens, eob)


def chain(symbols, n_syms):
    """a complete code over `symbols`: lengths 1, 2, 3, ... and the last two equal"""
    lens = [0] * n_syms
    for k, s in enumerate(symbols):
        lens[s] = min(k + 1, len(symbols) - 1)
    return lens


def inflate_or_none(raw: bytes):
    try:
        d = zlib.decompressobj(-15)
        out = d.decompress(raw)
        return out if d.eof else None
    except zlib.error:
        return None


# ---- the hand-made streams ---------------------------------------------------------------------------------------------------------------------------
def valid_streams(round_tokens=128):
    """-> {name: (raw deflate stream, what zlib inflates it to)}"""
    out = {}
    def add(name, w):
        raw = w.bytes()
        data = inflate_or_none(raw)
        assert data is not None, name
        out[name] = (raw, data)
    # a code of length 15: 16 symbols on a chain; the deepest are used (the first-level table does not hold them)
    syms = [ord("A"), 256, ord("C"), ord("G"), ord("T"), 257, ord("N"), 10, 64, 43, 73, 70, 48, 49, 50, 51]
    lit = chain(syms, 286); assert max(lit) == 15 and lit[50] == 15 and lit[51] == 15
    w = Bits(); dynamic_block(w, lit, [1, 1], [ord("A"), 50, 51, ord("C"), (3, 2), 49, 48, 51, 50, 10]); add("code_of_length_15", w)
    # a repeat that runs from the literal / length lengths into the distance lengths: 16 (previous length), and 18 (zeros)
    lit = [0] * 286
    for s in range(64, 96): lit[s] = 6                    # 32 codes of 6 bits = 1 / 2
    lit[256] = 2; lit[282] = lit[283] = lit[284] = lit[285] = 4      # 1 / 4 + 4 / 16: complete
    dist = [4] * 16
    rl = rle_lengths(lit + dist); assert any(s[0] == 16 and s[3] < 286 < s[4] for s in rl)
    w = Bits(); dynamic_block(w, lit, dist, [65, 66, 67, 68, (170, 3), 70, (258, 5), 95, (200, 2), (230, 150)]); add("repeat_16_crosses_into_distances", w)
    lit = [0] * 260
    lit[65] = 1; lit[256] = 1
    dist = [0, 0, 0, 0, 0, 1, 1]
    rl = rle_lengths(lit + dist); assert any(s[0] in (17, 18) and s[3] < 260 < s[4] for s in rl)
    w = Bits(); dynamic_block(w, lit, dist, [65, 65, 65]); add("repeat_of_zeros_crosses_into_distances", w)
    # one distance code only (zlib lets this one set be incomplete); no distance code at all
    lit = chain([ord("a"), ord("b"), 256, 257, 258], 259)
    w = Bits(); dynamic_block(w, lit, [1], [97, 98, (3, 1), (4, 1), 97]); add("one_distance_code", w)
    w = Bits(); dynamic_block(w, chain([ord("a"), ord("b"), 256], 257), [0], [97, 98, 98, 97, 97]); add("no_distance_code", w)
    # only the end-of-block code: one literal / length code of length 1
    lit = [0] * 257; lit[256] = 1
    w = Bits(); dynamic_block(w, lit, [0], []); add("end_of_block_only", w)
    # the largest distance with the largest length; the smallest distance with the largest length directly behind a stored block
    noise = np.random.default_rng(3).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = Bits(); stored_block(w, noise); fixed_block(w, [(258, 32768), 33, (258, 32768)]); add("distance_32768_length_258", w)
    w = Bits(); stored_block(w, b"x"); fixed_block(w, [(258, 1), (258, 1), (3, 1)]); add("distance_1_length_258_behind_stored", w)
    w = Bits(); stored_block(w, b""); stored_block(w, b"ab"); fixed_block(w, [(258, 2)], final=False); stored_block(w, b"", final=True); add("stored_fixed_stored", w)
    # overlaps of every small distance against lengths around the lanes' 64-byte step
    toks = [ord(c) for c in "abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ!?"]
    for d in (1, 2, 3, 5, 63, 64, 65):
        for l in (3, 63, 64, 65, 127, 128, 129, 258):
            toks += [(l, d), 35 + d % 7]
    w = Bits(); fixed_block(w, toks); add("overlaps", w)
    # token counts around the write-out round: literals and matches mixed; and a long run of rounds
    for n in (round_tokens - 1, round_tokens, round_tokens + 1, 2 * round_tokens, 5 * round_tokens + 3):
        toks = [97 + k % 26 if k % 3 else (3 + k % 5, 1 + k % 2) for k in range(1, n + 1)]
        w = Bits(); fixed_block(w, toks); add("tokens_%d" % n, w)
    # two dynamic blocks and a fixed one between them: the tables are rebuilt each time
    lit = chain([ord("a"), ord("b"), 256, 257, 258], 259)
    w = Bits(); dynamic_block(w, lit, [1], [97, 98, (3, 1)], final=False); fixed_block(w, [99, (5, 2)], final=False); fixed_block(w, [100], final=False)
    dynamic_block(w, chain([ord("z"), 256, 257], 258), [2, 2, 2, 2], [122, 122, (3, 4)]); add("dynamic_fixed_fixed_dynamic", w)
    # bits behind the final block's end are not looked at
    w = Bits(); fixed_block(w, [104, 105]); raw = w.bytes() + b"\xff\xff\xff"
    assert inflate_or_none(raw) == b"hi"; out["bytes_behind_the_final_block"] = (raw, b"hi")
    return out


def invalid_streams():
    """-> {name: (raw deflate stream, the INF_E_* rule)}: zlib refuses every one"""
    out = {}
    def add(name, raw, rule):
        assert inflate_or_none(raw) is None, name
        out[name] = (raw, rule)
    ok_lit = chain([ord("a"), ord("b"), 256, 257, 258], 259)
    def header_only(**kw):
        w = Bits(); dynamic_header(w, **kw); w.put(0, 32); return w.bytes()
    three = [0] * 257; three[97] = three[98] = three[256] = 1
    add("literal_set_over_subscribed", header_only(lit_lens=three, dist_lens=[1]), E_LITLEN_SET)
    two = [0] * 257; two[97] = 1; two[256] = 2
    add("literal_set_incomplete", header_only(lit_lens=two, dist_lens=[1]), E_LITLEN_SET)
    add("distance_set_over_subscribed", header_only(lit_lens=ok_lit, dist_lens=[1, 1, 1]), E_DIST_SET)
    add("distance_set_incomplete", header_only(lit_lens=ok_lit, dist_lens=[2]), E_DIST_SET)
    add("distance_set_incomplete_two_codes", header_only(lit_lens=ok_lit, dist_lens=[1, 2]), E_DIST_SET)
    add("code_length_set_over_subscribed", header_only(lit_lens=ok_lit, dist_lens=[1], clc_lens=[1, 1, 1] + [0] * 16), E_CODELEN_SET)
    add("code_length_set_incomplete", header_only(lit_lens=ok_lit, dist_lens=[1], clc_lens=[1] + [0] * 18), E_CODELEN_SET)
    add("code_length_set_empty", header_only(lit_lens=ok_lit, dist_lens=[1], clc_lens=[0] * 19), E_CODELEN_SET)
    no_eob = [0] * 257; no_eob[97] = no_eob[98] = 1
    add("no_end_of_block_code", header_only(lit_lens=no_eob, dist_lens=[1]), E_NO_EOB)
    add("repeat_without_a_previous_length", header_only(lit_lens=ok_lit, dist_lens=[1], cl_syms=[(16, 2, 0)]), E_REPEAT)
    add("repeat_past_the_last_length", header_only(lit_lens=ok_lit, dist_lens=[1], cl_syms=[(18, 7, 127), (18, 7, 127)]), E_REPEAT)
    add("repeat_16_past_the_last_length", header_only(lit_lens=[0] * 257, dist_lens=[0], cl_syms=[(18, 7, 127), (18, 7, 105), (3, 0, 0), (16, 2, 3)]), E_REPEAT)
    add("too_many_length_symbols", header_only(lit_lens=ok_lit, dist_lens=[1], hlit=30), E_SYMBOLS)
    add("too_many_distance_symbols", header_only(lit_lens=ok_lit, dist_lens=[1], hdist=30), E_SYMBOLS)
    w = Bits(); w.put(1, 1); w.put(3, 2); w.put(0, 29); add("block_type_3", w.bytes(), E_BTYPE)
    w = Bits(); fixed_block(w, [97], final=False); w.put(1, 1); w.put(3, 2); w.put(0, 29); add("block_type_3_behind_a_block", w.bytes(), E_BTYPE)
    w = Bits(); stored_block(w, b"abc", final=True, nlen=0xfffd); add("stored_len_and_nlen_disagree", w.bytes(), E_STORED)
    for s in (286, 287):
        w = Bits(); fixed_block(w, [97, ("sym", s), 98]); add("literal_length_symbol_%d" % s, w.bytes(), E_LITLEN_CODE)
    for s in (30, 31):
        w = Bits(); fixed_block(w, [97, 98, 99, ("dsym", 3, s), 98]); add("distance_symbol_%d" % s, w.bytes(), E_DIST_CODE)
    w = Bits(); fixed_block(w, [(3, 1)]); add("distance_before_the_first_byte", w.bytes(), E_FAR)
    w = Bits(); fixed_block(w, [97, 98, 99, (3, 4)]); add("distance_one_too_far", w.bytes(), E_FAR)
    w = Bits(); stored_block(w, b"abc"); fixed_block(w, [100, (5, 5)]); add("distance_too_far_behind_a_stored_block", w.bytes(), E_FAR)
    # a bit pattern without a code in the two sets zlib lets be incomplete
    lit = [0] * 257; lit[256] = 1
    w = Bits(); dynamic_header(w, lit, [0]); w.put(1, 1); w.put(0, 31); add("bits_that_are_no_literal_code", w.bytes(), E_LITLEN_CODE)
    w = Bits(); dynamic_header(w, ok_lit, [1]); lc = canon(ok_lit); w.code(*lc[97]); w.code(*lc[257]); w.put(1, 1); w.put(0, 31)
    add("bits_that_are_no_distance_code", w.bytes(), E_DIST_CODE)
    w2 = Bits(); dynamic_header(w2, ok_lit, [0]); w2.code(*lc[97]); w2.code(*lc[257]); w2.put(0, 32); add("a_match_without_any_distance_code", w2.bytes(), E_DIST_CODE)
    # input that ends before the final block does: in a header, inside a token, before the end-of-block code, in a stored block, before any bit
    text = fastq_like(3000, seed=9)
    good = deflate_raw(text, 6)
    for cut in (1, 5, 40, len(good) // 2, len(good) - 1):
        add("input_ends_at_%d_of_%d" % (cut, len(good)), good[:cut], E_INPUT)
    add("no_input_at_all", b"", E_INPUT)
    w = Bits(); fixed_block(w, [97, 98], eob=False); add("no_end_of_block", w.bytes(), E_INPUT)
    w = Bits(); fixed_block(w, [97, 98], final=False); add("no_final_block", w.bytes(), E_INPUT)
    w = Bits(); stored_block(w, b"abcdef", final=True); add("stored_block_cut", w.bytes()[:-2], E_INPUT)
    w = Bits(); stored_block(w, b"abcdef", final=True); add("stored_header_cut", w.bytes()[:3], E_INPUT)
    return out


def invalid_files():
    """BGZF bytes the member walker or the trailer check refuses -> {name: (bytes, rule, member index, zlib's gzip reader must refuse it too)}"""
    a, b = fastq_like(700, 2), fastq_like(900, 3)
    ra, rb = deflate_raw(a), deflate_raw(b)
    good = member(ra, a)
    out = {
        "crc_flipped": (good + member(rb, b, crc=zlib.crc32(b) ^ 0x10), E_CRC, 1, True),
        "isize_one_more": (good + member(rb, b, isize=len(b) + 1), E_ISIZE, 1, True),
        "isize_one_less": (good + member(rb, b, isize=len(b) - 1), E_ISIZE, 1, True),
        "isize_zero": (member(rb, b, isize=0), E_ISIZE, 0, True),
        "flg_with_fname": (good + member(rb, b, flg=12), WALKER, 1, False),
        "flg_without_fextra": (good + good + member(rb, b, flg=0), WALKER, 2, False),
        "no_bc_subfield": (good + member(rb, b, extra_front=b"XY\x02\x00ab", bc=False), WALKER, 1, False),
        "no_extra_field_content": (member(rb, b, bc=False), WALKER, 0, False),
        "bsize_past_the_input": (good + member(rb, b, bsize=12 + 6 + len(rb) + 8 + 1), WALKER, 1, False),
        "bsize_inside_the_header": (member(rb, b, bsize=10), WALKER, 0, False),
        "isize_above_65536": (good + member(rb, b, isize=65537), WALKER, 1, True),
        "trailing_bytes": (good + b"\x00", WALKER, 1, False),
        "trailing_bytes_like_a_header": (good + good[:11], WALKER, 1, False),
        "other_magic": (b"\x1f\x8b\x07" + good[3:], WALKER, 0, True),
        "subfield_runs_past_the_extra_field": (member(rb, b, extra_front=b"XY\xff\x00", bc=True)[:12 + 4] + good, WALKER, 0, False),
    }
    for name, (data, rule, idx, zl) in out.items():
        if zl:
            try:
                bgzf_reference(data); refused = False
            except (zlib.error, AssertionError):
                refused = True
            assert refused, name
    return out


def as_member(raw: bytes, data: bytes | None) -> bytes:
    """a hand-made stream as one BGZF member; an invalid one promises the largest ISIZE, so that the deflate rule is what fails first"""
    return member(raw, data) if data is not None else member(raw, crc=0, isize=65536)


# ---- FASTQ through blocks: Python restatements -------------------------------------------------------------------------------------------------------
def whole_records(text: bytes):
    """-> (records, offset behind the last whole record): a record is four lines, each ended by a newline"""
    pos, n = 0, 0
    while True:
        p = pos
        for _ in range(4):
            e = text.find(b"\n", p)
            if e < 0:
                return n, pos
            p = e + 1
        pos, n = p, n + 1


def cut_records(text: bytes, k: int) -> int:
    pos = 0
    for _ in range(4 * k):
        pos = text.index(b"\n", pos) + 1
    return pos


def record_lines(text: bytes):
    """the lines of a text in fours, the last line possibly without its newline -> [[l0, l1, l2, l3]] (missing lines: b'')"""
    lines, pos = [], 0
    while pos < len(text):
        e = text.find(b"\n", pos)
        e = len(text) if e < 0 else e + 1
        lines.append(text[pos:e]); pos = e
    return [lines[i:i + 4] + [b""] * (4 - len(lines[i:i + 4])) for i in range(0, len(lines), 4)]


def unlike(rec) -> bool:
    """fast_fastq.h::gz_reader_sees_the_same on one record's four lines: True when the reference's gz reader and its plain reader would differ"""
    l0, l1, l2, l3 = rec
    if not (len(l0) >= 2 and len(l1) >= 2 and len(l2) >= 1 and len(l3) >= 1 and max(map(len, rec)) < 1024 and l0[:1] == b"@"):
        return True
    if any(0 in l for l in rec):
        return True
    p1 = next((q for q in range(len(l0)) if l0[q] not in b">@"), len(l0) - 1)
    p2 = next((q for q in range(1, len(l0)) if l0[q] in b" /\t"), len(l0) - 1)
    return p2 - p1 <= 0


# ---- the lane code on the host -----------------------------------------------------------------------------------------------------------------------
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "inflate_checks_san" if sanitize else "inflate_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "inflate_checks.hip")])
    return exe


def run_program(exe, workdir, cases):
    """cases: [BGZF bytes] -> [(verdict, member, bytes)]"""
    src = os.path.join(workdir, os.path.basename(exe) + "_in.bin"); dst = os.path.join(workdir, os.path.basename(exe) + "_out.bin")
    with open(src, "wb") as f:
        for c in cases:
            f.write(struct.pack("<I", len(c)) + c)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout, r.stderr[-3000:])
    raw, at, out = open(dst, "rb").read(), 0, []
    for _ in cases:
        v, m, n = struct.unpack_from("<iII", raw, at); at += 12
        out.append((v, m, raw[at:at + n])); at += n
    assert at == len(raw)
    return out
