"""Helpers of the BAM index tests: hand-made BAM records with real CIGAR ops, the Python twin of the index dart_amd/csrc/dg_bamidx.h defines (a sequential
restatement: the hts_idx_push walk with last_bin / save_off, then the fill, the ascending bins and the neighbour merge -- record by record, not as the
kernels' scans), an independent reader (SAM specification 5.1.1 and 5.2: reg2bins, the candidate chunks, the linear index's lower bound, records read
through the compressed stream at their virtual offsets), and the native program tests/native/bamidx_checks.hip.  The definition is the header's comment: no
samtools exists where these tests run."""
from __future__ import annotations

import os, struct, subprocess, zlib
import common, bam_decode
import bamsort_inputs as bsi

BLOCK = 0xFF00
MAX_END = 1 << 29
PSEUDO = 37450
M, I, D, N, S, H, P, EQ, X = range(9)


class RangeError(Exception):
    """a placed record ends behind 2^29 (args[0] = its index), or a file offset needs more than 48 bits"""


def record(refid, pos, flag, name=b"r", cigar=(), l_seq=0, mapq=0, tags=b"", fill=0):
    """bamsort_inputs.record with real CIGAR ops: cigar = [(len, op)]"""
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(name) + 1, mapq, 4680, len(cigar), flag, l_seq, -1, -1, 0)
    body += name + b"\0" + b"".join(struct.pack("<I", l << 4 | op) for l, op in cigar) + bytes([fill]) * ((l_seq + 1) // 2) + bytes([fill]) * l_seq + tags
    return struct.pack("<i", len(body)) + body


def fields(raw: bytes, at: int, n_chr: int):
    """-> dict(refid, pos, placed, mapped, rlen, beg, end, bin, size) of the record at `at`"""
    bs, refid, pos = struct.unpack_from("<Iii", raw, at)
    l_name = raw[at + 12]; n_cig, flag = struct.unpack_from("<HH", raw, at + 16)
    placed = 0 <= refid < n_chr; mapped = not flag & 4
    rlen = 0
    if mapped and n_cig:
        for c in struct.unpack_from("<%dI" % n_cig, raw, at + 36 + l_name):
            if c & 15 in (M, D, N, EQ, X):
                rlen += c >> 4
    end_raw = pos + (rlen if rlen else 1)
    beg = max(pos, 0); end = max(end_raw, beg + 1)
    return dict(refid=refid, pos=pos, placed=placed, mapped=mapped, rlen=rlen, beg=beg, end=end, bin=bam_decode.reg2bin(beg, end), size=4 + bs)


def offsets(raw: bytes):
    out, p = [], 0
    while p < len(raw):
        out.append(p); p += 4 + struct.unpack_from("<I", raw, p)[0]
    assert p == len(raw)
    return out


def coffs(block_sizes, first):
    c = [first]
    for s in block_sizes:
        c.append(c[-1] + s)
    if c[-1] >= 1 << 48:
        raise RangeError("file offset %d" % c[-1])
    return c


def voff(r, n_raw, coff):
    return coff[r // BLOCK] << 16 | r % BLOCK if r < n_raw else coff[-1] << 16


def walk(raw: bytes, block_sizes, first_block_offset: int, n_chr: int):
    """the hts_idx_push walk -> (per reference dict(bins = {bin: [[beg, end]]} in file order, lin = {window: voff}, mapped, unmapped, first, last_end),
    n_no_coor, per record (beg, end, bin, voff))"""
    n_raw = len(raw)
    assert len(block_sizes) == (n_raw + BLOCK - 1) // BLOCK and all(s >= 1 for s in block_sizes)
    coff = coffs(block_sizes, first_block_offset)
    refs = [dict(bins={}, lin={}, mapped=0, unmapped=0, first=None, last_end=None) for _ in range(n_chr)]
    n_no_coor, per_record = 0, []
    last_key, save_off = None, None
    for i, at in enumerate(offsets(raw)):
        f = fields(raw, at, n_chr)
        v = voff(at, n_raw, coff)
        per_record.append((f["beg"], f["end"], f["bin"], v))
        key = (f["refid"], f["bin"]) if f["placed"] else None
        if key != last_key:
            if last_key is not None:
                refs[last_key[0]]["bins"].setdefault(last_key[1], []).append([save_off, v])
            assert not (key is not None and last_key is None and i), "a placed record behind an unplaced one"
            last_key, save_off = key, v
        if not f["placed"]:
            n_no_coor += 1
            continue
        if f["end"] > MAX_END:
            raise RangeError(i)
        r = refs[f["refid"]]
        if r["first"] is None:
            r["first"] = v
        r["last_end"] = voff(at + f["size"], n_raw, coff)
        if f["mapped"]:
            r["mapped"] += 1
            for w in range(f["beg"] >> 14, ((f["end"] - 1) >> 14) + 1):
                r["lin"].setdefault(w, v)              # the first record in file order is the smallest offset
        else:
            r["unmapped"] += 1
    if last_key is not None:
        refs[last_key[0]]["bins"].setdefault(last_key[1], []).append([save_off, voff(n_raw, n_raw, coff)])
    return refs, n_no_coor, per_record


def finish(refs):
    """per reference: the bins ascending with neighbours merged, the filled linear index -> [(bins = [(bin, [(beg, end)])], intv = [voff], chunks before the merge)]"""
    out = []
    for r in refs:
        bins, before = [], 0
        for b in sorted(r["bins"]):
            merged = []
            for beg, end in r["bins"][b]:
                before += 1
                if merged and merged[-1][1] >> 16 >= beg >> 16:
                    merged[-1][1] = end
                else:
                    merged.append([beg, end])
            bins.append((b, [tuple(c) for c in merged]))
        n_intv = max(r["lin"]) + 1 if r["lin"] else 0
        intv, last = [], r["first"]
        for w in range(n_intv):
            last = r["lin"].get(w, last)
            intv.append(last)
        out.append((bins, intv, before))
    return out


def serialise(refs, done, n_no_coor):
    o = [b"BAI\1", struct.pack("<i", len(refs))]
    for r, (bins, intv, _) in zip(refs, done):
        has = r["mapped"] + r["unmapped"] > 0
        o.append(struct.pack("<i", len(bins) + (1 if has else 0)))
        for b, chunks in bins:
            o.append(struct.pack("<Ii", b, len(chunks)) + b"".join(struct.pack("<QQ", *c) for c in chunks))
        if has:
            o.append(struct.pack("<IiQQQQ", PSEUDO, 2, r["first"], r["last_end"], r["mapped"], r["unmapped"]))
        o.append(struct.pack("<i", len(intv)) + struct.pack("<%dQ" % len(intv), *intv))
    o.append(struct.pack("<Q", n_no_coor))
    return b"".join(o)


def build_bai(raw_sorted: bytes, block_sizes, first_block_offset: int, n_chr: int) -> bytes:
    refs, n_no_coor, _ = walk(raw_sorted, list(block_sizes), first_block_offset, n_chr)
    return serialise(refs, finish(refs), n_no_coor)


def twin_stats(raw_sorted: bytes, block_sizes, first_block_offset: int, n_chr: int):
    """dg_bam_index_finish's six statistics"""
    refs, n_no_coor, per_record = walk(raw_sorted, list(block_sizes), first_block_offset, n_chr)
    done = finish(refs)
    return [len(per_record) - n_no_coor, n_no_coor, sum(len(b) for b, _, _ in done), sum(x for _, _, x in done), sum(len(c) for b, _, _ in done for _, c in b),
            sum(len(i) for _, i, _ in done)]


def split_file(bam: bytes):
    """a BAM file -> (first_block_offset, the data blocks' compressed sizes, the records' bytes, n_chr); the header has blocks of its own (bam_decode asserts it)"""
    blocks = bam_decode.bgzf_blocks(bam)
    assert blocks and blocks[-1] == (b"", 28)
    blocks = blocks[:-1]
    data = b"".join(b for b, _ in blocks)
    assert data[:4] == b"BAM\1"
    p = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, p)[0]; p += 4
    for _ in range(n_ref):
        p += 4 + struct.unpack_from("<i", data, p)[0] + 4
    acc = first = k = 0
    while acc < p:
        acc += len(blocks[k][0]); first += blocks[k][1]; k += 1
    assert acc == p, "the header does not end on a block boundary"
    assert all(len(b) == BLOCK for b, _ in blocks[k:-1]) and (len(blocks) == k or 1 <= len(blocks[-1][0]) <= BLOCK)
    return first, [s for _, s in blocks[k:]], data[p:], n_ref


def build_bai_of_file(bam: bytes) -> bytes:
    first, sizes, raw, n_ref = split_file(bam)
    return build_bai(raw, sizes, first, n_ref)


def fake_file(raw: bytes, first_block_offset: int = 0):
    """the records as stored BGZF blocks behind `first_block_offset` bytes that are never read -> (file bytes, block sizes): what `query` reads in the CPU tests"""
    out, sizes = [bytes(first_block_offset)], []
    for p in range(0, len(raw), BLOCK):
        d = raw[p:p + BLOCK]
        z = zlib.compressobj(6, zlib.DEFLATED, -15); body = z.compress(d) + z.flush()
        blk = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(body) + 8 - 1) + body + struct.pack("<II", zlib.crc32(d) & 0xFFFFFFFF, len(d))
        out.append(blk); sizes.append(len(blk))
    return b"".join(out), sizes


# ---- the reader: independent of the twin's walk ----
def parse_bai(b: bytes):
    """-> dict(refs = [dict(bins = [(bin, [(beg, end)])] in file order, pseudo = None or (first, last_end, mapped, unmapped), intv = [voff])], n_no_coor)"""
    assert b[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", b, 4)[0]; p = 8
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", b, p)[0]; p += 4
        bins, pseudo = [], None
        for _ in range(n_bin):
            num, n_chunk = struct.unpack_from("<Ii", b, p); p += 8
            chunks = [struct.unpack_from("<QQ", b, p + 16 * k) for k in range(n_chunk)]; p += 16 * n_chunk
            if num == PSEUDO:
                assert n_chunk == 2 and pseudo is None
                pseudo = chunks[0] + chunks[1]
            else:
                assert num < PSEUDO and n_chunk >= 1
                bins.append((num, chunks))
        n_intv = struct.unpack_from("<i", b, p)[0]; p += 4
        intv = list(struct.unpack_from("<%dQ" % n_intv, b, p)); p += 8 * n_intv
        refs.append(dict(bins=bins, pseudo=pseudo, intv=intv))
    n_no_coor = struct.unpack_from("<Q", b, p)[0]; p += 8
    assert p == len(b), "bytes behind the index"
    return dict(refs=refs, n_no_coor=n_no_coor)


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(base + (beg >> shift), base + (end >> shift) + 1)
    return out


class _Bgzf:
    def __init__(self, data):
        self.data, self.cache = data, {}

    def block(self, coff):
        if coff not in self.cache:
            d = self.data
            assert d[coff:coff + 4] == b"\x1f\x8b\x08\x04" and d[coff + 12:coff + 14] == b"BC", "no BGZF block at %d" % coff
            bsize = struct.unpack_from("<H", d, coff + 16)[0] + 1
            self.cache[coff] = (zlib.decompress(d[coff + 18:coff + bsize - 8], -15), bsize)
        return self.cache[coff]

    def read(self, v, n):
        """n bytes from virtual offset v -> (bytes, the virtual offset behind them as bgzf_tell gives it)"""
        coff, u = v >> 16, v & 0xFFFF
        out = b""
        while True:
            blk, bsize = self.block(coff)
            take = blk[u:u + n - len(out)]
            out += take; u += len(take)
            if u == len(blk):
                coff += bsize; u = 0
            if len(out) == n:
                return out, coff << 16 | u
            assert len(take) or len(blk), "read behind the data"


def overlaps(f, tid, beg, end):
    return f["refid"] == tid and f["mapped"] and f["beg"] < end and f["end"] > beg


def query(bai: bytes, bam: bytes, tid: int, beg: int, end: int):
    """the mapped records of reference tid that overlap [beg, end), in file order, found the textbook way.  (Placed unmapped records do not touch the linear
    index, so no reader is promised them: they are left out here and in `brute`.)"""
    ix = parse_bai(bai)
    ref = ix["refs"][tid]
    want = set(reg2bins(beg, end))
    chunks = [c for num, cs in ref["bins"] if num in want for c in cs]
    w = beg >> 14
    min_off = ref["intv"][w] if w < len(ref["intv"]) else 0
    chunks = sorted(c for c in chunks if c[1] > min_off)
    z = _Bgzf(bam)
    found = {}
    for cb, ce in chunks:
        v = cb
        while v < ce:
            head, v1 = z.read(v, 4)
            body, v2 = z.read(v1, struct.unpack("<I", head)[0])
            rec = head + body
            if overlaps(fields(rec, 0, len(ix["refs"])), tid, beg, end):
                found[v] = rec
            v = v2
    return [found[v] for v in sorted(found)]


def scan(raw: bytes, n_chr: int):
    """every record's fields and bytes, once, for many `brute` calls"""
    return [(f, raw[at:at + f["size"]]) for at in offsets(raw) for f in [fields(raw, at, n_chr)]]


def brute(raw: bytes, n_chr: int, tid: int, beg: int, end: int, scanned=None):
    return [rec for f, rec in (scanned if scanned is not None else scan(raw, n_chr)) if overlaps(f, tid, beg, end)]


# ---- the crafted records of the CPU suite: name -> (n_chr, sorted records, first_block_offset) ----
def crafted_cases():
    big = lambda tid, pos, n, cigar: record(tid, pos, 0, b"big%d" % n, cigar, l_seq=100, tags=b"ZZZ" + b"t" * 3000 + b"\0")
    ops = [(5, S), (10, M), (2, I), (3, D), (700, N), (4, EQ), (1, X), (6, P), (7, H)]            # every op code 0..8: rlen = 10 + 3 + 700 + 4 + 1
    main = [
        record(0, -1, 0, b"pos_m1", [(10, M)], l_seq=10),                       # pos -1, mapped: beg 0, end 9
        record(0, -1, 4, b"pos_m1_unmapped_placed"),
        record(0, 0, 0, b"pos0", [(50, M)], l_seq=50),
        record(0, 0, 0, b"no_cigar_mapped"),                                     # n_cigar_op = 0 on a mapped record: one base
        record(0, 100, 0, b"all_ops", ops, l_seq=22),
        record(0, 100, 0, b"n" * 254, [(30, M)], l_seq=30),                      # a name of 254 bytes in front of the CIGAR
        record(0, 16384 - 100, 0, b"ends_at_16k", [(100, M)], l_seq=100),        # end exactly at the boundary: one window
        record(0, 16384 - 100, 16, b"crosses_16k_by_one", [(101, M)], l_seq=101),
        record(0, 20000, 4, b"placed_unmapped", l_seq=20),
        record(0, 20000, 0, b"spliced", [(50, M), (60000, N), (51, M)], l_seq=101),        # several windows, a level-4 bin
        record(0, (1 << 26) - 10, 0, b"spans_level1", [(20, M)], l_seq=20),      # bin 0
        record(0, (1 << 26) + 5 * 16384, 0, b"after_a_gap", [(20, M)], l_seq=20),        # windows filled from their predecessor in front of it
        record(0, MAX_END - 40, 0, b"ends_at_2_29", [(40, M)], l_seq=40),        # end = 2^29: accepted
        # reference 1 has no records
        record(2, 5 * 16384 + 7, 16, b"late_start", [(30, M)], l_seq=30),        # leading empty windows: the reference's first record's start
        record(2, 5 * 16384 + 7, 0 | 4, b"placed_unmapped_2"),
        record(-1, -1, 4, b"unplaced"), record(-1, 55, 4, b"unplaced_with_pos"),
    ]
    main = sorted(main, key=lambda r: bsi.key(r, 3))
    # two bins in turn (a 16 kb bin, and its parent for the records with an intron across the boundary): every chunk is one record of ~3 KB, so a bin's
    # neighbours merge inside a block and stay apart across a block's end; a record that ends exactly at a block's end and one that straddles
    spread = [big(0, 10 + k, k, [(50, M), (20000, N), (50, M)] if k & 1 else [(100, M)]) for k in range(60)]
    assert spread == sorted(spread, key=lambda r: bsi.key(r, 2))
    size = sum(len(r) for r in spread)
    pad = BLOCK - size % BLOCK
    filler = record(1, 0, 0, b"filler", [(1, M)], l_seq=1, tags=b"ZZZ" + b"t" * (pad - 36 - 7 - 4 - 4 - 2) + b"\0") if pad >= 64 else b""
    spread2 = spread + ([filler] if filler else []) + [record(1, 7, 0, b"behind_the_block", [(9, M)], l_seq=9)]
    assert not filler or sum(len(r) for r in spread2[:-1]) % BLOCK == 0
    return {
        "main": (3, main, 0),
        "main_far": (3, main, 1 << 40),                                          # offsets need 48 bits
        "spread": (2, spread2, 12345),
        "unplaced_only": (2, [record(-1, -1, 4, b"u%d" % k, l_seq=10) for k in range(5)], 77),
        "empty": (4, [], 99),
        "one": (2, [record(1, 7, 16, b"only", [(5, M)], l_seq=5)], 0),
    }


def stored_sizes(raw: bytes, seed: int = 5):
    """made-up compressed sizes, all different, for inputs whose blocks are never read"""
    n = (len(raw) + BLOCK - 1) // BLOCK
    return [1000 + (seed * 7919 + k * 104729) % 60000 for k in range(n)]


# ---- the native program ----
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "bamidx_checks_san" if sanitize else "bamidx_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "bamidx_checks.hip")])
    return exe


def run_program(exe, workdir, tag, n_chr, raw, block_sizes, first_block_offset):
    """-> dict(recs = [(beg, end, bin, voff)], chunks = [(key, beg, end)] sorted, before the merge, merged = the same after it, lin = {(ref, window): voff} as filled,
    bad = index of the first record out of range or None, bytes = the index)"""
    src = os.path.join(workdir, "bamidx_%s.in" % tag); txt = os.path.join(workdir, "bamidx_%s.txt" % tag); out = os.path.join(workdir, "bamidx_%s.bai" % tag)
    with open(src, "wb") as f:
        f.write(struct.pack("<qQqq", n_chr, first_block_offset, len(raw), len(block_sizes)))
        sz = struct.pack("<%dI" % len(block_sizes), *block_sizes)
        f.write(sz + bytes(-len(sz) % 8) + raw)
    r = subprocess.run([exe, src, txt, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    res = dict(recs=[], chunks=[], merged=[], lin={}, bad=None, bytes=open(out, "rb").read())
    for line in open(txt).read().splitlines():
        w = line.split()
        if w[0] == "rec":
            res["recs"].append(tuple(int(x) for x in w[2:6]))
        elif w[0] in ("chunk", "merged"):
            res["chunks" if w[0] == "chunk" else "merged"].append(tuple(int(x) for x in w[1:4]))
        elif w[0] == "lin":
            res["lin"][(int(w[1]), int(w[2]))] = int(w[3])
        elif w[0] == "bad":
            res["bad"] = int(w[1])
    return res
