"""Helpers of the QC tests: the sequential Python twin of the definition in dart_amd/csrc/dg_qc.h (one record at a time, one base at a time), a second, independent
restatement (every record expanded to per-base tuples with a plain CIGAR expansion, counted in dictionaries), the text (text_of), record builders with explicit
bases, qualities and mate fields, hand-made cases that each hold what they are named for, and the native program tests/native/qc_checks.hip.  The definition is
the header's comment: no samtools exists where these tests run."""
from __future__ import annotations

import collections, os, struct, subprocess
import numpy as np
import common
import pileup_inputs as pui
from pileup_inputs import NIBBLE, Ref, offsets, read_of
from bamidx_inputs import M, I, D, N, S, H, P, EQ, X

CYCLES, ISIZE, INDEL = 512, 8001, 65
DEFAULT_EXCLUDE = 0x904
FILTERS = [(DEFAULT_EXCLUDE, 0), (0x704, 0), (4, 0), (DEFAULT_EXCLUDE, 4)]
SN_NAMES = ["records", "malformed", "profiled", "left_out", "bases", "profiled_bases", "aligned", "mismatches", "inserted_bases", "deleted_bases", "clipped", "n_ops",
            "skipped_bases", "bases_without_quality", "quality_sum", "pairs"]
FS_NAMES = ["total", "primary", "secondary", "supplementary", "duplicates", "primary_duplicates", "mapped", "primary_mapped", "paired", "read1", "read2", "properly_paired",
            "with_mate_mapped", "singletons", "mate_on_other_chr", "mate_on_other_chr_mapq5"]
SN = {n: k for k, n in enumerate(SN_NAMES)}
INT32_MIN = -(1 << 31)


def layout(n_chr):
    """section name -> (first word, shape); "words" -> their number"""
    out, at = {}, 0
    for name, shape in (("FS", (2, 16)), ("CH", (n_chr + 1, 2)), ("MQ", (256,)), ("IS", (3, ISIZE)), ("RL", (2, CYCLES)), ("PC", (2, 12, CYCLES)), ("ID", (2, INDEL)), ("SN", (32,))):
        out[name] = (at, shape); at += int(np.prod(shape))
    out["words"] = at
    return out


def views(words, n_chr):
    lay = layout(n_chr)
    assert len(words) == lay["words"]
    return {k: words[v[0]:v[0] + int(np.prod(v[1]))].reshape(v[1]) for k, v in lay.items() if k != "words"}


def record(tid, pos, flag, name, cigar, seq, mapq=30, qual=None, next_tid=-1, next_pos=-1, tlen=0, l_seq=None, tags=b"", block_size=None):
    """a BAM record with explicit bases (a string over =ACMGRSVTWYHKDBN), qualities (bytes, one value, or None = 30 everywhere) and mate fields"""
    nib = [NIBBLE[c] for c in seq] + [0]
    packed = bytes(nib[k] << 4 | nib[k + 1] for k in range(0, len(seq), 2))
    q = bytes([30]) * len(seq) if qual is None else bytes([qual]) * len(seq) if isinstance(qual, int) else bytes(qual)
    assert len(q) == len(seq)
    ls = len(seq) if l_seq is None else l_seq
    body = struct.pack("<iiBBHHHIiii", tid, pos, len(name) + 1, mapq, 4680, len(cigar), flag, ls, next_tid, next_pos, tlen)
    body += name + b"\0" + b"".join(struct.pack("<I", l << 4 | op) for l, op in cigar) + packed + q + tags
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def rec_on(ref, tid, pos, flag, name, cigar, edits=(), mapq=30, **kw):
    return record(tid, pos, flag, name, cigar, read_of(ref, tid, pos, cigar, edits), mapq, **kw)


# ---- the twin ----
def twin(raw: bytes, ref: Ref, exclude=DEFAULT_EXCLUDE, min_mapq=0):
    """-> the words (numpy uint64), record by record, base by base"""
    n_chr = ref.n_chr
    words = [0] * layout(n_chr)["words"]
    lay = layout(n_chr)

    def add(sec, idx, v=1):
        at, shape = lay[sec]
        flat = 0
        for i, n in zip(idx, shape):
            assert 0 <= i < n
            flat = flat * n + i
        words[at + flat] += v

    for at in offsets(raw):
        add("SN", (SN["records"],))
        avail = len(raw) - at
        whole = False
        if avail >= 36:
            bs, refid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, next_refid, next_pos, tlen = struct.unpack_from("<IiiBBHHHIiii", raw, at)
            size = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
            whole = size <= 4 + bs and size <= avail
        if not whole:
            add("SN", (SN["malformed"],)); continue
        fail, primary, mapped = flag >> 9 & 1, not flag & 0x900, not flag & 4
        rows = [0]
        if primary: rows.append(1)
        if flag & 0x100: rows.append(2)
        elif flag & 0x800: rows.append(3)
        if flag & 0x400: rows += [4, 5] if primary else [4]
        if mapped: rows += [6, 7] if primary else [6]
        if primary and flag & 1:
            rows.append(8)
            if flag & 0x40: rows.append(9)
            if flag & 0x80: rows.append(10)
            if flag & 2 and mapped: rows.append(11)
            if mapped and not flag & 8:
                rows.append(12)
                if next_refid != refid:
                    rows.append(14)
                    if mapq >= 5: rows.append(15)
            if mapped and flag & 8: rows.append(13)
        for r in rows:
            add("FS", (fail, r))
        add("CH", (refid if 0 <= refid < n_chr else n_chr, 0 if mapped else 1))
        if primary and mapped:
            add("MQ", (mapq,))
        if primary and mapped and flag & 1 and not flag & 8 and flag & 0x40 and next_refid == refid and tlen != 0:
            a, b = flag >> 4 & 1, flag >> 5 & 1
            f, r = (pos, next_pos) if a == 0 else (next_pos, pos)
            add("IS", (2 if a == b else 0 if f <= r else 1, min(abs(tlen), ISIZE - 1))); add("SN", (SN["pairs"],))
        if primary:
            add("RL", (flag >> 7 & 1, min(l_seq, CYCLES - 1))); add("SN", (SN["bases"],), l_seq)
        c = pui.classify(raw, at, ref, exclude, min_mapq)
        if c[0] in ("left_out", "range"):
            add("SN", (SN["left_out"],))
        if c[0] != "counted":
            continue
        add("SN", (SN["profiled"],))
        _, refid, pos, s, cigar, nib = c
        k = flag >> 7 & 1
        qual_at = at + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
        cyc = lambda i: min(l_seq - 1 - i if s else i, CYCLES - 1)

        def base(i, cls, p):
            n, q = nib[i], raw[qual_at + i]
            rb = ref.base(refid, p) if cls == "M" else None
            if n in (1, 2, 4, 8):
                code = {1: 0, 2: 1, 4: 2, 8: 3}[n]
                col, mism = 3 - code if s else code, cls == "M" and code != rb
            elif n == 0 and cls == "M":
                col, mism = 3 - rb if s else rb, False
            else:
                col, mism = 4, cls == "M"
            add("PC", (k, col, cyc(i))); add("SN", (SN["profiled_bases"],))
            if q == 0xff:
                add("SN", (SN["bases_without_quality"],))
            else:
                add("PC", (k, 5, cyc(i)), q); add("SN", (SN["quality_sum"],), q)
            add("PC", (k, {"M": 6, "I": 8, "S": 9}[cls], cyc(i))); add("SN", (SN[{"M": "aligned", "I": "inserted_bases", "S": "clipped"}[cls]],))
            if mism:
                add("PC", (k, 7, cyc(i))); add("SN", (SN["mismatches"],))

        p, q = pos, 0
        for w in cigar:
            op, ln = w & 15, w >> 4
            if op in (M, EQ, X):
                for j in range(ln):
                    base(q + j, "M", p + j)
                p += ln; q += ln
            elif op == I:
                if ln:
                    add("PC", (k, 10, cyc(q))); add("ID", (0, min(ln, INDEL - 1)))
                for j in range(ln):
                    base(q + j, "I", None)
                q += ln
            elif op == S:
                for j in range(ln):
                    base(q + j, "S", None)
                q += ln
            elif op == D:
                if ln:
                    add("PC", (k, 11, cyc(max(q, 1) - 1))); add("ID", (1, min(ln, INDEL - 1))); add("SN", (SN["deleted_bases"],), ln)
                p += ln
            elif op == N:
                if ln:
                    add("SN", (SN["n_ops"],)); add("SN", (SN["skipped_bases"],), ln)
                p += ln
    return np.array(words, dtype=np.uint64)


# ---- the independent restatement ----
def naive(raw: bytes, ref: Ref, exclude=DEFAULT_EXCLUDE, min_mapq=0):
    """every record expanded to per-base tuples (cycle, set of columns) with a plain CIGAR expansion, counted with dictionaries; its own field reads, its own
    flag names.  -> the words"""
    n_chr = ref.n_chr
    cnt = collections.Counter()
    pos_of = 0
    while pos_of + 4 <= len(raw):
        rec = raw[pos_of:]
        block = int.from_bytes(rec[0:4], "little")
        pos_of += 4 + block
        cnt["SN", 0] += 1
        if len(rec) < 36:
            cnt["SN", 1] += 1; continue
        i32 = lambda o: int.from_bytes(rec[o:o + 4], "little", signed=True)
        tid, pos, l_name, mapq, n_cig, flag, l_seq, mtid, mpos, tlen = i32(4), i32(8), rec[12], rec[13], rec[16] | rec[17] << 8, rec[18] | rec[19] << 8, int.from_bytes(rec[20:24], "little"), i32(24), i32(28), i32(32)
        need = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        if need > 4 + block or need > len(rec):
            cnt["SN", 1] += 1; continue
        bit = {"paired": 1, "proper": 2, "unmapped": 4, "mate_unmapped": 8, "reverse": 16, "mate_reverse": 32, "read1": 64, "read2": 128, "secondary": 256, "fail": 512, "dup": 1024, "supp": 2048}
        has = {n for n, b in bit.items() if flag & b}
        prim = not has & {"secondary", "supp"}
        mapped = "unmapped" not in has
        fs = {"total"}
        fs |= {"primary"} if prim else set()
        fs |= {"secondary"} if "secondary" in has else {"supplementary"} if "supp" in has else set()
        if "dup" in has: fs |= {"duplicates"} | ({"primary_duplicates"} if prim else set())
        if mapped: fs |= {"mapped"} | ({"primary_mapped"} if prim else set())
        if prim and "paired" in has:
            fs.add("paired")
            fs |= {n for n in ("read1", "read2") if n in has}
            if "proper" in has and mapped: fs.add("properly_paired")
            if mapped and "mate_unmapped" in has: fs.add("singletons")
            if mapped and "mate_unmapped" not in has:
                fs.add("with_mate_mapped")
                if mtid != tid:
                    fs.add("mate_on_other_chr")
                    if mapq > 4: fs.add("mate_on_other_chr_mapq5")
        for n in fs:
            cnt["FS", 1 if "fail" in has else 0, FS_NAMES.index(n)] += 1
        cnt["CH", tid if tid in range(n_chr) else n_chr, 0 if mapped else 1] += 1
        if prim and mapped:
            cnt["MQ", mapq] += 1
        if prim and mapped and {"paired", "read1"} <= has and "mate_unmapped" not in has and mtid == tid and tlen:
            rv, mrv = "reverse" in has, "mate_reverse" in has
            if rv == mrv: row = 2
            else:
                fwd, rev = (mpos, pos) if rv else (pos, mpos)
                row = 1 if fwd > rev else 0
            cnt["IS", row, min(-tlen if tlen < 0 else tlen, 8000)] += 1; cnt["SN", 15] += 1
        if prim:
            cnt["RL", 1 if "read2" in has else 0, min(l_seq, 511)] += 1; cnt["SN", 4] += l_seq
        # the profile: the allele counts' conditions, restated
        if not (tid in range(n_chr) and pos >= 0 and mapped and n_cig > 0 and not flag & exclude and mapq >= min_mapq):
            continue
        ops = [(int.from_bytes(rec[36 + l_name + 4 * j:40 + l_name + 4 * j], "little") >> 4, "MIDNSHP=X???????"[rec[36 + l_name + 4 * j] & 15]) for j in range(n_cig)]
        end, beyond = pos, False
        for ln, o in ops:
            if o in "M=XDN":
                end += ln
                if o in "M=X" and ln and end > (1 << 32) - 1: beyond = True
        if beyond:
            cnt["SN", 3] += 1; continue
        if l_seq == 0:
            continue
        if sum(ln for ln, o in ops if o in "MIS=X") != l_seq or end > ref.chr_len[tid]:
            cnt["SN", 3] += 1; continue
        cnt["SN", 2] += 1
        expanded = "".join(o * ln for ln, o in ops if o in "MIS=X")
        sq = 36 + l_name + 4 * n_cig
        letters = ["=ACMGRSVTWYHKDBN"[rec[sq + j // 2] >> 4 if j % 2 == 0 else rec[sq + j // 2] & 15] for j in range(l_seq)]
        quals = rec[sq + (l_seq + 1) // 2:sq + (l_seq + 1) // 2 + l_seq]
        rv = 1 if flag & 16 else 0
        k = 1 if flag & 128 else 0
        cycle = [min(l_seq - 1 - j, 511) if rv else min(j, 511) for j in range(l_seq)]
        refpos, p = [None] * l_seq, pos
        j = 0
        for ln, o in ops:
            if o in "M=X":
                for t in range(ln): refpos[j + t] = p + t
            if o in "M=XDN": p += ln
            if o in "MIS=X": j += ln
        comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
        tuples = []
        for j in range(l_seq):
            cols = set()
            al = expanded[j] in "M=X"
            r = "ACGT"[ref.base(tid, refpos[j])] if al else None
            seen = letters[j] if letters[j] in "ACGT" else r if (letters[j] == "=" and al) else None
            cols.add("ACGT".index(comp[seen] if rv else seen) if seen else 4)
            cols.add(6 if al else 8 if expanded[j] == "I" else 9)
            if al and (letters[j] not in "ACGT=" or (letters[j] in "ACGT" and letters[j] != r)): cols.add(7)
            tuples.append((cycle[j], cols, quals[j]))
        for c, cols, q in tuples:
            for col in cols:
                cnt["PC", k, col, c] += 1
            cnt["PC", k, 5, c] += 0 if q == 255 else q
            cnt["SN", 5] += 1; cnt["SN", 13] += q == 255; cnt["SN", 14] += 0 if q == 255 else q
            cnt["SN", 6] += 6 in cols; cnt["SN", 7] += 7 in cols; cnt["SN", 8] += 8 in cols; cnt["SN", 10] += 9 in cols
        j = 0
        for ln, o in ops:
            if ln and o == "I": cnt["PC", k, 10, cycle[j]] += 1; cnt["ID", 0, min(ln, 64)] += 1
            if ln and o == "D": cnt["PC", k, 11, cycle[max(j, 1) - 1]] += 1; cnt["ID", 1, min(ln, 64)] += 1; cnt["SN", 9] += ln
            if ln and o == "N": cnt["SN", 11] += 1; cnt["SN", 12] += ln
            if o in "MIS=X": j += ln
    lay = layout(n_chr)
    words = np.zeros(lay["words"], np.uint64)
    for key, v in cnt.items():
        at, shape = lay[key[0]]
        words[at + int(np.ravel_multi_index(key[1:], shape))] = v
    return words


# ---- the text ----
def derived(words, n_chr):
    w = [int(x) for x in words]
    lay = layout(n_chr)
    sn = w[lay["SN"][0]:lay["SN"][0] + 32]
    is_at = lay["IS"][0]
    tot = [w[is_at + b] + w[is_at + ISIZE + b] + w[is_at + 2 * ISIZE + b] for b in range(ISIZE)]
    div = lambda a, b: a // b if b else 0
    n_below = sum(tot[:ISIZE - 1])
    pairs, run, median = sn[15], 0, 0
    if pairs:
        for b in range(ISIZE):
            run += tot[b]
            if run >= (pairs + 1) // 2:
                median = b; break
    return [("error_ppm", div(sn[7] * 10 ** 6, sn[6])), ("mean_quality_milli", div(sn[14] * 1000, sn[5] - sn[13])),
            ("insert_mean_milli", div(sum(b * n for b, n in enumerate(tot[:ISIZE - 1])) * 1000, n_below)), ("insert_median", median)]


def text_of(words, names, lengths) -> bytes:
    n_chr = len(names)
    w = [int(x) for x in words]
    lay = layout(n_chr)
    sec = lambda name: w[lay[name][0]:lay[name][0] + int(np.prod(lay[name][1]))]
    fs, ch, mq, is_, rl, pc, id_, sn = (sec(n) for n in ("FS", "CH", "MQ", "IS", "RL", "PC", "ID", "SN"))
    out = []
    tab = lambda *x: out.append("\t".join(str(y) for y in x))
    for k, n in enumerate(SN_NAMES): tab("SN", n, sn[k])
    for n, v in derived(words, n_chr): tab("SN", n, v)
    for k, n in enumerate(FS_NAMES): tab("FS", n, fs[k], fs[16 + k])
    for t in range(n_chr + 1):
        nm = names[t] if t < n_chr else b"*"
        tab("CH", nm.decode() if isinstance(nm, bytes) else nm, int(lengths[t]) if t < n_chr else 0, ch[2 * t], ch[2 * t + 1])
    for q in range(256):
        if mq[q]: tab("MQ", q, mq[q])
    for b in range(ISIZE):
        if is_[b] or is_[ISIZE + b] or is_[2 * ISIZE + b]: tab("IS", b, is_[b], is_[ISIZE + b], is_[2 * ISIZE + b])
    for b in range(CYCLES):
        if rl[b] or rl[CYCLES + b]: tab("RL", b, rl[b], rl[CYCLES + b])
    for k in range(2):
        rows = [[pc[(k * 12 + col) * CYCLES + c] for col in range(12)] for c in range(CYCLES)]
        last = max([c for c in range(CYCLES) if any(rows[c])], default=-1)
        for c in range(last + 1): tab("PC", "last" if k else "first", c + 1, *rows[c])
    for b in range(INDEL):
        if id_[b] or id_[INDEL + b]: tab("ID", b, id_[b], id_[INDEL + b])
    return ("\n".join(out) + "\n").encode()


# ---- hand-made cases ----
REF = pui.random_ref(11, [3000, 2000])
NAMES = [b"chrA", b"b"]
LENGTHS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 700]
BIG_LENGTHS = [16383, 16384, 16385]


def quals_of(n, salt=0):
    """n quality bytes that move along the read, with 0, 93 and 0xff among them"""
    q = bytearray((7 * i + salt) % 94 for i in range(n))
    for i, v in ((0, 0), (n // 2, 93), (n - 1, 0xff), (n // 3, 0xff)):
        if n > 3 or i == 0: q[i] = v
    return bytes(q)


def liar(R=REF):
    """n_cigar_op says 60000 ops, block_size holds one: not whole (dg_bam_sort_add refuses it: only the lane code's tests see it)"""
    r = bytearray(rec_on(R, 0, 50, 0x43, b"liar", [(10, M)], {3: "!"}, next_tid=0, next_pos=90, tlen=50)); struct.pack_into("<H", r, 16, 60000)
    return bytes(r)


def crafted_cases(R=REF, names=NAMES):
    """name -> records, all on R (two chromosomes of at least 3000 and 2000 bases)"""
    L0, L1 = R.chr_len[0], R.chr_len[1]
    flags4 = [0x43, 0x93, 0x53, 0x83]                                  # read1 fwd, read2 rev, read1 rev, read2 fwd
    lengths = []
    for n, L in enumerate(LENGTHS + [0]):
        for v in range(2):
            name = (b"n%d" % (n % 10) + b"xxxxxxx")[:1 + (n + 5 * v) % 8]      # names of 1 .. 8 letters: odd and even places of the bases and the qualities
            flag = flags4[(n + 2 * v) % 4]
            if L == 0:
                lengths.append(record(0, 10, flag, name, [(10, M)], "", l_seq=0)); continue
            cigar = [(L, M)] if v == 0 or L < 5 else [(2, S), (L - 3, M), (1, S)]
            edits = {j: "!" for j in {0, L - 1, L // 2, min(255, L - 1), min(256, L - 1)}} if v == 0 else {j: c for j, c in ((2, "!"), (L - 2, "N"), (L // 2, "=")) if 0 <= j < L}
            lengths.append(rec_on(R, 0, 40 + 3 * n, flag, name, cigar, edits, qual=quals_of(L, n), next_tid=0, next_pos=40, tlen=(1 if v else -1) * (200 + n)))
    big = [rec_on(R, 1, 10, flags4[k], b"big%d" % k, [(3, S), (900, M), (L - 903 - 900, I), (900, M)], {5: "!", L - 1: "!", 1000: "=", 1800: "N"}, qual=quals_of(L, k))
           for k, L in enumerate(BIG_LENGTHS)]
    ops = [
        rec_on(R, 0, 100, 0, b"i_first", [(3, I), (20, M)], {1: "=", 5: "="}), rec_on(R, 0, 100, 16, b"i_first_rev", [(3, I), (20, M)], {0: "N"}),
        rec_on(R, 0, 150, 0, b"i_last", [(20, M), (3, I)], {21: "R"}), rec_on(R, 0, 150, 0x91, b"i_last_rev", [(20, M), (3, I)]),
        rec_on(R, 0, 200, 0, b"d_n", [(10, M), (5, D), (10, M), (300, N), (10, M)], {9: "!", 10: "!"}), rec_on(R, 0, 200, 16, b"d_n_rev", [(10, M), (5, D), (10, M), (300, N), (10, M)], {29: "!"}),
        rec_on(R, 0, 260, 0, b"d_first", [(4, D), (10, M)]), rec_on(R, 0, 260, 16, b"d_behind_clip", [(2, S), (4, D), (10, M)]),
        rec_on(R, 0, 300, 0, b"zero_ops", [(0, M), (5, M), (0, I), (0, D), (0, N), (5, M), (0, S)], {0: "!"}),
        rec_on(R, 0, 350, 0, b"all_ops", [(7, H), (5, S), (10, M), (2, I), (3, D), (70, N), (4, EQ), (1, X), (6, P), (2, S), (7, H)], {1: "=", 7: "!", 11: "=", 16: "=", 20: "="}),
        rec_on(R, 0, 350, 16, b"all_ops_rev", [(7, H), (5, S), (10, M), (2, I), (3, D), (70, N), (4, EQ), (1, X), (6, P), (2, S), (7, H)], {1: "=", 7: "!", 11: "=", 16: "=", 20: "="}),
        rec_on(R, 0, 400, 0, b"iupac", [(16, M)], dict(zip(range(16), "=ACMGRSVTWYHKDBN"))), rec_on(R, 0, 400, 16, b"iupac_rev", [(16, M)], dict(zip(range(16), "=ACMGRSVTWYHKDBN"))),
        rec_on(R, 0, 420, 0, b"eq_x", [(8, EQ), (8, X)], {3: "!", 12: "="}),
    ]
    for k, L in enumerate((63, 64, 65, 200)):
        ops.append(rec_on(R, 0, 500 + 10 * k, 0x43 if k & 1 else 0x93, b"ins%d" % L, [(10, M), (L, I), (10, M)], qual=quals_of(20 + L, k)))
        ops.append(rec_on(R, 1, 500 + 10 * k, 0x53 if k & 1 else 0x83, b"del%d" % L, [(10, M), (L, D), (10, M)]))
    ends = [rec_on(R, 0, 0, 0, b"first0", [(9, M)], {0: "!"}), rec_on(R, 0, L0 - 9, 16, b"last0", [(9, M)], {8: "!"}), rec_on(R, 1, 0, 16, b"first1", [(9, M)], {0: "!"}),
            rec_on(R, 1, L1 - 9, 0, b"last1", [(9, M)], {8: "!", 7: "="}), rec_on(R, 1, L1 - 1, 0, b"only_last1", [(4, S), (1, M)], {4: "!"}),
            rec_on(R, 1, L1 - 19, 0, b"last1_long", [(19, M)], {18: "=", 17: "!", 3: "="}),
            rec_on(R, 0, L0 - 8, 0, b"past0", [(9, M)]), record(0, 700, 0, b"l_seq_short", [(20, M)], "A" * 19), record(0, 700, 0, b"l_seq_long", [(20, M)], "A" * 21),
            record(1, (1 << 31) - 1, 0, b"range", pui.TO_THE_EDGE + [(9, M)], "ACGTACGTA")]
    pairs = []
    for t, tl in enumerate((1, -1, 7999, -7999, 8000, 8001, -8001, INT32_MIN, (1 << 31) - 1, 0)):
        pairs.append(rec_on(R, 0, 800, 0x63, b"tlen%d" % t, [(10, M)], next_tid=0, next_pos=900, tlen=tl))
    for a in (0, 1):
        for b in (0, 1):
            for t, (pos, npos) in enumerate(((600, 700), (650, 650), (700, 600))):
                pairs.append(rec_on(R, 1, pos, 0x43 | a << 4 | b << 5, b"ori%d%d%d" % (a, b, t), [(10, M)], next_tid=1, next_pos=npos, tlen=50 + t))
    pairs += [rec_on(R, 0, 800, 0xa3, b"read2_is_not_counted", [(10, M)], next_tid=0, next_pos=900, tlen=300), rec_on(R, 0, 800, 0x6b, b"mate_unmapped", [(10, M)], next_tid=0, next_pos=800, tlen=300),
              rec_on(R, 0, 800, 0x63, b"other_chr", [(10, M)], next_tid=1, next_pos=900, tlen=300), rec_on(R, 0, 800, 0x163, b"secondary_pair", [(10, M)], next_tid=0, next_pos=900, tlen=300),
              rec_on(R, 0, 800, 0x60, b"not_paired", [(10, M)], next_tid=0, next_pos=900, tlen=300)]
    flags = [record(-1, -1, 4, b"unplaced", [], "ACGTA", mapq=0), record(-1, -1, 0x4d, b"unplaced_pair", [], "ACGTA", mapq=0), record(1, 77, 0x45 | 0x20, b"placed_unmapped", [], "ACGTACG", mapq=0, next_tid=1, next_pos=77),
             rec_on(R, 1, 77, 0x89 | 0x10, b"its_singleton_mate", [(7, M)], next_tid=1, next_pos=77), record(0, 5, 4, b"placed_unmapped_with_cigar", [(4, M)], "ACGT"),
             rec_on(R, 0, 900, 0x100, b"secondary", [(10, M)], {5: "!"}), rec_on(R, 0, 900, 0x800, b"supplementary", [(10, M)], {5: "!"}), rec_on(R, 0, 900, 0x900, b"both", [(10, M)], {5: "!"}),
             rec_on(R, 0, 900, 0x200, b"qcfail", [(10, M)], {5: "!"}), rec_on(R, 0, 900, 0x243, b"qcfail_pair", [(10, M)], next_tid=0, next_pos=950, tlen=60),
             rec_on(R, 0, 900, 0x400, b"duplicate", [(10, M)], {5: "!"}), rec_on(R, 0, 900, 0x500, b"secondary_duplicate", [(10, M)]), rec_on(R, 0, 900, 0x483, b"duplicate_pair", [(10, M)], next_tid=0, next_pos=950)]
    for mq in (0, 4, 5, 255):
        flags.append(rec_on(R, 0, 1000, 0x43, b"mq%d" % mq, [(10, M)], {2: "!"}, mapq=mq, next_tid=1, next_pos=10, tlen=0))
        flags.append(rec_on(R, 0, 1000, 0, b"mq%d_single" % mq, [(10, M)], mapq=mq))
    flags += [rec_on(R, 0, 1000, 0x43, b"next_m1", [(10, M)], next_tid=-1, next_pos=-1), rec_on(R, 0, 1000, 0x3, b"neither_read", [(10, M)], next_tid=0, next_pos=1000),
              rec_on(R, 0, 1000, 0xc3, b"both_reads", [(10, M)], next_tid=0, next_pos=1000), rec_on(R, 0, 1000, 0x47, b"proper_but_unmapped", [(10, M)], next_tid=0, next_pos=1000)]
    quals = [rec_on(R, 0, 1200, 0, b"q0", [(12, M)], qual=0), rec_on(R, 0, 1200, 16, b"q93", [(12, M)], qual=93), rec_on(R, 0, 1200, 0, b"qff", [(12, M)], qual=0xff),
             rec_on(R, 0, 1200, 0x93, b"qmix", [(2, S), (8, M), (2, I)], {3: "!"}, qual=bytes([0, 93, 0xff, 1, 2, 0xff, 40, 41, 93, 0, 0xff, 7]))]
    return {"lengths": lengths, "big": big, "ops": ops, "ends": ends, "pairs": pairs, "flags": flags, "quals": quals, "empty": []}


def malformed_cases(R=REF):
    """name -> raw bytes: arrays with a record that is not whole (host lane code only)"""
    good = rec_on(R, 0, 200, 0, b"good", [(10, M)], {1: "!"})
    whole = rec_on(R, 0, 900, 0x43, b"cut", [(30, M)], {29: "!"}, next_tid=0, next_pos=950, tlen=80)
    return {"liar": good + liar(R) + good, "cut_quals": good + whole[:len(whole) - 1], "cut_bases": good + whole[:len(whole) - 34], "cut_head": good + whole[:30],
            "block_size_too_small": good + struct.pack("<I", 40) + whole[4:44] + good}


def random_records(rng, n, ref: Ref):
    """pileup_inputs.random_records with mate fields, qualities and more flags"""
    out = []
    for r in pui.random_records(rng, n, ref):
        b = bytearray(r)
        flag = struct.unpack_from("<H", b, 18)[0] | rng.choice([0, 0, 1, 1, 0x41, 0x81, 0x200, 0x800, 0x21, 0x9, 0x3])
        struct.pack_into("<H", b, 18, flag)
        tid = struct.unpack_from("<i", b, 4)[0]
        struct.pack_into("<iii", b, 24, rng.choice([tid, tid, tid, -1, 0]), rng.randrange(-1, 1500), rng.choice([0, 1, -1, 250, -250, 7999, 8000, 9000, -123456, rng.randrange(-600, 600)]))
        l_name, n_cig, l_seq = b[12], struct.unpack_from("<H", b, 16)[0], struct.unpack_from("<I", b, 20)[0]
        q_at = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
        for j in range(q_at, min(q_at + l_seq, len(b))):
            b[j] = rng.choice([0, 2, 11, 30, 37, 41, 93, 0xff])
        out.append(bytes(b))
    return out


# ---- the native program ----
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "qc_checks_san" if sanitize else "qc_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra + ["-o", exe, os.path.join(common.ROOT, "tests", "native", "qc_checks.hip")])
    return exe


def run_program(exe, workdir, tag, ref: Ref, raw, names, exclude=DEFAULT_EXCLUDE, min_mapq=0):
    """-> (the words, the text's bytes) of the lane code over `raw`"""
    src = os.path.join(workdir, "qc_%s.in" % tag); out_w = os.path.join(workdir, "qc_%s.words" % tag); out_t = os.path.join(workdir, "qc_%s.txt" % tag)
    name_off = [0]
    for nm in names:
        name_off.append(name_off[-1] + len(nm))
    pac = ref.pac()
    pad = lambda b: b + bytes(-len(b) % 8)
    with open(src, "wb") as f:
        f.write(struct.pack("<8q", ref.n_chr, exclude, min_mapq, 0, len(raw), name_off[-1], len(ref.codes), len(pac)))
        f.write(struct.pack("<%dq" % ref.n_chr, *ref.chr_off) + struct.pack("<%dq" % ref.n_chr, *ref.chr_len))
        f.write(pad(struct.pack("<%dI" % (ref.n_chr + 1), *name_off)) + pad(b"".join(names)) + pad(pac) + raw)
    r = subprocess.run([exe, "tables", src, out_w, out_t], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(out_w, dtype="<u8"), open(out_t, "rb").read()


def format_program(exe, workdir, tag, words, names, lengths):
    """-> the formatter's text of `words` through the native program (no tables are computed)"""
    src = os.path.join(workdir, "qcf_%s.in" % tag); out_t = os.path.join(workdir, "qcf_%s.txt" % tag)
    with open(src, "wb") as f:
        f.write(struct.pack("<q", len(names)) + struct.pack("<%dq" % len(names), *[int(x) for x in lengths]))
        for nm in names:
            f.write(struct.pack("<q", len(nm)) + nm)
        f.write(np.asarray(words, dtype="<u8").tobytes())
    r = subprocess.run([exe, "format", src, out_t], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(out_t, "rb").read()
