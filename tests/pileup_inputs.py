"""Helpers of the allele-count tests: the sequential Python twin of the definition in dart_amd/csrc/dg_pileup.h (observations in dictionaries, one walk over the
sorted positions -- record by record, not as the kernels' scans), a second, independent check (one row of counters per position, bumped base by base), record
builders with explicit bases, hand-made cases that each hold what they are named for, and the native program tests/native/pileup_checks.hip.  The definition is
the header's comment: no pileup tool exists where these tests run."""
from __future__ import annotations

import os, struct, subprocess
import numpy as np
import common
import bamsort_inputs as bsi
from bamidx_inputs import M, I, D, N, S, H, P, EQ, X

MAX_POS = (1 << 32) - 1
DEFAULT_EXCLUDE = 0x704
NIBBLE = {c: k for k, c in enumerate("=ACMGRSVTWYHKDBN")}
A_, C_, G_, T_, N_, DEL, INS = range(7)
SITE_ENTRY = np.dtype([("chr", "<u4"), ("pos", "<u4"), ("depth", "<u4"), ("depth_rev", "<u4"), ("ref", "<u4"), ("top", "<u4"), ("n", "<u4", (7,)), ("n_rev", "<u4", (7,))])


def offsets(raw: bytes):
    """where the records start; the last one may be cut short by the array's end"""
    out, p = [], 0
    while p + 4 <= len(raw):
        out.append(p); p += 4 + struct.unpack_from("<I", raw, p)[0]
    return out


class RangeError(Exception):
    """a record that passes the coverage track's conditions has a block that ends behind 2^32 - 1 (args[0] = its index)"""


class Ref:
    """the reference as the index's 2-bit text holds it: codes 0..3 of the forward strand, the chromosomes' offsets and lengths"""

    def __init__(self, codes, chr_len):
        self.codes = np.asarray(codes, np.uint8); self.chr_len = [int(x) for x in chr_len]
        self.chr_off = [sum(self.chr_len[:k]) for k in range(len(self.chr_len))]
        assert len(self.codes) == sum(self.chr_len)
        self.n_chr = len(self.chr_len)

    def base(self, tid, p):
        return int(self.codes[self.chr_off[tid] + p])

    def pac(self) -> bytes:
        L = len(self.codes)
        c = np.zeros((L + 3) // 4 * 4, np.uint8); c[:L] = self.codes
        q = c.reshape(-1, 4)
        body = (q[:, 0] << 6 | q[:, 1] << 4 | q[:, 2] << 2 | q[:, 3]).astype(np.uint8).tobytes()
        return body if L % 4 else body + b"\0"               # (the .pac file's own layout: L / 4 + 1 bytes)


def ref_of_index(ix) -> Ref:
    """host.Index -> Ref: the .pac file's forward text"""
    pac = np.asarray(ix.pac)
    codes = np.stack([pac >> 6 & 3, pac >> 4 & 3, pac >> 2 & 3, pac & 3], 1).reshape(-1)[:ix.l_pac]
    return Ref(codes, ix.chr_len)


def random_ref(seed, chr_len) -> Ref:
    rng = np.random.RandomState(seed)
    return Ref(rng.randint(0, 4, sum(chr_len)), chr_len)


def record(tid, pos, flag, name, cigar, seq, mapq=30, l_seq=None, tags=b""):
    """a BAM record with explicit bases: seq is a string over =ACMGRSVTWYHKDBN; l_seq: what the record says (default: len(seq))"""
    nib = [NIBBLE[c] for c in seq] + [0]
    packed = bytes(nib[k] << 4 | nib[k + 1] for k in range(0, len(seq), 2))
    ls = len(seq) if l_seq is None else l_seq
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, mapq, 4680, len(cigar), flag, ls, -1, -1, 0)
    body += name + b"\0" + b"".join(struct.pack("<I", l << 4 | op) for l, op in cigar) + packed + b"\x1e" * len(seq) + tags
    return struct.pack("<i", len(body)) + body


def read_of(ref: Ref, tid, pos, cigar, edits=(), ins="ACGT"):
    """the bases of a read that follows the reference along `cigar` from `pos`; inserted and clipped bases cycle through `ins`; edits: {read index: letter}
    (letter "!" = the complement of what stands there: a sure mismatch)"""
    out, p = [], pos
    for ln, op in cigar:
        if op in (M, EQ, X):
            out += ["ACGT"[ref.base(tid, p + k)] if 0 <= p + k < ref.chr_len[tid] else "A" for k in range(ln)]; p += ln
        elif op in (D, N):
            p += ln
        elif op in (I, S):
            out += [ins[(len(out) + k) % len(ins)] for k in range(ln)]
    edits = dict(edits)
    for k, c in edits.items():
        out[k] = "TGCA"["ACGT".index(out[k])] if c == "!" else c
    return "".join(out)


def rec_on(ref, tid, pos, flag, name, cigar, edits=(), mapq=30):
    return record(tid, pos, flag, name, cigar, read_of(ref, tid, pos, cigar, edits), mapq)


# ---- the twin ----
def classify(raw: bytes, at: int, ref: Ref, exclude: int, min_mapq: int):
    """-> ("skip" | "range" | "left_out" | "counted", refid, pos, s, [CIGAR words], nibbles)"""
    bs, refid, pos = struct.unpack_from("<Iii", raw, at)
    l_name, mapq = raw[at + 12], raw[at + 13]
    n_cig, flag = struct.unpack_from("<HH", raw, at + 16)
    l_seq = struct.unpack_from("<I", raw, at + 20)[0]
    size = min(4 + bs, len(raw) - at)
    if not (0 <= refid < ref.n_chr and pos >= 0 and not flag & 4 and n_cig > 0 and not flag & exclude and mapq >= min_mapq) or 36 + l_name + 4 * n_cig > size:
        return ("skip",)
    cigar = struct.unpack_from("<%dI" % n_cig, raw, at + 36 + l_name)
    p, qlen = pos, 0
    for c in cigar:
        op, ln = c & 15, c >> 4
        if op in (M, EQ, X):
            p += ln; qlen += ln
            if ln and p > MAX_POS:
                return ("range",)
        elif op in (D, N):
            p += ln
        elif op in (I, S):
            qlen += ln
    seq_at = at + 36 + l_name + 4 * n_cig
    if seq_at + (l_seq + 1) // 2 > at + size or l_seq == 0:
        return ("skip",)
    if qlen != l_seq or p > ref.chr_len[refid]:
        return ("left_out",)
    nib = [raw[seq_at + k // 2] >> 4 if k % 2 == 0 else raw[seq_at + k // 2] & 15 for k in range(l_seq)]
    return ("counted", refid, pos, flag >> 4 & 1, cigar, nib)


def allele_of(nibble, ref_base):
    return {1: A_, 2: C_, 4: G_, 8: T_, 0: ref_base}.get(nibble, N_)


def observations(ref: Ref, refid, pos, s, cigar, nib):
    """-> (blocks [(start, end)], alleles [(position, allele 0..6)]) of a counted record, in the walk's order"""
    blocks, alleles, p, q = [], [], pos, 0
    for c in cigar:
        op, ln = c & 15, c >> 4
        if op in (M, EQ, X):
            if ln:
                blocks.append((p, p + ln))
            for k in range(ln):
                a = allele_of(nib[q + k], ref.base(refid, p + k))
                if a != ref.base(refid, p + k):
                    alleles.append((p + k, a))
            p += ln; q += ln
        elif op == D:
            alleles += [(p + k, DEL) for k in range(ln)]; p += ln
        elif op == N:
            p += ln
        elif op == I:
            if ln:
                alleles.append((max(p, pos + 1) - 1, INS))
            q += ln
        elif op == S:
            q += ln
    return blocks, alleles


def twin(raw: bytes, ref: Ref, exclude=DEFAULT_EXCLUDE, min_mapq=0, min_alt=2):
    """-> (entries [(chr, pos, depth, depth_rev, ref, top, n x 7, n_rev x 7)], stats (10 values)); raises RangeError(index of the first record out of range)"""
    dep, cnt = {}, {}
    st = [0] * 10
    for i, at in enumerate(offsets(raw)):
        c = classify(raw, at, ref, exclude, min_mapq)
        if c[0] == "range":
            raise RangeError(i)
        if c[0] == "left_out":
            st[8] += 1
        if c[0] != "counted":
            continue
        _, refid, pos, s, cigar, nib = c
        blocks, alleles = observations(ref, refid, pos, s, cigar, nib)
        st[0] += 1; st[1] += len(blocks); st[2] += sum(e - b for b, e in blocks)
        for b, e in blocks:
            dep.setdefault((refid, b), [0, 0])[s] += 1
            dep.setdefault((refid, e), [0, 0])[s] -= 1
        for p, a in alleles:
            cnt.setdefault((refid, p), [[0, 0] for _ in range(7)])[a][s] += 1
            st[3 if a < DEL else 4 if a == DEL else 5] += 1
    entries, run, chrom = [], [0, 0], -1
    for key in sorted(set(dep) | set(cnt)):
        if key[0] != chrom:
            assert run == [0, 0]
            chrom = key[0]
        d = dep.get(key)
        if d:
            run = [run[0] + d[0], run[1] + d[1]]
            assert run[0] >= 0 and run[1] >= 0
        if key in cnt:
            n = [x[0] + x[1] for x in cnt[key]]; n_rev = [x[1] for x in cnt[key]]
            r = ref.base(*key)
            depth, depth_rev = run[0] + run[1], run[1]
            assert n[r] == 0
            n[r] = depth - sum(n[a] for a in range(5) if a != r); n_rev[r] = depth_rev - sum(n_rev[a] for a in range(5) if a != r)
            assert n[r] >= 0 and n_rev[r] >= 0
            top = max((a for a in range(7) if a != r), key=lambda a: (n[a], -a))
            st[6] += 1
            if n[top] >= min_alt:
                st[7] += 1; st[9] = max(st[9], depth)
                entries.append((key[0], key[1], depth, depth_rev, r, top) + tuple(n) + tuple(n_rev))
    assert run == [0, 0]
    return entries, tuple(st)


def text_of(entries, names) -> bytes:
    return b"".join(b"%s\t%d\t%s\t%s\n" % (names[e[0]], e[1] + 1, b"ACGT"[e[4]:e[4] + 1], b"\t".join(b"%d" % x for x in e[2:4] + e[6:])) for e in entries)


def as_tuples(arr):
    """a SITE_ENTRY array -> the twin's tuples"""
    return [(int(x["chr"]), int(x["pos"]), int(x["depth"]), int(x["depth_rev"]), int(x["ref"]), int(x["top"])) + tuple(int(v) for v in x["n"]) + tuple(int(v) for v in x["n_rev"]) for x in arr]


def brute(raw: bytes, ref: Ref, exclude=DEFAULT_EXCLUDE, min_mapq=0, min_alt=2):
    """the independent check: for every position of every chromosome a row of counters -- depth on both strands, the seven alleles on both strands -- bumped
    observation by observation as SAM text would be read (its own field reads and CIGAR walk over op letters); then every position with an allele that is not
    the reference base is a site.  -> entries, to be compared with the twin's"""
    tab = [np.zeros((ln + 1, 16), np.int64) for ln in ref.chr_len]           # [0] depth, [1] depth_rev, [2..8] n, [9..15] n_rev
    p = 0
    while p + 4 <= len(raw):
        size = 4 + int.from_bytes(raw[p:p + 4], "little")
        rec = raw[p:p + size]; p += size
        if len(rec) < 36:
            continue
        tid = int.from_bytes(rec[4:8], "little", signed=True); pos = int.from_bytes(rec[8:12], "little", signed=True)
        flag = rec[18] | rec[19] << 8; n_cig = rec[16] | rec[17] << 8; l_name = rec[12]; l_seq = int.from_bytes(rec[20:24], "little")
        if tid < 0 or tid >= ref.n_chr or pos < 0 or flag & 4 or n_cig == 0 or flag & exclude or rec[13] < min_mapq or 36 + l_name + 4 * n_cig > len(rec):
            continue
        ops = [(int.from_bytes(rec[36 + l_name + 4 * k:40 + l_name + 4 * k], "little") >> 4, "MIDNSHP=X???????"[rec[36 + l_name + 4 * k] & 15]) for k in range(n_cig)]
        sq = 36 + l_name + 4 * n_cig
        if l_seq == 0 or sq + (l_seq + 1) // 2 > len(rec) or sum(l for l, o in ops if o in "MIS=X") != l_seq or pos + sum(l for l, o in ops if o in "MDN=X") > ref.chr_len[tid]:
            continue
        letters = "".join("=ACMGRSVTWYHKDBN"[rec[sq + k // 2] >> 4 if k % 2 == 0 else rec[sq + k // 2] & 15] for k in range(l_seq))
        rev = 1 if flag & 16 else 0
        at, q, t = pos, 0, tab[tid]
        for ln, o in ops:
            if o in "M=X":
                for k in range(ln):
                    ch = letters[q + k]; r = ref.base(tid, at + k)
                    a = r if ch == "=" else "ACGT".index(ch) if ch in "ACGT" else 4
                    t[at + k, 0] += 1; t[at + k, 1] += rev; t[at + k, 2 + a] += 1; t[at + k, 9 + a] += rev
                at += ln; q += ln
            elif o == "D":
                t[at:at + ln, 2 + DEL] += 1; t[at:at + ln, 9 + DEL] += rev; at += ln
            elif o == "N":
                at += ln
            elif o == "I":
                if ln:
                    t[at - 1 if at > pos else pos, 2 + INS] += 1; t[at - 1 if at > pos else pos, 9 + INS] += rev
                q += ln
            elif o == "S":
                q += ln
    out = []
    for tid, t in enumerate(tab):
        codes = ref.codes[ref.chr_off[tid]:ref.chr_off[tid] + ref.chr_len[tid]]
        alt = t[:-1, 2:9].copy(); alt[np.arange(len(codes)), codes] = 0
        for pos in np.flatnonzero(alt.sum(1)):
            r = int(codes[pos]); row = t[pos]
            top = max((a for a in range(7) if a != r), key=lambda a: (row[2 + a], -a))
            if row[2 + top] >= min_alt:
                out.append((tid, int(pos), int(row[0]), int(row[1]), r, top) + tuple(int(x) for x in row[2:16]))
    return out


# ---- hand-made cases ----
REF = random_ref(11, [3000, 2000])
NAMES = [b"chrA", b"b"]
TO_THE_EDGE = [((1 << 28) - 1, N)] * 8                                                          # from pos 2^31 - 1 to 2^32 - 9
# the filter settings: (exclude, min_mapq, min_alt)
FILTERS = [(DEFAULT_EXCLUDE, 0, 2), (DEFAULT_EXCLUDE, 0, 1), (4, 0, 1), (0x400 | 4, 0, 3), (DEFAULT_EXCLUDE, 10, 1)]


def liar(R=REF):
    """n_cigar_op says 60000 ops, block_size holds one: the record counts for nothing (dg_bam_sort_add refuses it: only the lane code's tests see it)"""
    r = bytearray(rec_on(R, 0, 50, 0, b"liar", [(10, M)], {3: "!"})); struct.pack_into("<H", r, 16, 60000)
    return bytes(r)


def crafted_cases(R=REF, names=NAMES):
    """name -> (records in coordinate order, chromosome names); all on R (two chromosomes of at least 3000 and 2000 bases)"""
    L0, L1 = R.chr_len[0], R.chr_len[1]
    ops = [
        rec_on(R, 0, 100, 0, b"all_ops", [(5, S), (10, M), (2, I), (3, D), (700, N), (4, EQ), (1, X), (6, P), (7, H)], {7: "!", 20: "!"}),
        rec_on(R, 0, 100, 16, b"all_ops_again", [(5, S), (10, M), (2, I), (3, D), (700, N), (4, EQ), (1, X), (6, P), (7, H)], {7: "!", 20: "!"}),
        rec_on(R, 0, 300, 0, b"zero_m_first", [(0, M), (5, M)], {0: "!"}), rec_on(R, 0, 300, 0, b"zero_m_twin", [(0, M), (5, M)], {0: "!"}),
        rec_on(R, 0, 400, 0, b"i_at_start", [(3, I), (20, M)]), rec_on(R, 0, 400, 16, b"i_at_start_rev", [(3, I), (20, M)]),
        rec_on(R, 0, 450, 0, b"i_at_end", [(20, M), (3, I)]), rec_on(R, 0, 450, 0, b"i_at_end2", [(20, M), (3, I)]),
        rec_on(R, 0, 500, 0, b"i_behind_d", [(10, M), (2, D), (3, I), (10, M)]), rec_on(R, 0, 500, 0, b"i_behind_d2", [(10, M), (2, D), (3, I), (10, M)]),
        rec_on(R, 0, 600, 0, b"s_h_both_ends", [(4, H), (3, S), (20, M), (2, S), (5, H)], {3: "!", 22: "!"}),
        rec_on(R, 0, 600, 16, b"s_h_both_ends2", [(4, H), (3, S), (20, M), (2, S), (5, H)], {3: "!", 22: "!"}),
        rec_on(R, 0, 1000, 0, b"d_under", [(10, M), (5, D), (10, M)]), rec_on(R, 0, 1000, 0, b"d_under2", [(10, M), (5, D), (10, M)]), rec_on(R, 0, 1000, 16, b"over_the_d", [(25, M)], {12: "!"}),
        rec_on(R, 0, 1100, 0, b"n_gap", [(10, M), (50, N), (10, M)], {9: "!", 10: "!"}), rec_on(R, 0, 1100, 0, b"n_gap2", [(10, M), (50, N), (10, M)], {9: "!", 10: "!"}),
        rec_on(R, 0, 1200, 0, b"zero_len_i_d", [(10, M), (0, I), (0, D), (10, M)]),
    ]
    bases = [
        rec_on(R, 0, 100, 0, b"odd_last", [(31, M)], {30: "!"}), rec_on(R, 0, 100, 0, b"odd_last2", [(31, M)], {30: "!"}),
        rec_on(R, 0, 200, 0, b"even_last", [(30, M)], {29: "!"}), rec_on(R, 0, 200, 16, b"even_last2", [(30, M)], {29: "!"}),
        rec_on(R, 0, 300, 0, b"eq_n_iupac", [(12, M)], {2: "=", 5: "N", 8: "R"}), rec_on(R, 0, 300, 0, b"eq_n_iupac2", [(12, M)], {2: "=", 5: "N", 8: "M", 9: "!"}),
        rec_on(R, 0, 300, 16, b"all_eq", [(12, EQ)], {k: "=" for k in range(12)}),
        rec_on(R, 0, 400, 0, b"x_that_matches", [(10, X)]), rec_on(R, 0, 400, 0, b"eq_that_differs", [(10, EQ)], {4: "!"}), rec_on(R, 0, 400, 0, b"eq_that_differs2", [(10, EQ)], {4: "!"}),
    ]
    seams = []
    for start in range(4):                                   # reads starting at text offsets 0..3 mod 4 (chromosome 0 starts at text offset 0), a mismatch at each offset 0..16
        for k in range(17):                                  # around the 4-, 16- and 32-base seams of the packed text and the 16-base steps of the walk
            seams.append(rec_on(R, 0, 1000 + start, 16 if k & 1 else 0, b"seam%d_%d" % (start, k), [(40, M)], {k: "!", 39 - k: "!"}))
    seams += [rec_on(R, 0, 1500 + k, 0, b"every%d" % k, [(1 + k, S), (37, M)], {1 + k + j: "!" for j in range(0, 37, 3)}) for k in range(8)]
    ends = [
        rec_on(R, 0, 0, 0, b"pos0", [(5, M)], {0: "!"}), rec_on(R, 0, 0, 0, b"pos0_i", [(2, I), (5, M)], {2: "!"}),
        rec_on(R, 0, L0 - 20, 0, b"last_of_chr0", [(20, M)], {19: "!"}), rec_on(R, 0, L0 - 20, 16, b"last_of_chr0_2", [(20, M)], {19: "!", 0: "N"}),
        rec_on(R, 1, 0, 0, b"first_of_chr1", [(20, M)], {0: "!"}), rec_on(R, 1, 0, 0, b"first_of_chr1_2", [(20, M)], {0: "!"}),
        rec_on(R, 0, L0 - 19, 0, b"one_past_chr0", [(20, M)], {3: "!"}), rec_on(R, 1, L1 - 10, 0, b"d_past_chr1", [(5, M), (6, D)], {2: "!"}),
        rec_on(R, 1, L1 - 5, 0, b"ends_on_chr1", [(5, M)], {4: "!"}), rec_on(R, 1, L1 - 5, 0, b"ends_on_chr1_2", [(5, M)], {4: "!"}),
        record(0, 700, 0, b"l_seq_short", [(20, M)], "A" * 19), record(0, 700, 0, b"l_seq_long", [(20, M)], "A" * 21), record(0, 700, 0, b"l_seq_0", [(20, M)], ""),
        record(1, (1 << 31) - 1, 0, b"ends_at_2_32_m1", TO_THE_EDGE + [(8, M)], "ACGTACGT"),
    ]
    ends_bad = ends + [record(0, 7, 0x400, b"a_duplicate_out_of_range", TO_THE_EDGE[:1] * 17 + [(8, M)], "ACGTACGT"), record(1, (1 << 31) - 1, 0, b"ends_at_2_32", TO_THE_EDGE + [(9, M)], "ACGTACGTA")]
    nothing = [
        rec_on(R, 0, -1, 0, b"pos_m1", [(10, M)], {1: "!"}), record(0, 10, 0, b"no_cigar", [], "ACGTACGTAC"), rec_on(R, 0, 20, 4, b"placed_unmapped", [(10, M)], {1: "!"}),
        rec_on(R, 0, 200, 0, b"the_one_that_counts", [(10, M)], {1: "!"}), record(-1, -1, 4, b"unplaced", [], "ACGT"), record(-1, 30, 0, b"unplaced_with_cigar", [(10, M)], read_of(R, 0, 30, [(10, M)], {1: "!"})),
    ]
    filters = [rec_on(R, 0, 100, 0x100, b"secondary", [(10, M)], {5: "!"}), rec_on(R, 0, 100, 0x200, b"qcfail", [(10, M)], {5: "!"}), rec_on(R, 0, 100, 0x400, b"duplicate", [(10, M)], {5: "!"}),
               rec_on(R, 0, 100, 0, b"mapq10", [(10, M)], {5: "!"}, mapq=10), rec_on(R, 0, 100, 0, b"mapq9", [(10, M)], {5: "!"}, mapq=9),
               rec_on(R, 1, 100, 0x41, b"mate1_fwd", [(10, M)], {5: "!"}), rec_on(R, 1, 100, 0x91, b"mate2_rev", [(10, M)], {5: "!"}), rec_on(R, 1, 100, 0x81, b"mate2_fwd", [(10, M)], {5: "!"})]
    r0 = "ACGT"[R.base(0, 105)]
    alts = [c for c in "ACGT" if c != r0]
    min_alt = [rec_on(R, 0, 100, 0, b"one", [(10, M)], {5: alts[0]}),                                                        # position 105: one observation; 125: two; 145: three
               rec_on(R, 0, 120, 0, b"two_a", [(10, M)], {5: "!"}), rec_on(R, 0, 120, 16, b"two_b", [(10, M)], {5: "!"}),
               rec_on(R, 0, 140, 0, b"three_a", [(10, M)], {5: "!"}), rec_on(R, 0, 140, 16, b"three_b", [(10, M)], {5: "!"}), rec_on(R, 0, 140, 0, b"three_c", [(10, M)], {5: "!"})]
    r1 = "ACGT"[R.base(0, 505)]
    a1 = [c for c in "ACGT" if c != r1]
    ties = [rec_on(R, 0, 500, 0, b"tie_hi%d" % k, [(10, M)], {5: a1[2]}) for k in range(2)] + [rec_on(R, 0, 500, 0, b"tie_lo%d" % k, [(10, M)], {5: a1[0]}) for k in range(2)] + \
           [rec_on(R, 0, 600, 0, b"tie_del%d" % k, [(5, M), (1, D), (5, M)]) for k in range(2)] + [rec_on(R, 0, 600, 0, b"tie_n%d" % k, [(10, M)], {5: "N"}) for k in range(2)] + \
           [rec_on(R, 0, 700, 0, b"tie_ins%d" % k, [(5, M), (1, I), (5, M)]) for k in range(3)] + [rec_on(R, 0, 700, 0, b"tie_delb%d" % k, [(4, M), (1, D), (6, M)]) for k in range(3)]
    srt = lambda recs: sorted(recs, key=lambda r: bsi.key(r, 2))
    return {"ops": (srt(ops), names), "bases": (srt(bases), names), "seams": (srt(seams), names), "ends": (srt(ends), names), "ends_bad": (srt(ends_bad), names),
            "nothing": (srt(nothing), names), "nothing_liar": (srt(nothing[:4] + [liar(R)]) + nothing[4:], names), "filters": (srt(filters), names), "min_alt": (srt(min_alt), names),
            "ties": (srt(ties), names), "empty": ([], names)}


def random_records(rng, n, ref: Ref, span=1500, sub=0.03):
    """n records over `ref` with CIGARs of every op and bases that mostly follow the reference, clustered so that depths rise and keys collide; a few that count
    for nothing, a few that disagree with their l_seq or pass their chromosome's end"""
    out = []
    for k in range(n):
        cigar = [(rng.choice([0, 1, 2, 5, 17, 33]), rng.choice([M, M, M, M, I, D, N, S, EQ, X, H, P])) for _ in range(rng.randrange(1, 6))]
        flag = rng.choice([0, 16, 0x41, 0x91, 0x51, 0x81, 0x100, 0x400, 4])
        tid = rng.randrange(-1, ref.n_chr)
        if tid < 0:
            out.append(record(-1, -1, flag | 4, b"u%d" % k, [], "ACGT")); continue
        grid = rng.choice([1, 25])
        pos = rng.choice([-1] + [rng.randrange(0, span) // grid * grid] * 30 + [ref.chr_len[tid] - rng.randrange(1, 40)])
        seq = list(read_of(ref, tid, max(pos, 0), cigar))
        for j in range(len(seq)):
            if rng.random() < sub:
                seq[j] = rng.choice("ACGTN=RY")
        seq = "".join(seq)
        if rng.random() < 0.02:
            seq = seq[:-1] if seq else "A"
        out.append(record(tid, pos, flag, b"r%d" % k, cigar, seq, mapq=rng.randrange(0, 40)))
    return out


# ---- the native program ----
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "pileup_checks_san" if sanitize else "pileup_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "pileup_checks.hip")])
    return exe


def run_program(exe, workdir, tag, ref: Ref, raw, names, exclude=DEFAULT_EXCLUDE, min_mapq=0, min_alt=2):
    """-> dict(recs = [(state, events)], events = [(key, value)] sorted, keys = [(key, n, depth)], sites = the entries before the filter, entries = the kept ones,
    stats = the ten, bad = index of the first record out of range or None, text = the bytes)"""
    src = os.path.join(workdir, "pu_%s.in" % tag); txt = os.path.join(workdir, "pu_%s.txt" % tag); out = os.path.join(workdir, "pu_%s.tsv" % tag)
    name_off = [0]
    for nm in names:
        name_off.append(name_off[-1] + len(nm))
    pac = ref.pac()
    pad = lambda b: b + bytes(-len(b) % 8)
    with open(src, "wb") as f:
        f.write(struct.pack("<8q", ref.n_chr, exclude, min_mapq, min_alt, len(raw), name_off[-1], len(ref.codes), len(pac)))
        f.write(struct.pack("<%dq" % ref.n_chr, *ref.chr_off) + struct.pack("<%dq" % ref.n_chr, *ref.chr_len))
        f.write(pad(struct.pack("<%dI" % (ref.n_chr + 1), *name_off)) + pad(b"".join(names)) + pad(pac) + raw)
    r = subprocess.run([exe, src, txt, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    res = dict(recs=[], events=[], keys=[], sites=[], entries=[], stats=None, bad=None, text=open(out, "rb").read())
    for line in open(txt).read().splitlines():
        w = line.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "rec":
            res["recs"].append((v[1], v[2]))
        elif w[0] == "ev":
            res["events"].append(tuple(v))
        elif w[0] == "key":
            res["keys"].append(tuple(v))
        elif w[0] == "site":
            res["sites"].append(tuple(v))
        elif w[0] == "ent":
            res["entries"].append(tuple(v))
        elif w[0] == "stats":
            res["stats"] = tuple(v)
        elif w[0] == "bad":
            res["bad"] = v[0]
    return res


# ---- planted variants ----
def planted_case(ref: Ref, seed=29, n_snv=20, depth=20, rlen=101, flank=300):
    """-> (variants [(kind, chr, pos, allele)], reads as an uint8 array [n, rlen] of ASCII).  Reads come from a copy of `ref` with n_snv SNVs, one 3-base deletion
    and one 2-base insertion, each in a window of its own at about `depth`-fold coverage, either strand.  kind "snv": allele 0..3 observed at pos; "del": DEL at
    pos, pos + 1, pos + 2; "ins": INS anchored at pos (two bases inserted behind it).  Positions lie at least 5000 bases from the contigs' ends, on a grid that
    keeps the windows apart."""
    import random as _random
    rng = _random.Random(seed)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    variants, reads = [], []
    slots = [(c, p) for c in range(ref.n_chr) for p in range(5000, ref.chr_len[c] - 5000, 4000)]
    rng.shuffle(slots)
    for k, (c, p) in enumerate(sorted(slots[:n_snv + 2])):
        p += rng.randrange(0, 1000)
        lo = p - flank
        win = ["ACGT"[ref.base(c, x)] for x in range(lo, p + flank + rlen)]
        if k == 3:
            while len({ref.base(c, p - 1), ref.base(c, p), ref.base(c, p + 2), ref.base(c, p + 3)}) < 3:      # (a gap that cannot slide)
                p += 1
            del win[p - lo:p - lo + 3]; variants.append(("del", c, p, DEL))
        elif k == 7:
            r0, r1 = ref.base(c, p), ref.base(c, p + 1)
            ins = "ACGT"[(r1 + 1) % 4] + "ACGT"[(r0 + 2) % 4]
            win[p - lo + 1:p - lo + 1] = list(ins); variants.append(("ins", c, p, INS))
        else:
            a = (ref.base(c, p) + 1 + rng.randrange(3)) % 4
            win[p - lo] = "ACGT"[a]; variants.append(("snv", c, p, a))
        for _ in range(depth * (2 * flank) // rlen):
            s = rng.randrange(0, len(win) - rlen)
            r = win[s:s + rlen]
            if rng.random() < 0.5:
                r = [comp[x] for x in reversed(r)]
            reads.append(np.frombuffer("".join(r).encode(), np.uint8))
    return variants, np.stack(reads)


def depth_at(raw: bytes, ref: Ref, positions, exclude=DEFAULT_EXCLUDE, min_mapq=0):
    """the twin's depth at each (chr, pos): the counted records with a block over it"""
    out = {x: 0 for x in positions}
    for at in offsets(raw):
        c = classify(raw, at, ref, exclude, min_mapq)
        if c[0] == "counted":
            for b, e in observations(ref, *c[1:])[0]:
                for x in out:
                    if x[0] == c[1] and b <= x[1] < e:
                        out[x] += 1
    return out


def planted_found(raw: bytes, ref: Ref, entries, variants, min_depth=4):
    """-> (the planted variants whose positions all have a twin depth of at least min_depth, those of them whose positions are all kept sites with the planted
    allele on top)"""
    by_pos = {(e[0], e[1]): e for e in entries}
    places = {v: [(v[1], v[2] + k) for k in range(3 if v[0] == "del" else 1)] for v in variants}
    depth = depth_at(raw, ref, [x for v in variants for x in places[v]])
    deep = [v for v in variants if all(depth[x] >= min_depth for x in places[v])]
    found = [v for v in deep if all(x in by_pos and by_pos[x][5] == v[3] for x in places[v])]
    return deep, found
