"""Helpers of the MD / NM / ts tests: the sequential Python twin of the definition in dart_amd/csrc/dg_tags.h (record by record, base by base, one running count --
not the kernels' sixteen-base steps and bit scans), a second, independent restatement (every record expanded to per-base (read base, reference base, op) columns,
MD and NM printed from those; tags removed and appended through a generic aux decoder), records with explicit aux areas, hand-made cases that each hold what they
are named for, and the native program tests/native/tags_checks.hip.  The definition is the header's comment: no samtools exists where these tests run."""
from __future__ import annotations

import os, re, struct, subprocess
import numpy as np
import common
import bamsort_inputs as bsi
import pileup_inputs as pui
from pileup_inputs import Ref, record, rec_on, random_ref, read_of, offsets
from bamidx_inputs import M, I, D, N, S, H, P, EQ, X

MD_, NM_, TS_ = 1, 2, 4
ALL = 7
FLAG_SETS = [1, 2, 3, 4, 5, 6, 7]
NAMES_OF = {b"MD": MD_, b"NM": NM_, b"ts": TS_}
WIDTH = {ord(c): w for c, w in (("A", 1), ("c", 1), ("C", 1), ("s", 2), ("S", 2), ("i", 4), ("I", 4), ("f", 4))}
B_WIDTH = {ord(c): w for c, w in (("c", 1), ("C", 1), ("s", 2), ("S", 2), ("i", 4), ("I", 4), ("f", 4))}
PLUS = {("GT", "AG"), ("GC", "AG")}
MINUS = {("CT", "AC"), ("CT", "GC")}
REWRITE, NOT_ELIGIBLE, AUX_BAD = 0, 1, 2


# ---- the twin ----
def aux_items(rec: bytes, a: int, size: int):
    """the aux area [a, size) of the record -> [(start, bytes)] of its tags, or None when it cannot be walked"""
    out = []
    while a < size:
        if a + 3 > size:
            return None
        ty, v = rec[a + 2], a + 3
        if ty in WIDTH:
            ln = WIDTH[ty]
        elif ty in (ord("Z"), ord("H")):
            e = v
            while e < size and rec[e]:
                e += 1
            if e >= size:
                return None
            ln = e - v + 1
        elif ty == ord("B"):
            if v + 5 > size or rec[v] not in B_WIDTH:
                return None
            ln = 5 + B_WIDTH[rec[v]] * struct.unpack_from("<I", rec, v + 1)[0]
        else:
            return None
        if v + ln > size:
            return None
        out.append((a, 3 + ln)); a = v + ln
    return out


def nm_tag(nm: int) -> bytes:
    return b"NM" + (struct.pack("<cB", b"C", nm) if nm < 256 else struct.pack("<cH", b"S", nm) if nm < 65536 else struct.pack("<cI", b"I", nm))


def one(raw: bytes, at: int, ref: Ref, flags: int):
    """the record at `at` -> (its new bytes, kind, (removed, mismatches, indel bases, ts written, no motif, conflict))"""
    avail = len(raw) - at
    whole = 4 + struct.unpack_from("<I", raw, at)[0]
    size = min(whole, avail)
    old = raw[at:at + size]
    if whole > avail or avail < 36:
        return old, NOT_ELIGIBLE, None
    c = pui.classify(raw, at, ref, 0, 0)
    if c[0] != "counted":
        return old, NOT_ELIGIBLE, None
    _, refid, pos, s, cigar, nib = c
    l_name = raw[at + 12]
    aux_at = 36 + l_name + 4 * len(cigar) + (len(nib) + 1) // 2 + len(nib)
    if aux_at > size:
        return old, NOT_ELIGIBLE, None
    items = aux_items(old, aux_at, size)
    if items is None:
        return old, AUX_BAD, None
    kept = [old[a:a + n] for a, n in items if not NAMES_OF.get(old[a:a + 2], 0) & flags]
    md, u, p, q, mism, ins, dele, votes, introns = [], 0, pos, 0, 0, 0, 0, set(), 0
    for w in cigar:
        op, ln = w & 15, w >> 4
        if op in (M, EQ, X):
            for k in range(ln):
                r = ref.base(refid, p + k)
                if nib[q + k] == 0 or nib[q + k] == 1 << r:
                    u += 1
                else:
                    md.append("%d%s" % (u, "ACGT"[r])); u = 0; mism += 1
            p += ln; q += ln
        elif op == D:
            if ln:
                md.append("%d^%s" % (u, "".join("ACGT"[ref.base(refid, p + k)] for k in range(ln)))); u = 0; dele += ln
            p += ln
        elif op == N:
            if ln >= 4:
                introns += 1
                t = lambda x: "ACGT"[ref.base(refid, x)]
                motif = (t(p) + t(p + 1), t(p + ln - 2) + t(p + ln - 1))
                if motif in PLUS:
                    votes.add("+")
                elif motif in MINUS:
                    votes.add("-")
            p += ln
        elif op == I:
            ins += ln; q += ln
        elif op == S:
            q += ln
    md.append("%d" % u)
    tail, ts, no_motif, conflict = b"", 0, 0, 0
    if flags & NM_:
        tail += nm_tag(mism + ins + dele)
    if flags & MD_:
        tail += b"MDZ" + "".join(md).encode() + b"\0"
    if flags & TS_:
        if len(votes) == 1:
            g = votes.pop()
            tail += b"tsA" + (g if not s else "+" if g == "-" else "-").encode(); ts = 1
        elif introns:
            no_motif, conflict = (0, 1) if votes else (1, 0)
    body = old[4:aux_at] + b"".join(kept) + tail
    return struct.pack("<I", len(body)) + body, REWRITE, (len(items) - len(kept), mism, ins + dele, ts, no_motif, conflict)


def twin(raw: bytes, ref: Ref, flags: int):
    """-> (the new array, stats (8 values)); twin_kinds gives the per-record verdicts"""
    out, st = [], [0] * 8
    for at in offsets(raw):
        new, kind, d = one(raw, at, ref, flags)
        out.append(new)
        if kind == NOT_ELIGIBLE:
            st[1] += 1
        elif kind == AUX_BAD:
            st[2] += 1
        else:
            st[0] += 1; st[3] += d[0]; st[4] += d[1]; st[5] += d[2]; st[6] += d[3]; st[7] += d[4] | d[5] << 32
    return b"".join(out), tuple(st)


def twin_kinds(raw: bytes, ref: Ref, flags: int):
    return [(one(raw, at, ref, flags)[1], len(one(raw, at, ref, flags)[0])) for at in offsets(raw)]


# ---- the independent restatement ----
def decode_aux(area: bytes):
    """a generic aux decoder -> [(name, type letter, raw bytes of the whole tag)]; raises ValueError when the area is not a sequence of tags"""
    fixed = dict(A=1, c=1, C=1, s=2, S=2, i=4, I=4, f=4)
    out, view = [], memoryview(area)
    while len(view):
        if len(view) < 3:
            raise ValueError("a tag needs three bytes")
        name, ty = bytes(view[:2]), chr(view[2])
        if ty in fixed:
            n = 3 + fixed[ty]
        elif ty in "ZH":
            n = bytes(view).index(b"\0", 3) + 1          # (ValueError: no NUL)
        elif ty == "B":
            if len(view) < 8 or chr(view[3]) not in "cCsSiIf":
                raise ValueError("B header")
            n = 8 + fixed[chr(view[3])] * int.from_bytes(view[4:8], "little")
        else:
            raise ValueError("type")
        if n > len(view):
            raise ValueError("past the end")
        out.append((name, ty, bytes(view[:n]))); view = view[n:]
    return out


def columns(ref: Ref, tid, pos, ops, letters):
    """one column per CIGAR base: (op letter, read letter or None, reference letter or None, reference position or None)"""
    cols, at, q = [], pos, 0
    for ln, o in ops:
        for _ in range(ln):
            if o in "M=X":
                cols.append((o, letters[q], "ACGT"[ref.base(tid, at)], at)); at += 1; q += 1
            elif o in "DN":
                cols.append((o, None, "ACGT"[ref.base(tid, at)], at)); at += 1
            elif o in "IS":
                cols.append((o, letters[q], None, None)); q += 1
    return cols


def restate(raw: bytes, ref: Ref, flags: int) -> bytes:
    """the second way to the same array: SAM-like fields, per-base columns, MD through a string of column symbols collapsed by a regular expression"""
    out, p = [], 0
    while p + 4 <= len(raw):
        size = 4 + int.from_bytes(raw[p:p + 4], "little")
        rec = raw[p:p + size]; p += size
        keep = lambda: out.append(rec)
        if len(rec) < 36 or len(rec) != size:
            keep(); continue
        tid = int.from_bytes(rec[4:8], "little", signed=True); pos = int.from_bytes(rec[8:12], "little", signed=True)
        flag = rec[18] | rec[19] << 8; n_cig = rec[16] | rec[17] << 8; l_name = rec[12]; l_seq = int.from_bytes(rec[20:24], "little")
        if tid < 0 or tid >= ref.n_chr or pos < 0 or flag & 4 or n_cig == 0 or 36 + l_name + 4 * n_cig > len(rec):
            keep(); continue
        ops = [(int.from_bytes(rec[36 + l_name + 4 * k:40 + l_name + 4 * k], "little") >> 4, "MIDNSHP=X???????"[rec[36 + l_name + 4 * k] & 15]) for k in range(n_cig)]
        sq = 36 + l_name + 4 * n_cig
        aux = sq + (l_seq + 1) // 2 + l_seq
        end, too_far = pos, False
        for l, o in ops:
            if o in "M=X" and l and end + l > pui.MAX_POS:
                too_far = True
            if o in "MDN=X":
                end += l
        if too_far or l_seq == 0 or aux > len(rec) or sum(l for l, o in ops if o in "MIS=X") != l_seq or end > ref.chr_len[tid]:
            keep(); continue
        try:
            tags = decode_aux(rec[aux:])
        except ValueError:
            keep(); continue
        letters = "".join("=ACMGRSVTWYHKDBN"[rec[sq + k // 2] >> 4 if k % 2 == 0 else rec[sq + k // 2] & 15] for k in range(l_seq))
        cols = columns(ref, tid, pos, ops, letters)
        # one symbol per column that MD speaks of: '=' a match, the reference letter a mismatch, its lower case a deleted base
        sym = "".join("=" if o in "M=X" and (a == "=" or a == r) else r if o in "M=X" else r.lower() if o == "D" else "" for o, a, r, _ in cols)
        # a D op of its own starts a new '^' group even right behind another: mark the op boundaries
        marks, k = set(), 0
        for l, o in ops:
            if o == "D" and l:
                marks.add(k)
            if o in "M=XD":
                k += l
        pieces, run, k = [], 0, 0
        for ch in sym:
            if ch == "=":
                run += 1
            elif ch.isupper():
                pieces.append("%d%s" % (run, ch)); run = 0
            else:
                if k in marks:
                    pieces.append("%d^" % run); run = 0
                pieces.append(ch.upper())
            k += 1
        md = "".join(pieces) + "%d" % run
        assert re.fullmatch(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*", md), md
        nm = sum(1 for o, a, r, _ in cols if o in "M=X" and not (a == "=" or a == r)) + sum(l for l, o in ops if o in "ID")
        votes, at = [], pos
        for l, o in ops:
            if o == "N" and l >= 4:
                text = "".join("ACGT"[ref.base(tid, x)] for x in range(at, at + l))
                votes.append({"GTAG": "+", "GCAG": "+", "CTAC": "-", "CTGC": "-"}.get(text[:2] + text[-2:]))
            if o in "MDN=X":
                at += l
        new = [t for name, _, t in tags if not ((name == b"MD" and flags & MD_) or (name == b"NM" and flags & NM_) or (name == b"ts" and flags & TS_))]
        if flags & NM_:
            new.append(b"NM" + (b"C" + bytes([nm]) if nm < 256 else b"S" + nm.to_bytes(2, "little") if nm < 65536 else b"I" + nm.to_bytes(4, "little")))
        if flags & MD_:
            new.append(b"MDZ" + md.encode() + b"\0")
        voted = {v for v in votes if v}
        if flags & TS_ and len(voted) == 1:
            g = voted.pop()
            new.append(b"tsA" + ((g if not flag & 16 else {"+": "-", "-": "+"}[g]).encode()))
        body = rec[4:aux] + b"".join(new)
        out.append(len(body).to_bytes(4, "little") + body)
    return b"".join(out)


def tags_of(rec: bytes):
    """a whole record's aux area, decoded: {name: [raw value bytes, one per occurrence]} with the type letter in front"""
    l_name = rec[12]; n_cig = rec[16] | rec[17] << 8; l_seq = int.from_bytes(rec[20:24], "little")
    out = {}
    for name, ty, t in decode_aux(rec[36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq:]):
        out.setdefault(name, []).append(ty.encode() + t[3:])
    return out


def md_of(rec: bytes):
    v = tags_of(rec).get(b"MD")
    return v[-1][1:-1].decode() if v else None


def nm_of(rec: bytes):
    v = tags_of(rec).get(b"NM")
    return int.from_bytes(v[-1][1:], "little") if v else None


def ts_of(rec: bytes):
    v = tags_of(rec).get(b"ts")
    return v[-1][1:].decode() if v else None


def name_of(rec: bytes):
    return rec[36:36 + rec[12] - 1] if len(rec) > 36 else b""


# ---- aux builders ----
def tA(name, ch): return name + b"A" + ch
def tZ(name, text): return name + b"Z" + text + b"\0"
def tH(name, text): return name + b"H" + text + b"\0"
def tint(name, ty, v): return name + ty.encode() + struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[ty], v)
def tB(name, sub, vals): return name + b"B" + sub.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub], v) for v in vals)


EVERY_TYPE = tA(b"XA", b"q") + tint(b"Xc", "c", -3) + tint(b"XC", "C", 200) + tint(b"Xs", "s", -300) + tint(b"XS", "S", 60000) + tint(b"Xi", "i", -70000) + tint(b"XI", "I", 4000000000) + \
    tint(b"Xf", "f", 1.5) + tZ(b"XZ", b"text") + tZ(b"YZ", b"") + tH(b"XH", b"1AE301") + b"".join(tB(b"B" + sub.encode(), sub, [1, 2, 3]) for sub in "cCsSiIf") + tB(b"B0", "S", [])
OLD_MD, OLD_NM, OLD_TS = tZ(b"MD", b"7"), tint(b"NM", "i", 99), tA(b"ts", b"+")
AS_, XS_ = tint(b"AS", "C", 40), tint(b"XS", "C", 3)


# ---- the reference of the crafted cases: random, with intron motifs planted on chromosome 0 ----
INTRONS = {"gtag": (1200, 50, "GT", "AG"), "gcag": (1260, 50, "GC", "AG"), "ctac": (1320, 50, "CT", "AC"), "ctgc": (1380, 50, "CT", "GC"), "none": (1440, 50, "AA", "AA"),
           "four": (1500, 4, "GT", "AG"), "three": (1520, 3, "GT", "G")}


def _crafted_ref():
    base = random_ref(23, [3000, 2000])
    codes = base.codes.copy()
    for p, ln, head, tail in INTRONS.values():
        for k, ch in enumerate(head):
            codes[p + k] = "ACGT".index(ch)
        for k, ch in enumerate(tail):
            codes[p + ln - len(tail) + k] = "ACGT".index(ch)
    return Ref(codes, base.chr_len)


REF = _crafted_ref()
NAMES = [b"chrA", b"b"]


def _rec(tid, pos, flag, name, cigar, edits=(), tags=b"", R=None):
    R = R or REF
    return record(tid, pos, flag, name, cigar, read_of(R, tid, pos, cigar, edits), tags=tags)


def lying_records(R=None):
    """records whose block_size lies -- dg_bam_sort_add refuses them, only the lane code's tests see them; each must be the LAST record of its array"""
    R = R or REF
    whole = _rec(0, 900, 0, b"cut", [(30, M)], {29: "!"}, AS_)
    short = bytearray(whole[:len(whole) - len(AS_) - 5]); struct.pack_into("<I", short, 0, len(short) - 4)          # block_size ends inside the qualities
    return {"liar_n_cigar": pui.liar(R), "behind_the_array": whole[:len(whole) - 2], "inside_the_qualities": bytes(short), "twenty_bytes": whole[:20]}


def crafted_cases(R=None):
    """name -> records (any order); all on REF's shape (chromosome 0 with the planted introns, at least 3000 and 2000 bases).  Every record passes dg_bam_sort_add."""
    R = R or REF
    L0, L1 = R.chr_len
    r = lambda *a, **k: _rec(*a, R=R, **k)
    step = [r(0, 100 + 50 * j, 0, b"m%d" % n, [(n, M)], {n - 1: "!"}, AS_) for j, n in enumerate((1, 15, 16, 17, 31, 32, 33))] + \
           [r(0, 100 + 50 * j, 16, b"m%d_clean" % n, [(n, M)]) for j, n in enumerate((1, 15, 16, 17, 31, 32, 33))] + \
           [r(0, 500, 0, b"at15", [(40, M)], {15: "!"}), r(0, 500, 0, b"at16", [(40, M)], {16: "!"}), r(0, 500, 0, b"at15_16", [(40, M)], {15: "!", 16: "!"}),
            r(0, 600, 0, b"odd_start_s", [(1, S), (37, M)], {1: "!", 17: "!", 37: "!"}), r(0, 600, 0, b"odd_start_i", [(3, I), (35, M)], {3: "!", 19: "!"}),
            r(0, 600, 0, b"odd_then_even", [(5, M), (3, I), (20, M), (1, I), (20, M)], {4: "!", 8: "!", 28: "!", 29: "!"})] + \
           [r(0, 1000 + k, 0, b"pos_mod4_%d" % k, [(40, M)], {0: "!", 15 - k: "!", 16: "!", 39: "!"}) for k in range(4)] + \
           [r(1, L1 - 20, 0, b"last_of_last", [(20, M)], {19: "!"}), r(1, L1 - 40, 0, b"last_of_last_40", [(40, M)], {0: "!", 39: "!"}), r(1, L1 - 17, 16, b"last_of_last_17", [(17, M)], {16: "!"}),
            r(1, L1 - 1, 0, b"the_last_base", [(1, M)], {0: "!"}), r(0, L0 - 20, 0, b"last_of_first", [(20, M)], {19: "!"}), r(0, L0 - 33, 0, b"last_of_first_33", [(33, M)], {32: "!", 16: "!"})]
    text = [r(0, 100, 0, b"run%d" % n, [(2 * n + 1, M)], {n: "!"}) for n in (9, 10, 99, 100)] + \
           [r(0, 400, 0, b"side_by_side", [(20, M)], {5: "!", 6: "!"}), r(0, 400, 0, b"first_and_last", [(20, M)], {0: "!", 19: "!"}),
            r(0, 450, 0, b"d_then_mismatch", [(10, M), (2, D), (10, M)], {10: "!"}), r(0, 450, 0, b"two_d", [(10, M), (2, D), (3, D), (10, M)]),
            r(0, 450, 0, b"d_over_seam", [(14, M), (5, D), (20, M)], {13: "!"}), r(0, 450, 0, b"d_zero", [(10, M), (0, D), (10, M)]), r(0, 450, 0, b"d_first_op", [(2, D), (10, M)]),
            r(0, 500, 0, b"i_first", [(3, I), (20, M)]), r(0, 500, 16, b"i_last", [(20, M), (3, I)]), r(0, 520, 0, b"s_both", [(4, S), (20, M), (3, S)], {4: "!", 23: "!"}),
            r(0, 540, 0, b"h_p", [(5, H), (10, M), (6, P), (10, M), (7, H)], {9: "!", 10: "!"}), r(0, 560, 0, b"l_seq_1", [(1, M)]), r(0, 560, 0, b"l_seq_1_s", [(1, S)]),
            r(0, 1600, 0, b"thousand", [(1000, M)], {k: "!" for k in range(1000)}), r(0, 1600, 16, b"thousand_x", [(1000, X)], {k: "!" for k in range(0, 1000, 2)})] + \
           [record(0, 700 + k, 0, b"nibbles%d" % k, [(16, M)], "=ACMGRSVTWYHKDBN") for k in range(4)] + [record(0, 705, 0, b"nibbles_odd", [(1, S), (16, EQ)], "A=ACMGRSVTWYHKDBN")]
    nm = [r(0, 100, 0, b"nm255", [(300, M)], {k: "!" for k in range(255)}), r(0, 100, 0, b"nm256", [(300, M)], {k: "!" for k in range(256)}),
          r(0, 100, 0, b"nm255_indel", [(100, M), (100, I), (100, M), (154, D), (10, M)], {0: "!"}), r(0, 100, 0, b"nm256_indel", [(100, M), (100, I), (100, M), (155, D), (10, M)], {0: "!"}),
          r(0, 100, 0, b"nm0", [(30, M)], tags=OLD_NM)]
    ts = []
    for name in ("gtag", "gcag", "ctac", "ctgc", "none", "four", "three"):
        p, ln = INTRONS[name][:2]
        ts += [r(0, p - 10, 0, name.encode(), [(10, M), (ln, N), (10, M)], {9: "!"}, AS_), r(0, p - 10, 16, name.encode() + b"_rev", [(10, M), (ln, N), (10, M)], {10: "!"}),
               r(0, p - 10, 0x91, name.encode() + b"_mate2_rev", [(10, M), (ln, N), (10, M)])]
    two = lambda a, b: [(10, M), (50, N), (INTRONS[b][0] - INTRONS[a][0] - 50, M), (INTRONS[b][1], N), (10, M)]
    ts += [r(0, 1190, 0, b"two_agree", two("gtag", "gcag")), r(0, 1190, 16, b"two_agree_rev", two("gtag", "gcag")), r(0, 1250, 0, b"two_conflict", two("gcag", "ctac")),
           r(0, 1310, 16, b"two_minus", two("ctac", "ctgc")), r(0, 1370, 0, b"canonical_and_not", two("ctgc", "none")), r(0, 1430, 0, b"not_and_short", two("none", "four")),
           r(0, 1190, 0, b"old_ts_no_new", [(30, M)], tags=OLD_TS), r(0, 1190, 0, b"intron_at_the_start", [(1, M), (9, D), (50, N), (10, M)])]
    aux = [r(0, 100, 0, b"every_type", [(20, M)], {3: "!"}, EVERY_TYPE), r(0, 100, 0, b"no_aux", [(20, M)], {3: "!"}),
           r(0, 100, 0, b"old_first", [(20, M)], {3: "!"}, OLD_MD + OLD_NM + OLD_TS + AS_ + XS_), r(0, 100, 0, b"old_middle", [(20, M)], {3: "!"}, AS_ + OLD_NM + XS_ + OLD_MD + EVERY_TYPE + OLD_TS + XS_[:2] + b"Z\0"),
           r(0, 100, 0, b"old_last", [(20, M)], {3: "!"}, AS_ + XS_ + OLD_TS + OLD_NM + OLD_MD), r(0, 100, 0, b"old_twice", [(20, M)], {3: "!"}, OLD_MD + AS_ + OLD_MD + OLD_NM + OLD_NM + XS_ + OLD_TS + OLD_TS),
           r(0, 100, 0, b"old_only", [(20, M)], {3: "!"}, OLD_NM), r(0, 100, 0, b"old_other_types", [(20, M)], {3: "!"}, tint(b"MD", "i", 5) + tZ(b"NM", b"seven") + tB(b"ts", "c", [1, 2])),
           r(0, 100, 0, b"unknown_type", [(20, M)], {3: "!"}, AS_ + b"XQq\x01" + XS_), r(0, 100, 0, b"z_without_nul", [(20, M)], {3: "!"}, AS_ + b"XZZabc"),
           r(0, 100, 0, b"b_past_the_end", [(20, M)], {3: "!"}, AS_ + b"XBBi" + struct.pack("<I", 3) + bytes(8)), r(0, 100, 0, b"b_bad_subtype", [(20, M)], {3: "!"}, b"XBBZ" + struct.pack("<I", 0)),
           r(0, 100, 0, b"b_huge_count", [(20, M)], {3: "!"}, b"XBBI" + struct.pack("<I", 0xFFFFFFFF)), r(0, 100, 0, b"two_bytes_left", [(20, M)], {3: "!"}, AS_ + b"XY"),
           r(0, 100, 0, b"value_cut", [(20, M)], {3: "!"}, AS_ + b"XIi\x01\x02"), r(0, 100, 0, b"old_md_unreadable_behind", [(20, M)], {3: "!"}, OLD_MD + b"XZZabc")]
    far = [(1 << 28) - 1, N]
    not_eligible = [record(-1, -1, 4, b"unplaced", [], "ACGT", tags=OLD_NM), _rec(0, 20, 4, b"unmapped_with_pos", [(10, M)], {1: "!"}, OLD_NM, R=R), record(0, 10, 0, b"no_cigar", [], "ACGTACGTAC", tags=OLD_MD),
                    record(0, 700, 0, b"l_seq_0", [(20, M)], "", tags=OLD_MD), record(0, 700, 0, b"l_seq_short", [(20, M)], "A" * 19), record(0, 700, 0, b"l_seq_long", [(20, M)], "A" * 21),
                    r(0, L0 - 19, 0, b"one_past_chr0", [(20, M)], {3: "!"}), r(1, L1 - 10, 0, b"d_past_chr1", [(5, M), (6, D)], {2: "!"}), r(1, L1 - 10, 0, b"n_past_chr1", [(5, M), (600, N), (5, M)]),
                    r(0, -1, 0, b"pos_m1", [(10, M)]), record(1, (1 << 31) - 1, 0, b"out_of_range", [tuple(far)] * 8 + [(9, M)], "ACGTACGTA", tags=OLD_NM),
                    r(0, 200, 0, b"the_one_that_counts", [(10, M)], {1: "!"}, OLD_NM)]
    return {"step": step, "text": text, "nm": nm, "ts": ts, "aux": aux, "not_eligible": not_eligible, "empty": []}


def sort_records(recs, n_chr=2):
    return sorted(recs, key=lambda x: bsi.key(x, n_chr))


def with_old_tags(recs, rng):
    """the records with an old NM:i (as the mapper writes it), and now and then an old MD or ts, behind whatever aux they have"""
    out = []
    for x in recs:
        extra = tint(b"NM", "C", rng.randrange(0, 9)) + tint(b"AS", "C", rng.randrange(0, 200)) + (OLD_MD if rng.random() < 0.1 else b"") + (OLD_TS if rng.random() < 0.1 else b"")
        body = x[4:] + extra
        out.append(struct.pack("<I", len(body)) + body)
    return out


# ---- the native program ----
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "tags_checks_san" if sanitize else "tags_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "tags_checks.hip")])
    return exe


def run_program(exe, workdir, tag, ref: Ref, raw: bytes, flags: int):
    """-> dict(out = the new array, recs = [(kind, new size)], stats = the eight)"""
    src = os.path.join(workdir, "tg_%s.in" % tag); txt = os.path.join(workdir, "tg_%s.txt" % tag); out = os.path.join(workdir, "tg_%s.bin" % tag)
    pac = ref.pac()
    pad = lambda b: b + bytes(-len(b) % 8)
    with open(src, "wb") as f:
        f.write(struct.pack("<8q", ref.n_chr, flags, len(raw), len(ref.codes), len(pac), 0, 0, 0))
        f.write(struct.pack("<%dq" % ref.n_chr, *ref.chr_off) + struct.pack("<%dq" % ref.n_chr, *ref.chr_len))
        f.write(pad(pac) + raw)
    r = subprocess.run([exe, src, txt, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    res = dict(out=open(out, "rb").read(), recs=[], stats=None)
    for line in open(txt).read().splitlines():
        w = line.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "rec":
            res["recs"].append((v[1], v[2]))
        elif w[0] == "stats":
            res["stats"] = tuple(v)
    return res
