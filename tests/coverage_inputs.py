"""Helpers of the coverage-track tests: the sequential Python twin of the definition in dart_amd/csrc/dg_coverage.h (events in a dictionary, one walk over the
sorted keys -- record by record, not as the kernels' scans), a second, independent check (a per-base numpy depth array, run-length encoded), hand-made records
that each hold what they are named for, and the native program tests/native/coverage_checks.hip.  The definition is the header's comment: no bedtools or
samtools exists where these tests run."""
from __future__ import annotations

import os, struct, subprocess
import numpy as np
import common
import bamsort_inputs as bsi
from bamidx_inputs import record, offsets, M, I, D, N, S, H, P, EQ, X

MAX_POS = (1 << 32) - 1
DEFAULT_EXCLUDE = 0x704
ENTRY = np.dtype([("chr", "<u4"), ("start", "<u4"), ("end", "<u4"), ("depth", "<u4")])
PER_BASE_LIMIT = 1 << 20                                        # the per-base check looks at positions below this


class RangeError(Exception):
    """a counted record has a block that ends behind 2^32 - 1 (args[0] = its index)"""


def counted(raw: bytes, at: int, n_chr: int, exclude: int, min_mapq: int, strand):
    """-> (refid, pos, [CIGAR words]) of a counted record, else None"""
    bs, refid, pos = struct.unpack_from("<Iii", raw, at)
    l_name, mapq = raw[at + 12], raw[at + 13]
    n_cig, flag = struct.unpack_from("<HH", raw, at + 16)
    if not (0 <= refid < n_chr and pos >= 0 and not flag & 4 and n_cig > 0 and not flag & exclude and mapq >= min_mapq):
        return None
    s = (flag >> 4 & 1) ^ (flag >> 7 & 1)
    if strand is not None and s != {"+": 0, "-": 1}[strand]:
        return None
    if 36 + l_name + 4 * n_cig > min(4 + bs, len(raw) - at):
        return None
    return refid, pos, struct.unpack_from("<%dI" % n_cig, raw, at + 36 + l_name)


def blocks_of(pos, cigar):
    out, p = [], pos
    for c in cigar:
        op, ln = c & 15, c >> 4
        if op in (M, EQ, X):
            if ln:
                out.append((p, p + ln))
            p += ln
        elif op in (D, N):
            p += ln
    return out


def twin(raw: bytes, n_chr: int, exclude=DEFAULT_EXCLUDE, min_mapq=0, strand=None):
    """-> (entries [(chr, start, end, depth)], stats (7 values)); raises RangeError(index of the first record out of range)"""
    ev, n_counted, n_blocks, aligned = {}, 0, 0, 0
    for i, at in enumerate(offsets(raw)):
        c = counted(raw, at, n_chr, exclude, min_mapq, strand)
        if c is None:
            continue
        n_counted += 1
        for s, e in blocks_of(c[1], c[2]):
            if e > MAX_POS:
                raise RangeError(i)
            n_blocks += 1; aligned += e - s
            ev[(c[0], s)] = ev.get((c[0], s), 0) + 1
            ev[(c[0], e)] = ev.get((c[0], e), 0) - 1
    bps = sorted(k for k, d in ev.items() if d)
    entries, depth, deepest = [], 0, 0
    for q, k in enumerate(bps):
        depth += ev[k]
        assert depth >= 0
        deepest = max(deepest, depth)
        if depth:
            assert bps[q + 1][0] == k[0]
            entries.append((k[0], k[1], bps[q + 1][1], depth))
    assert depth == 0
    covered = sum(e - s for _, s, e, _ in entries)
    assert sum((e - s) * d for _, s, e, d in entries) == aligned
    return entries, (n_counted, n_blocks, len(bps), len(entries), covered, aligned, deepest)


def text_of(entries, names) -> bytes:
    return b"".join(b"%s\t%d\t%d\t%d\n" % (names[c], s, e, d) for c, s, e, d in entries)


def as_array(entries):
    return np.array(entries, dtype=ENTRY) if entries else np.zeros(0, ENTRY)


def per_base(raw: bytes, n_chr: int, exclude=DEFAULT_EXCLUDE, min_mapq=0, strand=None, limit=PER_BASE_LIMIT):
    """the independent check: one depth counter per base of [0, limit) of every chromosome, bumped base range by base range, then run-length encoded ->
    entries, to be compared with clip(twin's entries, limit).  Its own field reads and CIGAR walk (position by position over the op list as SAM text would
    be read: consumes-reference ops move, M = X count)."""
    depth = np.zeros((n_chr, limit), np.int64)
    p = 0
    while p < len(raw):
        size = 4 + int.from_bytes(raw[p:p + 4], "little")
        rec = raw[p:p + size]; p += size
        refid = int.from_bytes(rec[4:8], "little", signed=True); pos = int.from_bytes(rec[8:12], "little", signed=True)
        flag = rec[18] | rec[19] << 8; n_cig = rec[16] | rec[17] << 8; l_name = rec[12]
        if refid < 0 or refid >= n_chr or pos < 0 or flag & 4 or n_cig == 0 or flag & exclude or rec[13] < min_mapq:
            continue
        rev = bool(flag & 16) != bool(flag & 128)
        if (strand == "+" and rev) or (strand == "-" and not rev):
            continue
        if 36 + l_name + 4 * n_cig > len(rec):
            continue
        at = pos
        for k in range(n_cig):
            w = int.from_bytes(rec[36 + l_name + 4 * k:40 + l_name + 4 * k], "little")
            ch = "MIDNSHP=X"[w & 15] if w & 15 < 9 else "?"
            if ch in "M=X":
                depth[refid, min(at, limit):min(at + (w >> 4), limit)] += 1
            if ch in "M=XDN":
                at += w >> 4
    out = []
    for t in range(n_chr):
        row = depth[t]
        cuts = np.flatnonzero(np.diff(row)) + 1
        starts = np.concatenate(([0], cuts)); ends = np.concatenate((cuts, [limit]))
        out += [(t, int(s), int(e), int(row[s])) for s, e in zip(starts, ends) if row[s]]
    return out


def clip(entries, limit=PER_BASE_LIMIT):
    return [(c, s, min(e, limit), d) for c, s, e, d in entries if s < limit]


# the filter settings every case is run with: (exclude, min_mapq, strand)
FILTERS = [(DEFAULT_EXCLUDE, 0, None), (4, 0, None), (0x100 | 4, 0, None), (0x200 | 4, 0, None), (0x400 | 4, 0, None), (DEFAULT_EXCLUDE, 10, None), (DEFAULT_EXCLUDE, 0, "+"),
           (DEFAULT_EXCLUDE, 0, "-")]
ALL_OPS = [(5, S), (10, M), (2, I), (3, D), (700, N), (4, EQ), (1, X), (6, P), (7, H)]         # every op code 0..8: blocks [100, 110), [813, 817), [817, 818)
TO_THE_EDGE = [((1 << 28) - 1, N)] * 8                                                           # from pos 2^31 - 1 to 2^32 - 9


def liar():
    """n_cigar_op says 60000 ops, block_size holds one: the record counts for nothing (dg_bam_sort_add refuses it: only the lane code's tests see it)"""
    r = bytearray(record(0, 50, 0, b"liar", [(10, M)], l_seq=10)); struct.pack_into("<H", r, 16, 60000)
    return bytes(r)


def crafted_cases():
    """name -> (n_chr, records in coordinate order, chromosome names)"""
    rec = lambda tid, pos, flag, name, cigar, mapq=30: record(tid, pos, flag, name, cigar, l_seq=sum(l for l, op in cigar if op in (M, I, S, EQ, X)), mapq=mapq)
    cigar = [
        rec(0, 100, 0, b"all_ops", ALL_OPS),
        rec(0, 300, 0, b"zero_m_first", [(0, M), (5, M)]), rec(0, 320, 0, b"zero_m_only", [(0, M)]),
        rec(0, 400, 0, b"abut_across_i", [(10, M), (3, I), (10, M)]),
        rec(0, 500, 0, b"n_gap", [(10, M), (50, N), (10, M)]),
        rec(0, 1000, 0, b"d_under", [(10, M), (5, D), (10, M)]), rec(0, 1000, 0, b"over_the_d", [(25, M)]),
        rec(0, 2000, 0, b"d_alone", [(10, M), (5, D), (10, M)]),
    ]
    depth = [
        rec(0, 100, 0, b"a", [(50, M)]), rec(0, 150, 0, b"b_begins_where_a_ends", [(50, M)]),
        rec(0, 300, 0, b"c", [(50, M)]), rec(0, 350, 0, b"d1", [(50, M)]), rec(0, 350, 0, b"d2", [(50, M)]),
    ] + [rec(0, 1000, 16 if k & 1 else 0, b"pile%d" % k, [(50, M)]) for k in range(12)] + [rec(1, p, 0, b"digits%d" % len(str(p)), [(3, M)]) for p in [7 * 10 ** k for k in range(9)] + [2 * 10 ** 9]]
    edge = [rec(0, 0, 0, b"pos0", [(5, M)]), rec(1, (1 << 31) - 1, 0, b"ends_at_2_32_m1", TO_THE_EDGE + [(8, M)])]
    edge_bad = [rec(0, 0, 0, b"pos0", [(5, M)]), rec(0, 7, 0x400, b"a_duplicate_out_of_range", TO_THE_EDGE[:1] * 17 + [(8, M)]), rec(1, (1 << 31) - 1, 0, b"ends_at_2_32", TO_THE_EDGE + [(9, M)])]
    nothing = [
        rec(0, -1, 0, b"pos_m1", [(10, M)]), record(0, 10, 0, b"no_cigar", l_seq=10), rec(0, 20, 4, b"placed_unmapped", [(10, M)]),
        rec(0, 200, 0, b"the_one_that_counts", [(10, M)]), record(-1, -1, 4, b"unplaced", l_seq=10), rec(-1, 30, 0, b"unplaced_with_cigar", [(10, M)]),
    ]
    filters = [rec(0, 100, 0x100, b"secondary", [(10, M)]), rec(0, 200, 0x200, b"qcfail", [(10, M)]), rec(0, 300, 0x400, b"duplicate", [(10, M)]),
               rec(0, 400, 0, b"mapq10", [(10, M)], mapq=10), rec(0, 500, 0, b"mapq9", [(10, M)], mapq=9),
               rec(1, 100, 0, b"unpaired_fwd", [(10, M)]), rec(1, 200, 16, b"unpaired_rev", [(10, M)]),
               rec(1, 300, 0x41, b"mate1_fwd", [(10, M)]), rec(1, 400, 0x51, b"mate1_rev", [(10, M)]), rec(1, 500, 0x81, b"mate2_fwd", [(10, M)]), rec(1, 600, 0x91, b"mate2_rev", [(10, M)])]
    refs = [rec(0, 90, 0, b"ends_at_100", [(10, M)]), rec(2, 100, 0, b"begins_at_100", [(10, M)]), rec(3, 110, 0, b"begins_where_ref2_ends", [(5, M)])]
    two, four = [b"chrA", b"b"], [b"one", b"empty_middle", b"three", b"a_longer_name_4"]
    srt = lambda recs, n: sorted(recs, key=lambda r: bsi.key(r, n))
    return {
        "cigar": (2, srt(cigar, 2), two), "depth": (2, srt(depth, 2), two), "edge": (2, srt(edge, 2), two), "edge_bad": (2, srt(edge_bad, 2), two),
        "nothing": (2, srt(nothing, 2), two), "nothing_liar": (2, srt(nothing[:4] + [liar()], 2) + nothing[4:], two), "filters": (2, srt(filters, 2), two),
        "refs": (4, srt(refs, 4), four), "empty": (3, [], [b"x", b"y", b"z"]),
    }


def random_records(rng, n, n_chr, span=3000):
    """n records with CIGARs of every op, clustered so that depths rise and keys collide; a few that count for nothing"""
    out = []
    for k in range(n):
        ops = []
        for _ in range(rng.randrange(1, 6)):
            ops.append((rng.choice([0, 1, 2, 5, 30, 101]), rng.choice([M, M, M, I, D, N, S, EQ, X, H, P])))
        flag = rng.choice([0, 16, 0x41, 0x91, 0x51, 0x81, 0x100, 0x400, 4])
        tid = rng.randrange(-1, n_chr)
        grid = rng.choice([1, 50])
        pos = rng.choice([-1] + [rng.randrange(0, span) // grid * grid] * 30) if tid >= 0 else -1
        out.append(record(tid, pos, flag, b"r%d" % k, ops, l_seq=0, mapq=rng.randrange(0, 40)))
    return out


# ---- the native program ----
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "coverage_checks_san" if sanitize else "coverage_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "coverage_checks.hip")])
    return exe


def flags_of(strand, entries_only=False):
    return (1 if entries_only else 0) | {None: 0, "+": 2, "-": 4}[strand]


def run_program(exe, workdir, tag, n_chr, raw, names, exclude=DEFAULT_EXCLUDE, min_mapq=0, strand=None):
    """-> dict(recs = [(counted, blocks)], blocks = [(record, start, end)], events = [(key, delta)] sorted, bps = [(key, depth)], entries = [(chr, start, end,
    depth)], stats = the seven, bad = index of the first record out of range or None, text = the bytes)"""
    src = os.path.join(workdir, "cov_%s.in" % tag); txt = os.path.join(workdir, "cov_%s.txt" % tag); out = os.path.join(workdir, "cov_%s.bedgraph" % tag)
    name_off = [0]
    for nm in names:
        name_off.append(name_off[-1] + len(nm))
    with open(src, "wb") as f:
        f.write(struct.pack("<6q", n_chr, flags_of(strand), exclude, min_mapq, len(raw), name_off[-1]))
        off = struct.pack("<%dI" % (n_chr + 1), *name_off)
        f.write(off + bytes(-len(off) % 8) + b"".join(names) + bytes(-name_off[-1] % 8) + raw)
    r = subprocess.run([exe, src, txt, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    res = dict(recs=[], blocks=[], events=[], bps=[], entries=[], stats=None, bad=None, text=open(out, "rb").read())
    for line in open(txt).read().splitlines():
        w = line.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "rec":
            res["recs"].append((v[1], v[2]))
        elif w[0] == "blk":
            res["blocks"].append(tuple(v))
        elif w[0] == "ev":
            res["events"].append(tuple(v))
        elif w[0] == "bp":
            res["bps"].append(tuple(v))
        elif w[0] == "ent":
            res["entries"].append(tuple(v))
        elif w[0] == "stats":
            res["stats"] = tuple(v)
        elif w[0] == "bad":
            res["bad"] = v[0]
    return res
