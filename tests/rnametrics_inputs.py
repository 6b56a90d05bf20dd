"""Helpers of the RNA-seq metrics tests: the sequential Python twin of the definition in dart_amd/csrc/dg_rnametrics.h (elementary intervals between the
annotation's boundaries, a bisect per block, events in a dictionary -- record by record, not as the kernels' sums), a second, independent restatement (`paint`:
class and strands painted per base, depth counted per base; for chromosomes of a few kb), hand-made annotations and records that each hold what they are named
for, and the native program tests/native/rnametrics_checks.hip.  The definition is the header's comment: no Picard or RSeQC exists where these tests run."""
from __future__ import annotations

import bisect, os, struct, subprocess
import numpy as np
import common
import coverage_inputs as cvi
from bamidx_inputs import record, offsets, M, I, D, N, S, H, P, EQ, X

MAX_POS = (1 << 32) - 1
DEFAULT_EXCLUDE, DEFAULT_MIN_COV = 0x904, 100
RIBOSOMAL = 1
TX = np.dtype([("chr", "<i4"), ("strand", "<u4"), ("flags", "<u4"), ("cds_start", "<u4"), ("cds_end", "<u4"), ("n_exons", "<u4"), ("first_exon", "<u8")])      # dg_rna_tx
EXON = np.dtype([("start", "<u4"), ("end", "<u4")])                                                                                                  # dg_rna_exon
OFF = dict(BA=0, RC=5, ST=10, BC=14, SN=314, words=330)
SN_NAMES = ["records", "counted", "blocks", "aligned_bases", "transcripts", "eligible_transcripts", "contributing_transcripts", "segments"]
SN = {n: k for k, n in enumerate(SN_NAMES)}
CLASS_NAMES = ["intergenic", "intronic", "utr", "coding", "ribosomal"]
ST_NAMES = ["sense", "antisense", "ambiguous", "intergenic"]
FILTERS = [(DEFAULT_EXCLUDE, 0), (0x704, 0), (4, 0), (DEFAULT_EXCLUDE, 10), (0x400 | 4, 0)]
RangeError = cvi.RangeError


def tx(chr, strand, exons, cds=(0, 0), flags=0):
    """a transcript: exons [(start, end)] in any order"""
    return dict(chr=chr, strand=strand, flags=flags, cds=tuple(cds), exons=[tuple(e) for e in exons])


def pack(annot):
    """-> (TX array, EXON array) as dg_rna_annot wants them"""
    t = np.zeros(len(annot), TX); ex = []
    for k, a in enumerate(annot):
        t[k] = (a["chr"], a["strand"], a["flags"], a["cds"][0], a["cds"][1], len(a["exons"]), len(ex))
        ex += a["exons"]
    return t, np.array(ex, EXON) if ex else np.zeros(0, EXON)


def merged(a):
    out = []
    for s, e in sorted(a["exons"]):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return [tuple(x) for x in out]


def class_of(a, p):
    """(class, strands) that transcript a alone gives base p; (0, 0) outside its span"""
    m = merged(a)
    if not m[0][0] <= p < m[-1][1]:
        return 0, 0
    cls = 1
    if any(s <= p < e for s, e in m):
        cls = 4 if a["flags"] & RIBOSOMAL else 3 if a["cds"][0] <= p < a["cds"][1] else 2
    return cls, 1 << a["strand"]


def flatten(annot, n_chr):
    """-> (per chromosome ([segment starts], [(class, strands)]), the eligible transcripts [(chr, strand, L, merged exons)])"""
    segs = []
    for c in range(n_chr):
        here = [a for a in annot if a["chr"] == c]
        cuts = set()
        for a in here:
            m = merged(a)
            cuts.update(x for se in m for x in se)
            cuts.update(min(max(x, m[0][0]), m[-1][1]) for x in a["cds"])
        starts, pairs, prev = [], [], (0, 0)
        for p in sorted(cuts):
            now = (max([class_of(a, p)[0] for a in here] + [0]), sum({class_of(a, p)[1] for a in here}))
            if now != prev:
                starts.append(p); pairs.append(now); prev = now
        segs.append((starts, pairs))
    elig = [(a["chr"], a["strand"], sum(e - s for s, e in merged(a)), merged(a)) for a in annot]
    return segs, [t for t in elig if t[2] >= 100]


def sample_positions(t):
    c, strand, L, m = t
    out = []
    for b in range(100):
        o = (2 * b + 1) * L // 200
        if strand:
            o = L - 1 - o
        for s, e in m:
            if o < e - s:
                out.append(s + o); break
            o -= e - s
    return out


def counted_records(raw, n_chr, exclude, min_mapq):
    """-> (number of records, [(index, refid, flag, blocks)] of the counted ones); raises RangeError(index of the first record out of range)"""
    out, offs = [], offsets(raw)
    for i, at in enumerate(offs):
        c = cvi.counted(raw, at, n_chr, exclude, min_mapq, None)
        if c is None:
            continue
        blocks = cvi.blocks_of(c[1], c[2])
        if any(e > MAX_POS for s, e in blocks):
            raise RangeError(i)
        out.append((i, c[0], struct.unpack_from("<H", raw, at + 18)[0], blocks))
    return len(offs), out


def st_row(flag, b):
    s = (flag >> 4 & 1) ^ (flag >> 7 & 1)
    return 3 if b == 0 else 2 if b == 3 else 0 if s == (1 if b == 2 else 0) else 1


def body(words, elig, depth_at, min_cov):
    """the BC rows and SN.contributing from depth_at(chr, g) -> the list of every eligible transcript's S"""
    sums = []
    for t in elig:
        d = [depth_at(t[0], g) for g in sample_positions(t)]
        sums.append(sum(d))
        if sums[-1] >= max(min_cov, 1):
            words[OFF["SN"] + SN["contributing_transcripts"]] += 1
            for b in range(100):
                words[OFF["BC"] + b] += d[b]; words[OFF["BC"] + 100 + b] += int(d[b] > 0); words[OFF["BC"] + 200 + b] += d[b] * 100000 // sums[-1]
    return sums


def twin(raw: bytes, n_chr: int, annot, exclude=DEFAULT_EXCLUDE, min_mapq=0, min_cov=DEFAULT_MIN_COV, want_sums=False):
    """-> the words (uint64 [330]); raises RangeError"""
    w = [0] * OFF["words"]
    segs, elig = flatten(annot, n_chr)
    n, recs = counted_records(raw, n_chr, exclude, min_mapq)
    ev = {}
    for i, c, flag, blocks in recs:
        starts, pairs = segs[c]
        top, bits = 0, 0
        for s, e in blocks:
            k = max(bisect.bisect_right(starts, s) - 1, 0)
            left = e - s
            while k < len(starts) and starts[k] < e:
                a, b = max(starts[k], s), min(starts[k + 1], e) if k + 1 < len(starts) else e
                w[OFF["BA"] + pairs[k][0]] += b - a; left -= b - a
                top = max(top, pairs[k][0]); bits |= pairs[k][1]
                k += 1
            w[OFF["BA"]] += left
            ev[c, s] = ev.get((c, s), 0) + 1; ev[c, e] = ev.get((c, e), 0) - 1
        w[OFF["RC"] + top] += 1; w[OFF["ST"] + st_row(flag, bits)] += 1
        w[OFF["SN"] + SN["blocks"]] += len(blocks)
    keys = sorted(ev)
    run, depth = 0, []
    for k in keys:
        run += ev[k]; depth.append(run)

    def depth_at(c, g):
        j = bisect.bisect_right(keys, (c, g))
        return depth[j - 1] if j else 0
    sums = body(w, elig, depth_at, min_cov)
    sn = OFF["SN"]
    w[sn + SN["records"]] = n; w[sn + SN["counted"]] = len(recs); w[sn + SN["aligned_bases"]] = sum(w[:5]); w[sn + SN["transcripts"]] = len(annot)
    w[sn + SN["eligible_transcripts"]] = len(elig); w[sn + SN["segments"]] = sum(len(s[0]) for s in segs)
    words = np.array(w, np.uint64)
    return (words, sums) if want_sums else words


def paint(raw: bytes, n_chr: int, annot, exclude=DEFAULT_EXCLUDE, min_mapq=0, min_cov=DEFAULT_MIN_COV):
    """the independent restatement: class and strands per base, depth per base -> the words.  For chromosomes of a few kb."""
    n, recs = counted_records(raw, n_chr, exclude, min_mapq)
    size = 2 + max([e for r in recs for s, e in r[3]] + [e for a in annot for s, e in a["exons"]] + [0])
    assert size < 1 << 16, "paint is for small chromosomes"
    cls = np.zeros((n_chr, size), np.int64); strands = np.zeros((n_chr, size), np.int64); depth = np.zeros((n_chr, size), np.int64)
    for a in annot:
        lo, hi = min(s for s, e in a["exons"]), max(e for s, e in a["exons"])
        mine = np.zeros(size, np.int64); mine[lo:hi] = 1
        for s, e in a["exons"]:
            mine[s:e] = 2
        if a["flags"] & RIBOSOMAL:
            mine[mine == 2] = 4
        else:
            inside = np.zeros(size, bool); inside[a["cds"][0]:a["cds"][1]] = True
            mine[(mine == 2) & inside] = 3
        cls[a["chr"]] = np.maximum(cls[a["chr"]], mine); strands[a["chr"], lo:hi] |= 1 << a["strand"]
    w = np.zeros(OFF["words"], np.uint64)
    for i, c, flag, blocks in recs:
        seen_cls, seen_str = [0], [0]
        for s, e in blocks:
            w[OFF["BA"]:OFF["BA"] + 5] += np.bincount(cls[c, s:e], minlength=5).astype(np.uint64)
            seen_cls.append(int(cls[c, s:e].max())); seen_str.append(int(np.bitwise_or.reduce(strands[c, s:e])))
            depth[c, s:e] += 1
        w[OFF["RC"] + max(seen_cls)] += 1; w[OFF["ST"] + st_row(flag, int(np.bitwise_or.reduce(seen_str)))] += 1
        w[OFF["SN"] + SN["blocks"]] += len(blocks)
    n_elig = 0
    for a in annot:
        covered = np.zeros(size, bool)
        for s, e in a["exons"]:
            covered[s:e] = True
        g = np.flatnonzero(covered)                          # the transcript's bases, left to right
        if len(g) < 100:
            continue
        n_elig += 1
        if a["strand"]:
            g = g[::-1]
        d = [int(depth[a["chr"], g[(2 * b + 1) * len(g) // 200]]) for b in range(100)]
        if sum(d) >= max(min_cov, 1):
            w[OFF["SN"] + SN["contributing_transcripts"]] += 1
            for b in range(100):
                w[OFF["BC"] + b] += d[b]; w[OFF["BC"] + 100 + b] += int(d[b] > 0); w[OFF["BC"] + 200 + b] += d[b] * 100000 // sum(d)
    pair = cls * 4 + strands
    n_seg = sum(int(np.count_nonzero(np.diff(np.concatenate([[0], pair[c]])))) for c in range(n_chr))
    sn = OFF["SN"]
    w[sn + SN["records"]] = n; w[sn + SN["counted"]] = len(recs); w[sn + SN["aligned_bases"]] = w[:5].sum(); w[sn + SN["transcripts"]] = len(annot)
    w[sn + SN["eligible_transcripts"]] = n_elig; w[sn + SN["segments"]] = n_seg
    return w


def views(words):
    w = np.asarray(words)
    return dict(words=w, BA=w[0:5], RC=w[5:10], ST=w[10:14], BC=w[14:314].reshape(3, 100), SN=w[314:330])


def text_of(words) -> bytes:
    v = {k: [int(x) for x in a.ravel()] for k, a in views(words).items()}
    div = lambda a, d: a // d if d else 0
    five, three, sn = sum(v["BC"][200:210]), sum(v["BC"][290:300]), v["SN"]
    out = ["SN\t%s\t%d" % (SN_NAMES[k], sn[k]) for k in range(8)]
    out += ["SN\tsense_ppm\t%d" % div(v["ST"][0] * 10 ** 6, v["ST"][0] + v["ST"][1]), "SN\tfive_prime_milli\t%d" % div(five, 10 * sn[6]),
            "SN\tthree_prime_milli\t%d" % div(three, 10 * sn[6]), "SN\tfive_to_three_milli\t%d" % div(1000 * five, three)]
    out += ["BA\t%s\t%d\t%d" % (CLASS_NAMES[k], v["BA"][k], div(v["BA"][k] * 10 ** 6, sn[3])) for k in range(5)]
    out += ["RC\t%s\t%d" % (CLASS_NAMES[k], v["RC"][k]) for k in range(5)]
    out += ["ST\t%s\t%d" % (ST_NAMES[k], v["ST"][k]) for k in range(4)]
    out += ["BC\t%d\t%d\t%d\t%d" % (b, v["BC"][b], v["BC"][100 + b], v["BC"][200 + b]) for b in range(100)]
    return ("\n".join(out) + "\n").encode()


# ---- hand-made annotation and records (two chromosomes; nothing lies on the second) ----
def crafted_annotation():
    return [
        tx(0, 0, [(300, 350), (100, 150), (150, 180), (170, 200)], cds=(120, 320)),      # 0: exons unsorted, touching, overlapping -> (100, 200), (300, 350); L 150; the CDS covers part of each
        tx(0, 1, [(220, 260)]),                                                          # 1: minus, nested in 0's intron, no CDS: UTR over intron, strands 3; L 40
        tx(0, 0, [(130, 140)], flags=RIBOSOMAL),                                         # 2: rRNA over 0's coding bases
        tx(0, 1, [(1200, 1230), (1000, 1040), (1100, 1130)], cds=(1010, 1220)),          # 3: minus, L 100: every base a sample, right to left
        tx(0, 0, [(1500, 1599)], cds=(1500, 1599)),                                      # 4: L 99, not eligible
        tx(0, 0, [(1700, 1801)], cds=(1650, 1900)),                                      # 5: L 101; a CDS that reaches beyond the span
        tx(0, 0, [(1900, 2000)]),                                                        # 6: L 100, no CDS
        tx(0, 0, [(2200, 2250), (2400, 2450)], cds=(2200, 2450)),                        # 7: L 100; its intron holds
        tx(0, 1, [(2300, 2350)], cds=(2310, 2340)),                                      # 8: another transcript's exon
        tx(0, 1, [(2500, 2600)], cds=(2500, 2600)),                                      # 9: L 100, never covered: S = 0
        tx(0, 1, [(2650, 2700)]),                                                        # 10: the last span's end
    ]


def crafted_cases():
    """name -> records (any order)"""
    rec = lambda tid, pos, flag, name, cigar, mapq=30: record(tid, pos, flag, name, cigar, l_seq=sum(l for l, op in cigar if op in (M, I, S, EQ, X)), mapq=mapq)
    edges = [rec(0, 90, 0, b"ends_%d" % (90 + l), [(l, M)]) for l in (9, 10, 11)] + [rec(0, 180, 0, b"ends_%d" % (180 + l), [(l, M)]) for l in (19, 20, 21)]
    edges += [rec(0, p, 0, b"starts_%d" % p, [(10, M)]) for p in (99, 100, 101, 199, 200, 201, 119, 120, 121, 129, 130, 139, 140)]
    edges += [rec(0, 90, 0, b"many_segments", [(270, M)]), rec(0, 10, 0, b"in_front_of_the_first", [(20, M)]), rec(0, 2900, 0, b"behind_the_last", [(50, M)]),
              rec(1, 100, 0, b"no_transcript_here", [(50, M)]), rec(0, 2690, 16, b"over_the_last_end", [(20, M)])]
    flags = (0, 16, 0x41, 0x51, 0x81, 0x91)
    strands = [rec(0, p, f, b"s%d_%x" % (p, f), [(10, M)]) for p in (105, 225, 1005, 1050, 1300, 2320) for f in flags]
    depth = [rec(0, 1920, 0, b"in_in_out", [(30, M)])] + [rec(0, 1900, 16 if k & 1 else 0, b"pile%d" % k, [(50, M)]) for k in range(12)]
    depth += [rec(0, 1000, 0, b"minus_5p_end", [(5, M), (3, I), (5, M), (2, S)]), rec(0, 1030, 0, b"across_introns", [(10, M), (60, N), (30, EQ), (70, D), (1, X), (4, M)]),
              rec(0, 1700, 0, b"first_base_only", [(1, M)]), rec(0, 1800, 0, b"last_base_only", [(1, M)]), rec(0, 1750, 0, b"zero_length_op", [(0, M), (5, M)])]
    spliced = [rec(0, 2230, 0x63, b"n_over_an_exon", [(20, M), (150, N), (20, M)]), rec(0, 2330, 0x93, b"n_over_an_exon", [(20, M), (50, N), (10, M)])]
    filters = [rec(0, 1910, 0x100, b"secondary", [(10, M)]), rec(0, 1910, 0x200, b"qcfail", [(10, M)]), rec(0, 1910, 0x400, b"duplicate", [(10, M)]),
               rec(0, 1910, 0x800, b"supplementary", [(10, M)]), rec(0, 1910, 4, b"placed_unmapped", [(10, M)]), rec(0, 1910, 0, b"mapq10", [(10, M)], mapq=10),
               rec(0, 1910, 0, b"mapq9", [(10, M)], mapq=9), record(0, 1910, 0, b"no_cigar", l_seq=10), rec(0, -1, 0, b"pos_m1", [(10, M)]), record(-1, -1, 4, b"unplaced", l_seq=10)]
    return dict(edges=edges, strands=strands, depth=depth, spliced=spliced, filters=filters)


TO_THE_EDGE = cvi.TO_THE_EDGE


def range_cases():
    """-> (records that end exactly at 2^32 - 1, records of which the second is out of range)"""
    rec = lambda tid, pos, flag, name, cigar: record(tid, pos, flag, name, cigar, l_seq=sum(l for l, op in cigar if op in (M, I, S, EQ, X)), mapq=30)
    ok = [rec(0, 0, 0, b"pos0", [(5, M)]), rec(1, (1 << 31) - 1, 0, b"ends_at_2_32_m1", TO_THE_EDGE + [(8, M)])]
    bad = [rec(0, 0, 0, b"pos0", [(5, M)]), rec(0, 7, 0x400, b"a_duplicate_out_of_range", TO_THE_EDGE[:1] * 17 + [(8, M)]), rec(1, (1 << 31) - 1, 0, b"ends_at_2_32", TO_THE_EDGE + [(9, M)])]
    return ok, bad


def bad_annotations(n_chr=2):
    """(the rule, transcripts, the exon array's length or None) of annotations that each break one rule in transcript 1"""
    good = tx(0, 0, [(10, 20)])
    cases = [("chromosome", [good, tx(n_chr, 0, [(10, 20)])]), ("chromosome", [good, tx(-1, 0, [(10, 20)])]), ("strand", [good, tx(0, 2, [(10, 20)])]),
             ("flags", [good, tx(0, 0, [(10, 20)], flags=2)]), ("no exon", [good, tx(0, 0, [])]), ("start < end", [good, tx(0, 0, [(10, 20), (30, 30)])]),
             ("start < end", [good, tx(0, 0, [(20, 10)])]), ("cds_start <= cds_end", [good, tx(0, 0, [(10, 20)], cds=(15, 12))])]
    return cases


def random_annotation(rng, n_chr, n_tx, span=2500):
    out = []
    for _ in range(n_tx):
        p = rng.randrange(0, span)
        ex = []
        for _ in range(rng.randrange(1, 6)):
            ln = rng.choice([1, 20, 50, 100, 130]); ex.append((p, p + ln)); p += ln + rng.choice([-10, 0, 0, 40, 200])
            p = max(p, 0)
        lo, hi = min(s for s, e in ex), max(e for s, e in ex)
        cds = rng.choice([(0, 0), (lo, hi), (lo + (hi - lo) // 3, hi - (hi - lo) // 3)])
        rng.shuffle(ex)
        out.append(tx(rng.randrange(n_chr), rng.randrange(2), ex, cds, RIBOSOMAL if rng.random() < 0.1 else 0))
    return out


# ---- the native program ----
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "rnametrics_checks_san" if sanitize else "rnametrics_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "rnametrics_checks.hip")])
    return exe


def run_program(exe, workdir, tag, n_chr, raw, annot, exclude=DEFAULT_EXCLUDE, min_mapq=0, min_cov=DEFAULT_MIN_COV, n_exons=None):
    """-> dict(rc = the exit status (0; 3: the annotation was refused), err = the refusal's text, words, text, segs = [(chr, start, class, strands)], elig, bad)"""
    src = os.path.join(workdir, "rm_%s.in" % tag); txt = os.path.join(workdir, "rm_%s.txt" % tag); out = os.path.join(workdir, "rm_%s.metrics" % tag)
    t, ex = pack(annot)
    with open(src, "wb") as f:
        f.write(struct.pack("<8q", n_chr, exclude, min_mapq, min_cov, len(raw), len(t), len(ex), len(ex) if n_exons is None else n_exons))
        f.write(t.tobytes() + ex.tobytes() + raw)
    r = subprocess.run([exe, src, txt, out], capture_output=True, text=True)
    assert r.returncode in (0, 3), r.stdout + r.stderr
    res = dict(rc=r.returncode, err=r.stderr, words=None, segs=[], elig=None, bad=None, recs=[], text=open(out, "rb").read() if os.path.exists(out) and r.returncode == 0 else b"")
    if r.returncode:
        return res
    for line in open(txt).read().splitlines():
        w = line.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "seg":
            res["segs"].append(tuple(v))
        elif w[0] == "elig":
            res["elig"] = v[0]
        elif w[0] == "bad":
            res["bad"] = v[0]
        elif w[0] == "rec":
            res["recs"].append(tuple(v))
        elif w[0] == "words":
            res["words"] = np.array(v, np.uint64)
    return res


# ---- the mapper's own records: a golden case's genome with a seeded random annotation ----
CASE_SEEDS = {"pe101_spliced": 3}       # chosen on the golden SAM of the case (the reference's records at -mis 5): rich_enough holds
CASE_MIN_COV = 10                       # 3000 reads of 101 over 500 kb: a depth of 0.6, so S is about 60 for a well-covered transcript


def case_annotation(case, seed):
    """the gene-count tests' random annotation over the case's genome, a gene as one transcript; a quarter without CDS, the rest with a CDS that leaves a fifth
    of the span at either end, one in twelve ribosomal"""
    import random
    import genecount_inputs as gci
    n_genes, exons = gci.case_annotation(case, seed)
    rng = random.Random(seed + 1000)
    out = []
    for g in range(n_genes):
        mine = [e for e in exons if e[4] == g]
        if not mine:
            continue
        lo, hi = min(e[1] for e in mine), max(e[2] for e in mine)
        cds = (0, 0) if rng.random() < 0.25 else (lo + (hi - lo) // 5, hi - (hi - lo) // 5)
        out.append(tx(mine[0][0], mine[0][3], [(e[1], e[2]) for e in mine], cds, RIBOSOMAL if rng.random() < 1 / 12 else 0))
    return out


def records_of_sam(sam_text: str, names):
    """the fields of a SAM text's lines the metrics read, as BAM records without bases: refID, pos, flag, MAPQ and the CIGAR"""
    import re
    ops = "MIDNSHP=X"
    tid = {(n.decode() if isinstance(n, bytes) else n): k for k, n in enumerate(names)}
    out = []
    for line in sam_text.split("\n"):
        if not line or line[0] == "@":
            continue
        f = line.split("\t")
        cigar = [] if f[5] == "*" else [(int(l), ops.index(o)) for l, o in re.findall(r"(\d+)([MIDNSHP=X])", f[5])]
        out.append(record(tid.get(f[2], -1), int(f[3]) - 1, int(f[1]), f[0].encode()[:200], cigar, l_seq=0, mapq=int(f[4])))
    return out


def rich_enough(words, sums, annot, n_chr, min_cov=CASE_MIN_COV):
    """every class of BA, all four ST rows, and at least ten contributing transcripts on each strand"""
    v = views(words)
    elig = flatten(annot, n_chr)[1]
    per_strand = [sum(1 for t, s in zip(elig, sums) if t[1] == k and s >= max(min_cov, 1)) for k in (0, 1)]
    return bool(v["BA"].all() and v["ST"].all() and min(per_strand) >= 10)


def write_gtf(path, annot, chr_names):
    """the transcripts as a GTF file: an exon line per exon in the given order, a CDS line for a transcript with one, gene_biotype "rRNA" on the flagged ones"""
    with open(path, "w") as f:
        f.write("# a test annotation\n")
        for k, a in enumerate(annot):
            name = chr_names[a["chr"]].decode() if isinstance(chr_names[a["chr"]], bytes) else chr_names[a["chr"]]
            attrs = 'gene_id "G%05d"; transcript_id "T%05d.1";%s' % (k, k, ' gene_biotype "rRNA";' if a["flags"] & RIBOSOMAL else ' gene_biotype "protein_coding";')
            line = lambda feature, s, e: f.write("%s\ttest\t%s\t%d\t%d\t.\t%s\t.\t%s\n" % (name, feature, s + 1, e, "-" if a["strand"] else "+", attrs))
            line("transcript", min(s for s, e in a["exons"]), max(e for s, e in a["exons"]))
            for s, e in a["exons"]:
                line("exon", s, e)
            if a["cds"][0] < a["cds"][1]:
                line("CDS", a["cds"][0], a["cds"][1])
