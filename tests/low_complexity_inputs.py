"""Inputs of the low-complexity parity tests (CPU: tests/test_low_complexity_oracle.py, GPU: tests/test_gpu_low_complexity.py, fixtures:
tests/golden/make_low_complexity.py): genomes of at most 64 kb made of what real DNA has and random text has not -- homopolymers,
microsatellites, a text that equals its own reverse complement, contigs present several times -- with copy counts on both sides of the small
numbers the repeat paths turn on (max_dup 100 / 1000, the floor of 128 rows of k_seed_heavy_walk, 16 seeds per unit, the sorter's 4096-pair
tile), and about 500 reads per genome that lie in, beside and across the runs.  Everything is a pure function of the genome's name."""
from __future__ import annotations

import hashlib
import os
import numpy as np
from dart_amd import synth, host

NAMES = ["homopolymer", "homopolymer_long", "dinuc", "self_rc", "palindrome", "twins", "ladder", "micro"]
READ_LENGTHS = (36, 101, 250)
RUNG_WINDOWS = (18, 20, 22, 25, 30, 36, 45, 60, 75, 90, 101, 250)          # lengths of the windows inside a rung, beside its 17-mer and the whole rung
MAX_SINGLE, MAX_PAIRS = 380, 100                    # reads per genome: at most 380 single ones and 100 pairs (+ 2 odd pairs)
SE_FLAGS = ([], ["-mis", "5"], ["-mis", "5", "-m", "-max_dup", "1000"])
PE_FLAGS = (["-mis", "5"], ["-all_sj"])
MULTI_RUN = "se: -mis 5 -m -max_dup 1000"
INDEX_EXT = ("amb", "ann", "bwt", "pac", "sa")
MICRO_UNITS = (b"A", b"T", b"AC", b"AT", b"CAG", b"GATA", b"AAAAT", b"TTAGGG")
# the ladder's rungs: (unit, copies of the unit-phase-0 17-mer in the text of both strands); a run of R = (copies - 1) * len(unit) + 17 bases.
# 99 / 100 / 101 and 999 / 1000 / 1001: an interval of max_dup rows is kept, one of max_dup + 1 is not (default and -max_dup 1000);
# 127 / 128 / 129: the floor of k_seed_heavy_walk; G x 116 and ATC x 149 bases: a 101-base read inside has 16 / 17 places, so 16 / 17 seeds.
# Every rung has a unit of its own (no rotation or reverse complement of another's), so its 17-mer lies in no other rung.
PROBE_K = 17
LADDER = ((b"A", 99), (b"AC", 100), (b"AG", 101), (b"AAC", 127), (b"AAG", 128), (b"AAT", 129), (b"ACC", 999), (b"ACG", 1000), (b"ACT", 1001),
          (b"G", 100), (b"ATC", 45))

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_CODE = np.zeros(256, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
_COMP = np.full(256, ord("N"), np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    _COMP[_a] = _b


def _seed(name: str, salt: int) -> int:
    return 77000 + 10 * NAMES.index(name) + salt


def revcomp(s: bytes) -> bytes:
    return _COMP[np.frombuffer(s, np.uint8)[::-1]].tobytes()


def tile(unit: bytes, n: int, phase: int = 0) -> bytes:
    """n bases of the unit repeated, starting at base `phase` of it"""
    return (unit * ((n + phase) // len(unit) + 2))[phase:phase + n]


def count_occurrences(text: bytes, pat: bytes) -> int:
    """overlapping occurrences of pat in text"""
    k, p = 0, text.find(pat)
    while p >= 0:
        k += 1
        p = text.find(pat, p + 1)
    return k


def _plant_run(codes, p: int, unit: bytes, R: int, lo: int, hi: int):
    """the run at [p, p + R); the bases next to it (inside [lo, hi)) are made to break the period, so the run is exactly R long"""
    u = len(unit)
    codes[p:p + R] = _CODE[np.frombuffer(tile(unit, R), np.uint8)]
    if p - 1 >= lo:
        codes[p - 1] = (int(_CODE[unit[(-1) % u]]) + 1) & 3
    if p + R < hi:
        codes[p + R] = (int(_CODE[unit[R % u]]) + 1) & 3


_genomes = {}


def make_genome(name: str) -> synth.Genome:
    """-> the genome; g.runs = [(start, length, unit)] in forward coordinates of the concatenated contigs, g.long_gaps = exon chains as lists of
    (start, length) (micro only), g.rungs = indices into g.runs of the ladder's rungs in LADDER's order (ladder only)"""
    if name in _genomes:
        return _genomes[name]
    rng = np.random.default_rng(_seed(name, 0))
    rnd = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    enc = lambda s: _CODE[np.frombuffer(s, np.uint8)]
    runs, chains, introns, rungs = [], [], [], []
    if name == "homopolymer":
        lens = [500, 600]                                # the run ends the forward strand: A..AT is in the text once, where the strands meet, and a
        codes = np.concatenate([rnd(500), enc(b"A" * 600)])      # read of the run with a T in it is given a place there, past the contig's last base
        codes[499] = codes[499] or 1
        runs = [(500, 600, b"A")]
    elif name == "homopolymer_long":
        lens = [4200]                                    # N = 8401 rows: the AA and the TT bucket hold 4199 suffixes each, more than one 4096-pair tile
        codes = enc(b"A" * 4200)
        runs = [(0, 4200, b"A")]
    elif name == "dinuc":
        lens = [1200, 1500, 1000]
        codes = np.concatenate([enc(tile(b"AC", 1200)), enc(tile(b"CAG", 1500)), rnd(1000)])
        runs = [(0, 1200, b"AC"), (1200, 1500, b"CAG")]
    elif name == "self_rc":
        lens = [900, 600]                                # (AT)450 is its own reverse complement
        codes = np.concatenate([enc(tile(b"AT", 900)), rnd(600)])
        runs = [(0, 900, b"AT")]
    elif name == "palindrome":
        h = rnd(1500)
        lens = [3000]
        codes = np.concatenate([h, (3 - h)[::-1]])
    elif name == "twins":
        t = rnd(3000)
        lens = [3000, 3000, 3000]
        codes = np.concatenate([t, t, (3 - t)[::-1]])
    elif name == "ladder":
        lens = [30000]
        codes = rnd(30000)
        R = [(c - 1) * len(u) + PROBE_K for u, c in LADDER]
        gap = (30000 - sum(R)) // (len(R) + 1)
        p = gap
        for (u, c), r in zip(LADDER, R):
            _plant_run(codes, p, u, r, 0, 30000)
            rungs.append(len(runs)); runs.append((p, r, u))
            p += r + gap
    elif name == "micro":
        lens = [30000, 30000]
        codes = rnd(60000)
        for co in (0, 30000):
            p = co + int(rng.integers(100, 400))
            while True:
                u = MICRO_UNITS[int(rng.integers(0, len(MICRO_UNITS)))]
                r = int(np.exp(rng.uniform(np.log(24), np.log(400))))
                if p + r + 100 > co + 30000:
                    break
                _plant_run(codes, p, u, r, co, co + 30000)
                runs.append((p, r, u))
                p += r + int(rng.integers(300, 1500))
        # exon chains from 4 kb on: 60-base exons around a skip of 300 .. 3000 bases whose two ends lie in the middle of 24-base runs of one unit, in
        # phase, so that the read is periodic over its junction and the boundary can be put at any base of the run; every third chain has a 24-base
        # middle exon; half of the skips get GT..AG (or CT..AC) written over their ends afterwards (which cuts the tie short on that side)
        # A chain is placed where what it writes touches no planted run and no earlier chain, and where its exons hold nothing an earlier chain wrote
        hit = lambda spans, others: any(x < b and a < y for a, b in spans for x, y in others)
        kept = [(a - 2, a + r + 2) for a, r, _ in runs]  # what later chains must not write over: the runs and their flanks, earlier chains
        wrote = []                                       # what earlier chains wrote
        for j in range(40):
            exons = [60, 24, 60] if j % 3 == 2 else [60, 60]
            while True:
                skips = [int(rng.integers(300, 3000)) for _ in exons[1:]]
                co = 30000 * int(rng.integers(0, 2))
                p = co + int(rng.integers(4000, 30000 - sum(exons) - sum(skips) - 100))
                chain, bounds = [(p, exons[0])], []
                p += exons[0]
                for e, sk in enumerate(skips):
                    bounds.append((p, p + sk))           # the exon ends at d, the next one starts at a
                    chain.append((p + sk, exons[e + 1]))
                    p += sk + exons[e + 1]
                wins = [(x - 12, x + 12) for da in bounds for x in da]
                ex = [(a, a + l) for a, l in chain]
                if not hit(wins, kept) and not hit(ex, wrote):
                    break
            kept += wins + ex; wrote += wins
            for d, a in bounds:
                u = MICRO_UNITS[int(rng.integers(0, len(MICRO_UNITS)))]
                codes[d - 12:d + 12] = enc(tile(u, 24))
                codes[a - 12:a + 12] = enc(tile(u, 24))
                motif = int(rng.random() < 0.5)
                if motif:
                    if rng.random() < 0.5:
                        codes[d:d + 2] = (2, 3); codes[a - 2:a] = (0, 2)
                    else:
                        codes[d:d + 2] = (1, 3); codes[a - 2:a] = (0, 1)
                introns.append((d, a - d, motif))
            chains.append(chain)
    else:
        raise KeyError(name)
    g = synth.Genome(["s%d" % (i + 1) for i in range(len(lens))], lens, np.ascontiguousarray(codes, np.uint8), np.asarray(introns, np.int64).reshape(-1, 3))
    g.runs, g.long_gaps, g.rungs = runs, chains, rungs
    _genomes[name] = g
    return g


def codes_sha256(name: str) -> str:
    return hashlib.sha256(make_genome(name).codes.tobytes()).hexdigest()


def both_strands(name: str) -> bytes:
    """the text the index is built on: the contigs, then their reverse complement"""
    f = make_genome(name).ascii().tobytes()
    return f + revcomp(f)


def rung_copies(name: str = "ladder"):
    """per rung: occurrences of its 17-mer (the unit from phase 0) in the text of both strands"""
    text = both_strands(name)
    return [count_occurrences(text, tile(u, PROBE_K)) for u, _ in LADDER]


def _sub(s: bytes, q: int, k: int) -> bytes:
    """base q replaced by the k-th other one"""
    b = bytearray(s)
    b[q] = b"ACGT"[(b"ACGT".index(b[q]) + k) & 3]
    return bytes(b)


def _contig_of(g, p: int):
    ci = int(np.searchsorted(np.cumsum(g.lengths), p, side="right"))
    return int(g.offsets[ci]), int(g.offsets[ci] + g.lengths[ci])


def _unique_spans(g):
    """(start, end) of the stretches outside every run, per contig, at least 60 bases long"""
    out = []
    for co, cl in zip(g.offsets.tolist(), g.lengths.tolist()):
        p = co
        for a, r, _ in sorted(g.runs):
            if co <= a < co + cl:
                if a - p >= 60: out.append((p, a))
                p = a + r
        if co + cl - p >= 60: out.append((p, co + cl))
    return out


def _thin(items, budget: int, keep):
    """at most `budget` of the items, in order: all that `keep` names and an even stride of the others"""
    must = [i for i, x in enumerate(items) if keep(x)]
    rest = [i for i, x in enumerate(items) if not keep(x)]
    room = max(0, budget - len(must))
    if len(rest) > room:
        rest = [rest[(k * len(rest)) // room] for k in range(room)]
    return [items[i] for i in sorted(must + rest)]


_single = {}


def tagged_single_reads(name: str):
    """-> list of (kind, run index or -1, bytes): the reads before the strand flip of every second one (see single_reads)"""
    if name in _single:
        return _single[name]
    g = make_genome(name)
    rng = np.random.default_rng(_seed(name, 1))
    text = g.ascii().tobytes()
    total = g.total
    out = []
    uniq = _unique_spans(g)
    per_run = max(1, 24 // max(1, len(g.runs)))          # rounds over the runs, so that every genome gets a few hundred reads
    for ri, (a, R, u) in enumerate(g.runs):
        co, ce = _contig_of(g, a)
        is_rung = ri in g.rungs
        for rep in range(2 if is_rung else per_run):
            for L in READ_LENGTHS:
                if R >= L:                               # wholly inside the run; then one with a substitution in its middle
                    p = a + int(rng.integers(0, R - L + 1))
                    if not is_rung:                      # (a rung's own windows follow below)
                        out.append(("inside", ri, text[p:p + L]))
                        out.append(("inside", ri, text[a + R - L:a + R]))
                    # (on the long homopolymer never the other strand's letter: A..AT is in the text once, where the strands meet, and would map there)
                    out.append(("inside_sub", ri, _sub(text[p:p + L], L // 2, 1 + rep % (2 if name == "homopolymer_long" else 3))))
                out.append(("pure_unit", ri, tile(u, L, int(rng.integers(0, len(u))))))
                k = int(rng.integers(18, L - 15))       # k bases of unique text, then the run: anchored on the left / on the right
                if a - k >= co and R >= L - k:
                    out.append(("anchor_left", ri, text[a - k:a - k + L]))
                    s = text[a - k:a - k + L + len(u)]   # one unit deleted from / inserted into the run part: its place is anyone's guess
                    out.append(("unit_del", ri, s[:k + 8] + s[k + 8 + len(u):]))
                    out.append(("unit_ins", ri, (s[:k + 8] + u + s[k + 8:])[:L]))
                if a + R + k <= ce and R >= L - k:
                    out.append(("anchor_right", ri, text[a + R + k - L:a + R + k]))
                if R + 40 <= L and a - 20 >= co and a + R + 20 <= ce:      # unique text on both sides of the whole run
                    lo = max(co, min(a - 20, a + R + 20 - L)); lo = max(co, min(lo, ce - L))
                    s = text[lo:lo + L]
                    out.append(("anchor_both", ri, s))
                    q = a - lo + (R // 2 // len(u)) * len(u)
                    out.append(("unit_del", ri, s[:q] + s[q + len(u):]))
                    out.append(("unit_ins", ri, s[:q] + u + s[q:]))
        if is_rung:                                      # unmodified windows of the rung, no two alike: in a homopolymer that takes a length each
            for L in RUNG_WINDOWS + ((R,) if R <= 1000 else ()):                 # (the library takes reads of up to 1000 bases)
                if L <= R:
                    p = a + R - L if L == 36 else a + int(rng.integers(0, R - L + 1))       # (the 36-base one ends with the run)
                    out.append(("inside", ri, text[p:p + L]))
        if is_rung or name in ("homopolymer", "homopolymer_long", "dinuc", "self_rc"):
            for rep in range(6):                         # the unit from phase 0, 17 bases: its interval is the run's copy count
                out.append(("pure17", ri, tile(u, PROBE_K)))
            # the same 17 bases, a base that neither the run nor its flank continues with, and the next 17 bases of the run: two seeds, the first with
            # the run's copy count as its interval and the second with that or one less.  Identical seeds of one place in the read alone give no
            # alignment (all of the pure reads above stay unmapped), so the read maps exactly where max_dup admits the copy count
            nxt = b"ACGT"[(b"ACGT".index(u[PROBE_K % len(u)]) + 2) & 3:][:1]
            for rep in range(6):
                out.append(("probe", ri, tile(u, PROBE_K) + nxt + tile(u, PROBE_K, (PROBE_K + 1) % len(u))))
    n_u = 60 if g.runs else 120
    for k in range(n_u):                                 # unique text: exact, one substitution, a poly-A tail the genome does not hold
        lo, hi = uniq[int(rng.integers(0, len(uniq)))] if uniq else (0, 0)
        if hi - lo < 40: continue
        L = min(READ_LENGTHS[k % 3], hi - lo)
        p = int(rng.integers(lo, hi - L + 1))
        s = text[p:p + L]
        kind = ("exact", "sub", "tail30")[k % 3]
        if kind == "sub": s = _sub(s, int(rng.integers(0, L)), int(rng.integers(1, 4)))
        if kind == "tail30": s = s[:L - 30] + b"A" * 30 if L >= 66 else s + b"A" * 30
        out.append((kind, -1, s))
    if name == "homopolymer_long":                       # no unique text at all: runs with two substitutions, random reads
        for k in range(60):
            L = READ_LENGTHS[k % 3]
            out.append(("inside_sub", 0, _sub(_sub(b"A" * L, L // 3, 1 + k % 2), 2 * L // 3, 1 + (k // 3) % 2)))
            out.append(("random", -1, _ACGT[rng.integers(0, 4, L)].tobytes()))
    if name in ("palindrome", "twins"):                  # windows over the centre of the palindrome / over the contig seams
        for b in (np.cumsum(g.lengths)[:-1].tolist() or [total // 2]):
            for L in READ_LENGTHS:
                for sh in (0, 3, L // 3):
                    out.append(("seam", -1, text[b - L // 2 + sh:b - L // 2 + sh + L]))
    for chain in g.long_gaps:
        s = b"".join(text[a:a + l] for a, l in chain)
        out.append(("spliced", -1, s))
        out.append(("spliced", -1, _sub(s, 5, 1)))
    out.append(("all_n", -1, b"N" * 50)); out.append(("all_n", -1, b"N" * 50))
    out.append(("short", -1, text[total // 2:total // 2 + 12])); out.append(("short", -1, text[total // 2:total // 2 + 12]))
    out = _thin(out, MAX_SINGLE, lambda r: r[0] in ("probe", "spliced", "all_n", "short") or (r[0] in ("inside", "inside_sub") and r[1] in g.rungs))
    _single[name] = out
    return out


def single_reads(name: str):
    """-> list of bytes: every second read comes from the reverse strand"""
    return [revcomp(s) if i % 2 else s for i, (_, _, s) in enumerate(tagged_single_reads(name))]


_paired = {}


def paired_reads(name: str):
    """-> (mate 1 list, mate 2 list) as sequenced (mate 2 not yet reverse-complemented): one mate unique and one in a run, both in runs, both
    unique, fragments over contig seams (on twins: mates on two copies), mate 1 over the micro introns"""
    if name in _paired:
        return _paired[name]
    g = make_genome(name)
    rng = np.random.default_rng(_seed(name, 2))
    text = g.ascii().tobytes()
    frags = []                                           # (mate 1 source, mate 2 source), both in the fragment's direction

    def pair(s, flen, L):
        return text[s:s + L], text[s + flen - L:s + flen]

    for ri, (a, R, u) in enumerate(g.runs):
        co, ce = _contig_of(g, a)
        for rep in range(max(1, 12 // len(g.runs))):
            for L in READ_LENGTHS:
                if R >= L + 5:                           # both mates inside the run
                    flen = int(rng.integers(L + 5, min(R, L + 300) + 1))
                    frags.append(pair(a + int(rng.integers(0, R - flen + 1)), flen, L))
                if a - L - 30 >= co and R >= L:          # mate 1 in unique text before the run, mate 2 inside it
                    s = a - L - int(rng.integers(5, 30))
                    frags.append(pair(s, min(a + R, s + 2 * L + int(rng.integers(40, 200))) - s, L))
                if a + R + L + 30 <= ce and R >= L:      # mate 1 inside the run, mate 2 behind it
                    e = a + R + L + int(rng.integers(5, 30))
                    s = max(a, e - 2 * L - int(rng.integers(40, 200)))
                    frags.append(pair(s, e - s, L))
    uniq = _unique_spans(g)
    for k in range(40 if g.runs else 90):                # both mates unique; every third pair with a substitution in each mate
        lo, hi = uniq[int(rng.integers(0, len(uniq)))] if uniq else (0, 0)
        L = READ_LENGTHS[k % 3]
        if hi - lo < L + 5: continue
        flen = int(rng.integers(L + 5, min(hi - lo, L + 300) + 1))
        a_, b_ = pair(int(rng.integers(lo, hi - flen + 1)), flen, L)
        if k % 3 == 0: a_, b_ = _sub(a_, int(rng.integers(0, L)), 1), _sub(b_, int(rng.integers(0, L)), 2)
        frags.append((a_, b_))
    for b in np.cumsum(g.lengths)[:-1].tolist():         # fragments over every contig seam: on twins, mates on two copies of one contig
        for L in (36, 101):
            for gap in (0, 40, 150):
                frags.append((text[b - L - gap:b - gap], text[b + gap:b + gap + L]))
    n_plain = len(frags)
    cend = {int(o): int(o + l) for o, l in zip(g.offsets, g.lengths)}
    for chain in g.long_gaps:                            # mate 1 over the skips, mate 2 behind the last exon
        a, l = chain[-1]
        ce = max(e for o, e in cend.items() if o <= a)
        if a + l + 20 + 60 <= ce:
            frags.append((b"".join(text[x:x + y] for x, y in chain), text[a + l + 20:a + l + 80]))
    frags = _thin([(k >= n_plain, f) for k, f in enumerate(frags)], MAX_PAIRS, lambda x: x[0])
    frags = [f for _, f in frags]
    frags.append((b"N" * 36, text[:36]))
    frags.append((text[:36], text[40:52]))               # a mate shorter than a seed
    m1, m2 = [], []
    for i, (a, b) in enumerate(frags):                   # every second fragment comes from the reverse strand
        if i % 2:
            m1.append(revcomp(b)); m2.append(a)
        else:
            m1.append(a); m2.append(revcomp(b))
    _paired[name] = (m1, m2)
    return m1, m2


def stored_pairs(m1, m2):
    """the batch as the loader stores it: mate 1, then mate 2 reverse-complemented, alternating"""
    out = []
    for a, b in zip(m1, m2):
        out.append(a); out.append(revcomp(b))
    return out


def write_fastq(path: str, seqs, mate: int | None = None) -> None:
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b"@r%d%s\n" % (i, b"" if mate is None else b"/%d" % mate) + s + b"\n+\n" + b"I" * len(s) + b"\n")


def reads_sha256(seqs) -> str:
    return hashlib.sha256(b"\n".join(seqs)).hexdigest()


def runs(name: str):
    """[(run label, paired, flags of the mapping)]: the label is the key of tests/golden/low_complexity.json"""
    return ([("%s se: %s" % (name, " ".join(f)), False, list(f)) for f in SE_FLAGS] +
            [("%s pe: %s" % (name, " ".join(f)), True, list(f)) for f in PE_FLAGS])


def write_inputs(name: str, d: str):
    """d/g.fa, d/a.fq (single-end), d/p1.fq + d/p2.fq (pairs) -> the file arguments of the single-end and of the paired run"""
    os.makedirs(d, exist_ok=True)
    make_genome(name).write_fasta(os.path.join(d, "g.fa"))
    write_fastq(os.path.join(d, "a.fq"), single_reads(name))
    pe = paired_reads(name)
    write_fastq(os.path.join(d, "p1.fq"), pe[0], 1); write_fastq(os.path.join(d, "p2.fq"), pe[1], 2)
    return ["-f", "a.fq"], ["-f", "p1.fq", "-f2", "p2.fq"]


def batch(name: str, paired: bool):
    """(seq_off, rlen, flat) of a run's reads, as host.pack_reads gives them"""
    return host.pack_reads(stored_pairs(*paired_reads(name)) if paired else single_reads(name))
