"""Inputs of the threshold parity tests (CPU: tests/test_thresholds_oracle.py, GPU: tests/test_gpu_thresholds.py, fixture:
tests/golden/make_thresholds.py): one genome of 2.25 Mb and ladders of reads, each of which walks ONE integer of the mapping path over one of the
reference's comparisons, from 2 below to 2 above, no value skipped.  A rung is a pair: the event read, which carries the integer, and a plain mate
(101 exact bases 200 bases beside it).  Every ladder stands at 8 sites: both strands, the event read as mate 1 and as mate 2, reads of 101, 150 and
250 bases where the construction leaves the length free, and at site 7 the event at a multiple of 128 text bases (the width of an Occ block and of
the packed text's rows).  Every piece of text a read is cut from holds only 16-mers that occur once in both strands (count16; the planted copies of
G and K: exactly as often as planted).  Everything is a pure function of this file.

The ladders, the comparison each one walks (reference file:line), and where the reference's object code puts the flip (tests/golden/thresholds.json):

  A_clean_t{5,10,31}   a gap of L text bases between two abutting exact seeds against -min_intron t: an N op `< MinIntronSize`   AlignmentCandidates.cpp:1057   flips t-1 | t
  A_sub_t{5,10,31}     the same with a substitution 3 bases before the gap, so gap filling decides: `PosDiff > MinIntronSize`    AlignmentCandidates.cpp:585,770   flips t | t+1
  B_read_t{100000,500000}  the gap L inside one read against -max_intron: `PosDiff < MaxIntronSize`                                AlignmentCandidates.cpp:265      flips t-1 | t
  B_mates_t{..}        the gap between the footprints of two plain mates: a control that must NOT flip (max_intron is not the pair's limit)
  B_chrend             the read's second part starts d bases from its chromosome's last base: the ChrLocMap clause of :265          flips -1 | 0 (forward strand)
  B_chrend_rev         the same reads from the other strand, where the clause looks at the other chromosome's block: compared, not judged
  C_fast_m{0,1,2,5,12} k isolated substitutions in a plain read against -mis m (k_pair writes these reports itself: dg_pair.h)      AlignmentCandidates.cpp:1172     flips m | m+1
  C_report_m{..}       k substitutions in a read with a 3000-base junction (the report path)                                       the same
  D_rgap               g substituted read bases before a 3000-base junction: `rGaps > 20`                                          AlignmentCandidates.cpp:693      flips 20 | 21
  D_jump               25 read bases with 3 substitutions over a deletion of j text bases: `PosDiff > MaxGaps`                      AlignmentCandidates.cpp:693      flips 5 | 6
                       (both judged by the count of second searches of the read gap, n_reseed / reseed_calls: see test_thresholds_oracle)
  E_reach              mate 2 D bases downstream of mate 1: `dist < 2000000`                                                       Mapping.cpp:420-429              flips 1999999 | 2000000
  E_ahead              mate 2 s bases downstream of mate 1, s = -2 .. 2: `PosDiff(mate 2) < PosDiff(mate 1)`                        Mapping.cpp:422                  flips -1 | 0
  F_cov_r{50,100,101,150,250}  c bases of text, the rest noise: `Score > (int)(rlen * 0.3)`                                        AlignmentCandidates.cpp:251,274  flips thr | thr+1
  G_cut, G_cut_single  a second locus that holds the read's first bases; the two candidates' scores v = 18 .. 23 apart: `> 20`       Mapping.cpp:395                  flips 20 | 21
                       (single-end, under -mis 12 -m and under -mis 5: in a pair the mate decides first)
  H_gap_r{10,15,20,25} x substitutions inside a read gap of r bases beside a junction: `max_score < (int)(rGaps * 0.8)`             AlignmentCandidates.cpp:452      flips r-(int)(.8r) | +1
  H_gapmis_r20         the same at -mis 2: `(rGaps - max_score) > MaxMismatch`                                                      AlignmentCandidates.cpp:452      flips 2 | 3
  K_product            mate 1 with na candidates, mate 2 with nb, through planted copies: `num1 * num2 > 1000`                      Mapping.cpp:411                  flips 1000 | 1001
                       (999 = 27 x 37, 1000 = 25 x 40 = 40 x 25, 1001 = 13 x 77 = 77 x 13; 998 and 1002 have no two factors within max_dup's 100)

  I_reseed             a read gap of g = 35 .. 39 bases that holds 15 + 1 + 15 bases of the left seed's diagonal: `rLen >= (int)(rlen * 0.85)`     AlignmentCandidates.cpp:609-611  flips 37 | 38
  B_read_heavy, D_jump_heavy, E_reach_heavy, E_ahead_heavy, F_cov_heavy   B (100 000), D_jump, E and F (100 bases) once more with a mate that lies in the text 17 times: the
                       pair's unit has more than 16 seeds, so the same comparisons are taken by k_chain_heavy's forms (dg_chain.h:217, :239-240, :398)

Ladder I's head / tail half (8 .. 12 bases against the `>= 10` of :670,680) and ladder J (local alignment quality, tools.cpp:199) are dropped: LADDERS_DROPPED says why.
Not built, with the reason: E's "two candidates of mate 2 at equal distance" -- the distance is PosDiff(mate 2) - PosDiff(mate 1) over candidates whose PosDiff all differ
(a candidate's PosDiff is its first seed's diagonal, and two clusters of one read never share one), so no two candidates of a mate lie at one distance.  That is argued from
the code, not shown by a run: the first-wins form of the strict `<` (dg_chain.h:123 and :402) stays unexercised.  The k-mer floor of :609 (thr >= KmerSize) cannot bind:
the second search runs on read gaps above 20 bases, where (int)(rlen * 0.85) is 17 or more.  D's gaps of 21 .. 25 bases hold no chain the second search would keep, so
D's rungs change the count of searches, not the records."""
from __future__ import annotations

import hashlib
import numpy as np
from dart_amd import synth, host

GENOME_LENGTHS = [2200000, 50000]
GENOME_SEED = 31
N_SITES = 8
READ_LENGTHS = (101, 150, 250)
MATE_LEN, MATE_GAP = 101, 200
RUNS = {"d": ["-mis", "5"],
        "i10": ["-mis", "5", "-min_intron", "10", "-max_intron", "100000"],
        "i31": ["-mis", "5", "-min_intron", "31"],
        "m0": [], "m1": ["-mis", "1"], "m2": ["-mis", "2"],
        "m12m": ["-mis", "12", "-m"], "m30": ["-mis", "30"]}
CLI_FLAGS = ["-mis", "5", "-min_intron", "10", "-max_intron", "50000"]      # (the parser lifts -max_intron to 100 000: the run "i10")
DUMP_RUN = ("pe", "i10")                                                   # the run whose stage dump is committed
LADDERS_DROPPED = {
    "I (head / tail)": "IdentifyHeadingSeed / IdentifyTailingSeed (AlignmentCandidates.cpp:665-683), which hold the `>= 10`, are called from nowhere in the reference: a head or tail of "
         "8 .. 12 bases beyond a 3000-base junction is soft-clipped at every length (reads of 101, 150 and 250 bases, both ends, both strands, -mis 5), no rung differs",
    "J": "CheckLocalAlignmentQuality (tools.cpp:166-201) is reached from ProcessHeadSequencePair / ProcessTailSequencePair alone, that is when the first or last pair of a "
         "candidate is not an exact seed; the pairs that gap filling and IdentifyNormalPairs add lie between two seeds, so a read's head or tail is soft-clipped instead: "
         "heads of 12, 15 and 20 bases with 1 .. 8 spread substitutions and with runs of 1 .. 6 came out as 12S / 15S / 20S on every rung"}

_COMP = np.full(256, ord("N"), np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    _COMP[_a] = _b
_CODE = np.zeros(256, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def revcomp(s: bytes) -> bytes:
    return _COMP[np.frombuffer(s, np.uint8)[::-1]].tobytes()


def _sub(s: bytes, q: int) -> bytes:
    """base q replaced by its transition partner (A <-> G, C <-> T)"""
    b = bytearray(s)
    b[q] = b"ACGT"[(b"ACGT".index(b[q]) + 2) & 3]
    return bytes(b)


def _gap_fill(a: bytes, b: bytes, how: int) -> bytes:
    """read bases that differ from the text behind the left seed (a) and from the text before the right seed (b), base by base"""
    out = bytearray()
    for x, y in zip(a, b):
        i, j = b"ACGT".index(x), b"ACGT".index(y)
        if how == 0: c = [c for c in ((i + 2) & 3, (i + 1) & 3, (i + 3) & 3) if c != j][0]
        elif how == 1: c = 3 - i
        else: c = (i + 1) & 3
        out.append(b"ACGT"[c])
    return bytes(out)


def _subs(s: bytes, places) -> bytes:
    for q in places:
        s = _sub(s, q)
    return s


# ---- the genome -------------------------------------------------------------------------------------------------------------------------------
G_ZONE_FROM, G_ZONE_TO = 1000000, 1200000          # G's reads come from FROM + 2000 * i; their partial copies are planted at TO + 2000 * i
G_DS = (19, 20, 21, 22, 23, 24)                    # d: the read's first 101 - d bases lie at a second place; the candidates' scores are 100 and 101 - d, d - 1 = 18 .. 23 apart
_state = {}


def make_genome() -> synth.Genome:
    if "g" not in _state:
        g = synth.make_genome(GENOME_LENGTHS, seed=GENOME_SEED)
        c = g.codes
        e = GENOME_LENGTHS[0]                       # ladder B_chrend reads over the end of chromosome 1: plain random text there (the generator's repeats may lie anywhere)
        c[e - 600:e + 600] = np.random.default_rng(GENOME_SEED + 1).integers(0, 4, 1200, dtype=np.uint8)
        _state["g"] = g                             # ladder G: 101 bases at p in text whose 16-mers occur once (looked up before anything is planted) ...
        _state["text"] = g.ascii().tobytes()
        _plant_heavy(c)
        _state["text"] = g.ascii().tobytes()
        _state.pop("kmers", None); _state.pop("cs", None)
        places, after = {}, 0
        for k in range(N_SITES):
            for j, d in enumerate(G_DS):
                i = k * len(G_DS) + j
                at = _find(max(after, G_ZONE_FROM + 2000 * i + 300), [(-MATE_GAP - MATE_LEN, 101 + MATE_GAP + MATE_LEN)])
                places[k, j] = (at, G_ZONE_TO + 2000 * i + 300)
                after = at + 1000
        assert after < G_ZONE_TO
        for (k, j), (p, q) in places.items():       # ... whose first 101 - d bases are copied to q, followed by a base that differs from the read's next one
            d = G_DS[j]
            c[q:q + 101 - d] = c[p:p + 101 - d]
            c[q + 101 - d] = (int(c[p + 101 - d]) + 1) & 3
        _state["g_places"] = places
        _state["k_fam"] = _plant_K(c)
        _state["text"] = g.ascii().tobytes()
        del _state["kmers"]
        _state.pop("cs", None)
    return _state["g"]


HEAVY_COPIES = 17                                    # a heavy ladder's plain mate (E: its mate 1) lies in the text 17 times: 17 seeds, so the pair's unit has more than the 16
HEAVY_MATE = ("B_read_heavy", "D_jump_heavy", "F_cov_heavy")      # seeds of k_pair's lane slice and goes through k_chain_heavy (dg_chain.h: d_gen_candidates_wave, the staged pairing)
HEAVY_E = ("E_reach_heavy", "E_ahead_heavy")


def _heavy_slot(name, k):
    """where a heavy ladder's planted mate starts; the event read starts 301 bases behind it (E: the planted mate 1 itself)"""
    if name in HEAVY_MATE:
        return 660000 + 6000 * (N_SITES * HEAVY_MATE.index(name) + k)
    return 37000 + 20000 * k + 4000 * HEAVY_E.index(name)


def _plant_heavy(c):
    """fresh text (no 16-mer of it in the genome as the generator left it) where the heavy ladders' reads are cut, and the 17 copies of their mates"""
    rng = np.random.default_rng(GENOME_SEED + 3)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def fresh(n):
        while True:
            v = rng.integers(0, 4, n, dtype=np.uint8)
            if (count16(acgt[v].tobytes()) == 0).all():
                return v
    def flanked(v, before, after):
        """a copy with a base on either side that differs from the one beside the original, so that a read reaching over the original's end matches there alone"""
        return np.concatenate([[(before + 1) & 3], v, [(after + 1) & 3]]).astype(np.uint8)
    plan = []                                        # drawn first, against the text as it is, then written
    for j, name in enumerate(HEAVY_MATE):
        for k in range(N_SITES):
            S = _heavy_slot(name, k)
            plan.append((S + 241, fresh(520)))
            if name == "B_read_heavy":
                plan.append((S + 301 + 100030, fresh(250)))
            Y = fresh(101)
            plan.append((S, Y))
            Yc = flanked(Y, int(c[S - 1]), int(c[S + 101]))
            for i in range(HEAVY_COPIES - 1):
                plan.append((1300000 + 110 * ((N_SITES * j + k) * (HEAVY_COPIES - 1) + i), Yc))
    for j, name in enumerate(HEAVY_E):
        for k in range(N_SITES):
            a = _heavy_slot(name, k)
            around = fresh(150)
            plan.append((a - 20, around))
            if name == "E_reach_heavy":
                plan.append((a + 2000000 - 20, fresh(150)))
            X = fresh(101)
            plan.append((a, X))
            Xc = flanked(X, int(around[19]), int(around[121]))
            for i in range(HEAVY_COPIES - 1):
                plan.append((GENOME_LENGTHS[0] + 5000 + 110 * ((N_SITES * j + k) * (HEAVY_COPIES - 1) + i), Xc))
    for at, v in plan:
        c[at:at + len(v)] = v


def _g_places(k, j):
    make_genome()
    return _state["g_places"][k, j]


def text() -> bytes:
    make_genome()
    return _state["text"]


def codes_sha256() -> str:
    return hashlib.sha256(make_genome().codes.tobytes()).hexdigest()


def _kmer_table():
    """sorted 16-mers (as 32-bit numbers) of both strands of the text, and how often each occurs"""
    if "kmers" not in _state:
        c = make_genome().codes.astype(np.uint32)
        both = np.concatenate([c, (3 - c)[::-1]])
        v = np.zeros(len(both) - 15, np.uint32)
        for i in range(16):
            v = (v << np.uint32(2)) | both[i:len(both) - 15 + i]
        _state["kmers"] = np.unique(v, return_counts=True)
    return _state["kmers"]


def count16(s: bytes) -> np.ndarray:
    """per 16-mer of s: its occurrences in both strands of the text"""
    keys, counts = _kmer_table()
    c = _CODE[np.frombuffer(s, np.uint8)].astype(np.uint32)
    v = np.zeros(len(c) - 15, np.uint32)
    for i in range(16):
        v = (v << np.uint32(2)) | c[i:len(c) - 15 + i]
    at = np.minimum(np.searchsorted(keys, v), len(keys) - 1)
    return np.where(keys[at] == v, counts[at], 0)


def _not_unique_before():
    """cs[i]: how many of the forward text's 16-mers that start before base i do not occur exactly once in both strands"""
    if "cs" not in _state:
        c = count16(text())
        _state["cs"] = np.concatenate([[0], np.cumsum(c != 1)])
    return _state["cs"]


def _find(start: int, pieces, event_at: int | None = None, lo: int = 400, hi: int | None = None, also=None) -> int:
    """the first a >= start such that every piece (a + x, a + y) of the text holds 16-mers that occur once; with event_at, a + event_at is a multiple of 128"""
    if _state.get("force"):                          # (a heavy ladder: its sites are planted ones)
        return _state["force"].pop(0)
    cs = _not_unique_before()
    hi = GENOME_LENGTHS[0] - 400 if hi is None else hi
    a = max(start, lo)
    step = 53
    if event_at is not None:
        a += (-(a + event_at)) % 128
        step = 128
    while True:
        ok = also is None or also(a)
        for x, y in (pieces if ok else ()):
            if a + x < lo or a + y > hi or cs[a + y - 15] != cs[a + x]:
                ok = False
                break
        if ok:
            return a
        a += step


PIECES = []                                          # (ladder, site, start, end, expected count of every 16-mer) of every piece of text a read is cut from


def _note(ladder, k, spans, count=1):
    for x, y in spans:
        PIECES.append((ladder, k, x, y, count))


# ---- pairs ------------------------------------------------------------------------------------------------------------------------------------
def _orient(ev: bytes, e_lo: int, e_hi: int, k: int, ladder: str):
    """the event read (cut from text [e_lo, e_hi), forward) and a plain mate beside it -> (mate 1, mate 2, event mate) as sequenced.  Site k: strand k % 2,
    the event read is mate 1 for k // 2 even and mate 2 for k // 2 odd"""
    T = text()
    strand, as_m1 = k % 2, (k // 2) % 2 == 0
    if ladder in HEAVY_MATE:                         # the planted mate, upstream of the event read: the event read is mate 2 on the forward strand and mate 1 on the other
        lo = e_lo - MATE_GAP - MATE_LEN
        other = T[lo:lo + MATE_LEN]
        assert lo == _heavy_slot(ladder, k) and (count16(other) == HEAVY_COPIES).all(), (ladder, k)
        _note(ladder, k, [(lo, lo + MATE_LEN)], HEAVY_COPIES)
        return (other, revcomp(ev), 1) if strand == 0 else (revcomp(ev), other, 0)
    upstream = (strand == 0) == as_m1                # the event read is the fragment's upstream end
    if upstream:
        lo = e_hi + MATE_GAP
        other = T[lo:lo + MATE_LEN]
        m1, m2 = (ev, revcomp(other)) if strand == 0 else (revcomp(other), ev)
    else:
        lo = e_lo - MATE_GAP - MATE_LEN
        other = T[lo:lo + MATE_LEN]
        m1, m2 = (other, revcomp(ev)) if strand == 0 else (revcomp(ev), other)
    _note(ladder, k, [(lo, lo + MATE_LEN)])
    return m1, m2, 0 if as_m1 else 1


MATE_ROOM = [(-MATE_GAP - MATE_LEN, 0)]              # (relative to the event read's first base; the downstream mate's room is added per ladder)


def _rlen(k):
    return READ_LENGTHS[k % 3]


def _site_start(ladder_index: int, k: int) -> int:
    return 20000 + 61000 * k + 7000 * (ladder_index % 8) + 431 * ladder_index


class Rung(dict):
    pass


def _rung(ladder, k, value, m1, m2, ev):
    return Rung(ladder=ladder, site=k, value=int(value), m1=m1, m2=m2, event_mate=ev)


def _noise(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def _rng(ladder, k):
    return np.random.default_rng(int.from_bytes(hashlib.sha256(("%s/%d" % (ladder, k)).encode()).digest()[:4], "little"))


# ---- the ladders: each -> list of rungs -------------------------------------------------------------------------------------------------------------
def _gap_ladder(name, li, values, sub):
    """T[p:p+h] + T[p+h+L : ...]: the read leaves L text bases out after its first h bases"""
    T = text()
    out = []
    vmax = max(values)
    for k in range(N_SITES):
        n = _rlen(k)
        h = n // 2
        lo_room = MATE_GAP + MATE_LEN
        pieces = [(-lo_room, h), (h + min(values), h + vmax + (n - h) + lo_room)] if vmax > 1000 else [(-lo_room, h + vmax + (n - h) + lo_room)]
        p = _find(_site_start(li, k), pieces, event_at=h if k == 7 else None)
        for L in values:
            ev = T[p:p + h] + T[p + h + L:p + h + L + n - h]
            if sub:
                ev = _sub(ev, h - 4)
            _note(name, k, [(p, p + h), (p + h + L, p + h + L + n - h)])
            m1, m2, em = _orient(ev, p, p + h + L + n - h, k, name)
            out.append(_rung(name, k, L, m1, m2, em))
    return out


def _five(t):
    return [t - 2, t - 1, t, t + 1, t + 2]


def ladder_B_mates(name, li, t):
    """two plain mates; the text between their footprints is L bases"""
    T = text()
    out = []
    for k in range(N_SITES):
        p = _find(_site_start(li, k), [(0, 101), (101 + t - 2, 101 + t + 2 + 101)])
        for L in _five(t):
            x, y = T[p:p + 101], T[p + 101 + L:p + 202 + L]
            _note(name, k, [(p, p + 101), (p + 101 + L, p + 202 + L)])
            m1, m2 = (x, revcomp(y)) if k % 2 == 0 else (revcomp(y), x)
            out.append(_rung(name, k, L, m1, m2, (k // 2) % 2))
    return out


def ladder_B_chrend(name, li, strand):
    """first half a few hundred bases before the end of chromosome 1, second half starting d bases from the chromosome's last base (d < 0: before it).  On the
    forward strand the second half is the later seed and d is what :265 compares; the event read is mate 2 with its mate upstream in chromosome 1 (even k // 2) or
    mate 1 with its mate downstream in chromosome 2"""
    T = text()
    last = GENOME_LENGTHS[0] - 1
    out = []
    for k in range(N_SITES):
        n = _rlen(k)
        h = n // 2
        p = _find(last - 3000 - 700 * k - h, [(-MATE_GAP - MATE_LEN, h)], hi=sum(GENOME_LENGTHS))
        for d in (-2, -1, 0, 1, 2):
            q = last + d
            ev = T[p:p + h] + T[q:q + n - h]
            _note(name, k, [(p, p + h), (q, q + n - h)])
            up = (k // 2) % 2 == 0
            lo = p - MATE_GAP - MATE_LEN if up else last + 3 + n + MATE_GAP
            other = T[lo:lo + MATE_LEN]
            _note(name, k, [(lo, lo + MATE_LEN)])
            x, y = (other, ev) if up else (ev, other)
            m1, m2 = (x, revcomp(y)) if strand == 0 else (revcomp(y), x)
            out.append(_rung(name, k, d, m1, m2, int(up) if strand == 0 else 1 - int(up)))
    return out


def _mis_places(n, kmax, fast):
    """kmax places for substitutions in a read of n bases, 17 or more bases between the groups (so that a seed lies between them): single bases, or (more than
    7 places) pairs two apart.  A read with a junction (not fast: 250 bases, the junction behind base 125) keeps 25 bases on either side of it free"""
    if not fast or kmax > 7:
        assert n == 250 and kmax <= 14
        groups = [20, 45, 70, 95, 150, 175, 200]
        return groups[:kmax] if kmax <= 7 else [groups[i // 2] + 2 * (i % 2) for i in range(kmax)]
    step = min(25, (n - 20) // max(1, kmax))
    assert step >= 17, (n, kmax)
    return [20 + step * i for i in range(kmax)]


def ladder_C(name, li, m, fast):
    T = text()
    out = []
    ks = [k_ for k_ in _five(m) if k_ >= 0]
    for k in range(N_SITES):
        n = 250 if (m > 5 or not fast) else _rlen(k)
        if m == 5 and fast and n == 101:
            n = 150
        h = n // 2
        L = 0 if fast else 3000
        p = _find(_site_start(li, k), [(-MATE_GAP - MATE_LEN, h), (h + L, L + n + MATE_GAP + MATE_LEN)], event_at=h if k == 7 else None)
        base = T[p:p + h] + T[p + h + L:p + L + n]
        places = _mis_places(n, max(ks), fast)
        assert len(set(places)) == len(places) and max(places) < n - 17, (name, places)
        for kk in ks:
            ev = _subs(base, places[:kk])
            _note(name, k, [(p, p + h), (p + h + L, p + L + n)])
            m1, m2, em = _orient(ev, p, p + L + n, k, name)
            out.append(_rung(name, k, kk, m1, m2, em))
    return out


def ladder_D_rgap(name, li, how=0):
    """40 bases of text, g substituted bases, 3000 text bases left out, 60 bases of text"""
    T = text()
    out = []
    for k in range(N_SITES):
        p = _find(_site_start(li, k), [(-MATE_GAP - MATE_LEN, 3000 + 140 + MATE_GAP + MATE_LEN)], event_at=40 if k == 7 else None)
        for g in _five(20):
            e_hi = p + 40 + g + 3000 + 60
            mid = _gap_fill(T[p + 40:p + 40 + g], T[e_hi - 60 - g:e_hi - 60], how)
            ev = T[p:p + 40] + mid + T[e_hi - 60:e_hi]
            _note(name, k, [(p, p + 40), (e_hi - 60, e_hi)])
            m1, m2, em = _orient(ev, p, e_hi, k, name)
            out.append(_rung(name, k, g, m1, m2, em))
    return out


def ladder_D_jump(name, li):
    """40 bases of text, 25 read bases of which the first, the middle and the last are substituted, j text bases left out behind them, 60 bases of text"""
    T = text()
    out = []
    for k in range(N_SITES):
        p = _find(_site_start(li, k), [(-MATE_GAP - MATE_LEN, 140 + MATE_GAP + MATE_LEN)], event_at=40 if k == 7 else None)
        for j in (3, 4, 5, 6, 7):
            mid = _subs(T[p + 40:p + 65], (0, 12, 24))
            e_hi = p + 65 + j + 60
            ev = T[p:p + 40] + mid + T[e_hi - 60:e_hi]
            _note(name, k, [(p, p + 40), (e_hi - 60, e_hi)])
            m1, m2, em = _orient(ev, p, e_hi, k, name)
            out.append(_rung(name, k, j, m1, m2, em))
    return out


def ladder_E(name, li, t):
    """mate 1 = 101 bases at a, mate 2 = 101 bases at a + D, D around t (2 000 000: the reach; 0: mate 2 upstream of mate 1 by a base or two)"""
    T = text()
    out = []
    for k in range(N_SITES):
        a = _find(20000 + 21000 * k + 977 * li, [(0, 101), (t - 2, t + 2 + 101)] if t else [(-2, 103)], lo=2)
        for D in _five(t):
            x, y = T[a:a + 101], T[a + D:a + D + 101]
            if name in HEAVY_E:
                _note(name, k, [(a, a + 101)], HEAVY_COPIES)
                if t: _note(name, k, [(a + D, a + D + 101)])
            else:
                _note(name, k, [(a, a + 101), (a + D, a + D + 101)])
            m1, m2 = (x, revcomp(y)) if k % 2 == 0 else (revcomp(y), x)
            out.append(_rung(name, k, D, m1, m2, (k // 2) % 2))
    return out


def ladder_F(name, li, n):
    """c bases of text in the middle of a read of n bases, noise around them; the bases next to the text differ from the text's own, so the seed is c bases long"""
    T = text()
    thr = int(n * 0.3)
    out = []
    for k in range(N_SITES):
        rng = _rng(name, k)
        p = _find(_site_start(li, k), [(-MATE_GAP - MATE_LEN - n, n + MATE_GAP + MATE_LEN + n)])
        left = (n - thr) // 2
        while True:                                  # noise of which no 16-mer, alone or with the text beside it, occurs in the text
            nz = bytearray(_noise(rng, n))
            evs = []
            for c in _five(thr):
                ev = bytearray(nz)
                ev[left:left + c] = T[p:p + c]
                ev[left - 1] = _sub(T[p - 1:p], 0)[0]
                ev[left + c] = _sub(T[p + c:p + c + 1], 0)[0]
                evs.append(bytes(ev))
            if all((count16(e)[[i for i in range(n - 15) if i < left or i + 16 > left + c]] == 0).all() for e, c in zip(evs, _five(thr))):
                break
        for c, ev in zip(_five(thr), evs):
            _note(name, k, [(p, p + c)] if c >= 16 else [])
            m1, m2, em = _orient(bytes(ev), p - left, p - left + n, k, name)
            out.append(_rung(name, k, c, m1, m2, em))
    return out


def ladder_G(name, li):
    """101 bases of text at p with base 101 - d substituted; the text holds the first 101 - d of them once more, 200 kb downstream (make_genome), followed by a
    third letter.  The read's seeds are its first 101 - d bases (at both places) and its last d - 1 (at p): two candidates of 100 and 101 - d bases.  (Without the
    substitution the read is one seed of 101 bases that only p holds, and the second place gets no seed at all.)  The rung's value is the scores' difference"""
    T = text()
    out = []
    for k in range(N_SITES):
        for j, d in enumerate(G_DS):
            p, q = _g_places(k, j)
            ev = _sub(T[p:p + 101], 101 - d)
            assert T[q:q + 101 - d] == ev[:101 - d] and T[q + 101 - d] not in (ev[101 - d], T[p + 101 - d])
            assert (count16(ev[:101 - d]) == 2).all() and (count16(T[p + 101 - d - 14:p + 101]) == 1).all(), (name, k, d)
            _note(name, k, [(p, p + 101 - d)], 2)
            _note(name, k, [(p + 101 - d + 1, p + 101)])
            m1, m2, em = _orient(ev, p, p + 101, k, name)
            out.append(_rung(name, k, d - 1, m1, m2, em))
    return out


def ladder_H(name, li, r):
    """40 bases of text, the next r text bases with x of them substituted, 3000 text bases left out, 50 bases of text: a read gap of r bases beside a junction"""
    T = text()
    thr = r - int(r * 0.8) if name.startswith("H_gap_") else 2
    out = []
    for k in range(N_SITES):
        # (the junction where it can lie at one place only: the three text bases behind the gap differ from the exon's first three, and the three before the exon from the gap's last three)
        clear = lambda a: all(T[a + 40 + r + i] != T[a + 40 + r + 3000 + i] and T[a + 40 + r - 1 - i] != T[a + 40 + r + 3000 - 1 - i] for i in range(3))
        p = _find(_site_start(li, k), [(-MATE_GAP - MATE_LEN, 3000 + 130 + MATE_GAP + MATE_LEN)], event_at=40 if k == 7 else None, also=clear)
        xs = [x for x in _five(thr) if x >= 0]
        for x in xs:
            places = [int((i + 0.5) * r / x) for i in range(x)]             # x places spread evenly over the gap
            assert len(set(places)) == x
            mid = _subs(T[p + 40:p + 40 + r], places)
            e_hi = p + 40 + r + 3000 + 50
            ev = T[p:p + 40] + mid + T[e_hi - 50:e_hi]
            _note(name, k, [(p, p + 40), (e_hi - 50, e_hi)])
            m1, m2, em = _orient(ev, p, e_hi, k, name)
            out.append(_rung(name, k, x, m1, m2, em))
    return out


def ladder_I_reseed(name, li):
    """40 bases of text, a read gap of g bases, 3000 text bases left out, 50 bases of text.  The gap holds 2 substituted bases, 15 bases of the text behind the left seed,
    one substituted base, 15 more bases of that text, and g - 33 substituted bases: no stretch of 16, so no seed; the second search of the gap finds a chain of 8-mers of
    l = 31 bases on the left seed's diagonal, which it keeps when l >= (int)(g * 0.85): g <= 37"""
    T = text()
    out = []
    for k in range(N_SITES):
        p = _find(_site_start(li, k), [(-MATE_GAP - MATE_LEN, 3000 + 140 + MATE_GAP + MATE_LEN)], event_at=40 if k == 7 else None)
        for g in (35, 36, 37, 38, 39):
            e_hi = p + 40 + g + 3000 + 50
            mid = bytearray(_gap_fill(T[p + 40:p + 40 + g], T[e_hi - 50 - g:e_hi - 50], 0))
            mid[2:17] = T[p + 42:p + 57]
            mid[18:33] = T[p + 58:p + 73]
            ev = T[p:p + 40] + bytes(mid) + T[e_hi - 50:e_hi]
            _note(name, k, [(p, p + 73), (e_hi - 50, e_hi)])
            m1, m2, em = _orient(ev, p, e_hi, k, name)
            out.append(_rung(name, k, g, m1, m2, em))
    return out


K_ZONE, K_SITE = 1420000, 66000
K_SHAPES = ((27, 37), (25, 40), (40, 25), (13, 77), (77, 13))       # (na, nb): 999, 1000, 1000, 1001, 1001 -- 998 and 1002 have no two factors within max_dup's 100


def _plant_K(c):
    """per site and shape: mate 2's text Y (101 bases) nb times -- nb - 1 copies below everything else and one 300 bases behind X -- and mate 1's text in two forms:
    A (80 bases) + a base + B (20 bases) na - 1 times above everything else (the decoys), and A + that base + other text once at X.  Mate 1 reads A + another base + B:
    its seeds are A (na places) and B (the decoys), so its candidates score 100 (decoys) and 80 (X); only the candidate at X has a mate downstream"""
    rng = np.random.default_rng(GENOME_SEED + 2)
    fam = {}
    for k in range(N_SITES):
        S = K_ZONE + K_SITE * k
        z2, xs, z1 = S, S + 29000, S + 33000
        for j, (na, nb) in enumerate(K_SHAPES):
            while True:                              # (text of which no 16-mer occurs in the genome as the generator left it)
                A, B, Y = (rng.integers(0, 4, n, dtype=np.uint8) for n in (80, 20, 101))
                if all((count16(np.frombuffer(b"ACGT", np.uint8)[v].tobytes()) == 0).all() for v in (A, B, Y)):
                    break
            cp = int(rng.integers(0, 4))
            for i in range(nb - 1):
                c[z2:z2 + 101] = Y; z2 += 150
            X = xs + 700 * j
            c[X:X + 80] = A; c[X + 80] = cp; c[X + 81] = (int(B[0]) + 1) & 3
            c[X + 300:X + 401] = Y
            for i in range(na - 1):
                c[z1:z1 + 80] = A; c[z1 + 80] = cp; c[z1 + 81:z1 + 101] = B; z1 += 150
            fam[k, j] = (A.copy(), B.copy(), Y.copy(), cp, X)
        assert z2 <= xs and z1 <= S + K_SITE
    return fam


def ladder_K(name, li):
    make_genome()
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for k in range(N_SITES):
        for j, (na, nb) in enumerate(K_SHAPES):
            A, B, Y, cp, X = _state["k_fam"][k, j]
            u = acgt[A].tobytes() + b"ACGT"[(cp + 2) & 3:][:1] + acgt[B].tobytes()
            y = acgt[Y].tobytes()
            assert (count16(u[:80]) == na).all() and (count16(u[81:]) == na - 1).all() and (count16(y) == nb).all(), (name, k, j)
            _note(name, k, [(X, X + 80)], na); _note(name, k, [(X + 300, X + 401)], nb)
            m1, m2 = (u, revcomp(y)) if k % 2 == 0 else (revcomp(y), u)
            out.append(_rung(name, k, na * nb, m1, m2, k % 2))
    return out


def _build():
    lad = {}
    li = [0]

    def add(name, rungs, run, flip, mode="pe", key="shape"):
        lad[name] = dict(rungs=rungs, run=run, mode=mode, flip=flip, key=key)
        li[0] += 1

    for t, run in ((5, "d"), (10, "i10"), (31, "i31")):
        add("A_clean_t%d" % t, _gap_ladder("A_clean_t%d" % t, li[0], _five(t), False), run, (t - 1, t), key="spliced")
        add("A_sub_t%d" % t, _gap_ladder("A_sub_t%d" % t, li[0], _five(t), True), run, (t, t + 1), key="filled")
    for t, run in ((100000, "i10"), (500000, "d")):
        add("B_read_t%d" % t, _gap_ladder("B_read_t%d" % t, li[0], _five(t), False), run, (t - 1, t), key="spliced")
        add("B_mates_t%d" % t, ladder_B_mates("B_mates_t%d" % t, li[0], t), run, None, key="proper")
    add("B_chrend", ladder_B_chrend("B_chrend", li[0], 0), "d", (-1, 0), key="spliced")
    add("B_chrend_rev", ladder_B_chrend("B_chrend_rev", li[0], 1), "d", "unjudged", key="shape")
    for m, run in ((0, "m0"), (1, "m1"), (2, "m2"), (5, "d"), (12, "m12m")):
        add("C_fast_m%d" % m, ladder_C("C_fast_m%d" % m, li[0], m, True), run, (m, m + 1), key="mapped")
        add("C_report_m%d" % m, ladder_C("C_report_m%d" % m, li[0], m, False), run, (m, m + 1), key="mapped")
    add("D_rgap", ladder_D_rgap("D_rgap", li[0], 0), "m30", (20, 21), key="n_reseed")
    add("D_jump", ladder_D_jump("D_jump", li[0]), "m30", (5, 6), key="n_reseed")
    add("E_reach", ladder_E("E_reach", li[0], 2000000), "d", (1999999, 2000000), key="proper")
    add("E_ahead", ladder_E("E_ahead", li[0], 0), "d", (-1, 0), key="proper")
    for n in (50, 100, 101, 150, 250):
        add("F_cov_r%d" % n, ladder_F("F_cov_r%d" % n, li[0], n), "d", (int(n * 0.3), int(n * 0.3) + 1), key="mapped")
    add("G_cut", ladder_G("G_cut", li[0]), "m12m", (20, 21), mode="se", key="n_hit")
    add("G_cut_single", lad["G_cut"]["rungs"], "d", (20, 21), mode="se", key="n_hit")
    for r in (10, 15, 20, 25):
        t = r - int(r * 0.8)
        add("H_gap_r%d" % r, ladder_H("H_gap_r%d" % r, li[0], r), "m12m", (t, t + 1), key="filled")
    add("H_gapmis_r20", ladder_H("H_gapmis_r20", li[0], 20), "m2", (2, 3), key="filled")
    add("I_reseed", ladder_I_reseed("I_reseed", li[0]), "m30", (37, 38), key="reseeded")
    add("K_product", ladder_K("K_product", li[0]), "d", (1000, 1001), key="proper")
    # the same comparisons inside units of more than 16 seeds: k_chain_heavy's forms (dg_chain.h:217, :239-240, :398)
    def forced(name, off):
        _state["force"] = [_heavy_slot(name, k) + off for k in range(N_SITES)]
    forced("B_read_heavy", 301)
    add("B_read_heavy", _gap_ladder("B_read_heavy", li[0], _five(100000), False), "i10", (99999, 100000), key="spliced")
    forced("D_jump_heavy", 301)
    add("D_jump_heavy", ladder_D_jump("D_jump_heavy", li[0]), "m30", (5, 6), key="n_reseed")
    forced("F_cov_heavy", 336)
    add("F_cov_heavy", ladder_F("F_cov_heavy", li[0], 100), "d", (30, 31), key="mapped")
    forced("E_reach_heavy", 0)
    add("E_reach_heavy", ladder_E("E_reach_heavy", li[0], 2000000), "d", (1999999, 2000000), key="proper")
    forced("E_ahead_heavy", 0)
    add("E_ahead_heavy", ladder_E("E_ahead_heavy", li[0], 0), "d", (-1, 0), key="proper")
    assert not _state["force"]
    return lad


def ladders():
    """{name: dict(rungs, run, mode, flip, key)}: the run ('pe' / 'se', key of RUNS) whose records judge the ladder, the two neighbouring values between
    which the outcome flips (None: a control that must not flip), and the outcome looked at (test_thresholds_oracle.outcome)"""
    if "ladders" not in _state:
        make_genome()
        del PIECES[:]
        _state["ladders"] = _build()
    return _state["ladders"]


def all_rungs():
    """every rung once, in ladder order (G_cut_single shares G_cut's reads)"""
    out = []
    for name, l in ladders().items():
        if name != "G_cut_single":
            out += l["rungs"]
    return out


def rung_index():
    """{(ladder, site, value): index of the pair in all_rungs()}"""
    idx = {(r["ladder"], r["site"], r["value"]): i for i, r in enumerate(all_rungs())}
    for r in ladders()["G_cut"]["rungs"]:
        idx[("G_cut_single", r["site"], r["value"])] = idx[("G_cut", r["site"], r["value"])]
    return idx


def stored(rungs):
    """the batch as the loader stores it: mate 1, then mate 2 reverse-complemented, alternating"""
    out = []
    for r in rungs:
        out.append(r["m1"]); out.append(revcomp(r["m2"]))
    return out


def reads_sha256() -> str:
    return hashlib.sha256(b"\n".join(stored(all_rungs()))).hexdigest()


def write_fastq(path1: str, path2: str, rungs) -> None:
    with open(path1, "wb") as f1, open(path2, "wb") as f2:
        for i, r in enumerate(rungs):
            f1.write(b"@t%d/1\n" % i + r["m1"] + b"\n+\n" + b"I" * len(r["m1"]) + b"\n")
            f2.write(b"@t%d/2\n" % i + r["m2"] + b"\n+\n" + b"I" * len(r["m2"]) + b"\n")


def write_single_fastq(path: str, rungs) -> None:
    """every mate as a read of its own, as stored"""
    with open(path, "wb") as f:
        for i, s in enumerate(stored(rungs)):
            f.write(b"@s%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n")


def batch(rungs):
    return host.pack_reads(stored(rungs))


def padded_2bit(reads):
    n = max(len(r) for r in reads)
    arr = np.full((len(reads), n), ord("A"), np.uint8)
    for i, r in enumerate(reads):
        arr[i, :len(r)] = np.frombuffer(r, np.uint8)
    words, nlist = host.pack_reads_2bit(arr)
    return words, nlist, n, np.asarray([len(r) for r in reads], np.uint16)
