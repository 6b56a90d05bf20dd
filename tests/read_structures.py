"""Named read and pair structures that dart_amd/synth.py::make_reads never makes: several junctions in one read, short exon
overhangs, long indels, indels at a read's end or beside a junction, stretches of noise, tandem gains and losses, chimeras, reads
across the seams of the text, and pairs that are not two mates facing each other on one chromosome.

Pure numpy, a pure function of (genome, seed, read length): `make` returns {class name: [(mate 1 bytes, mate 2 bytes), ...]} with
both mates as sequenced (the loader reverse-complements mate 2, host.interleave_pairs / GetData.cpp:157-162); `make_with_info`
adds, per pair, what was planted (which mate holds the event, its size).  Exon ends are put on GT..AG / CT..AC dinucleotides that
the genome already holds (found forward from a random position), so the index of the genome is the one the other tests use; one
exon end in four has no motif.  In the spliced and indel classes half of the pairs carry substitutions at 1 % on top."""
from __future__ import annotations

import numpy as np

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = np.full(256, ord("N"), np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    _COMP[_a] = _b

SPLICED_AND_INDEL = ("two_junctions", "three_junctions", "overhang", "junction_in_both_mates", "del_4_30", "del_31_120", "ins_4_30", "ins_31_80",
                     "two_indels", "indel_near_end", "indel_beside_junction")
NOISE = ("noise_island", "two_noise_islands", "noise_head", "noise_tail")
TANDEM = ("tandem_dup_in_read", "tandem_loss_in_read")
CHIMERA = ("chimera_other_strand", "chimera_other_chromosome", "chimera_backwards", "chimera_three_parts")
SEAMS = ("across_chromosome_boundary",)
PAIRS = ("pair_same_strand", "pair_outie", "pair_contained", "pair_dovetail", "pair_identical_mates", "pair_other_chromosome", "pair_far", "pair_mate_noise",
         "pair_mate_high_copy", "pair_both_multi", "pair_unequal_length", "pair_swapped_files")
MIDDLE_EXON_RANGES = ((6, 11), (12, 15), (16, 30), (31, 60))


def rc(a: np.ndarray) -> np.ndarray:
    return _COMP[a[::-1]]


class _Skip(Exception):
    """a draw that does not fit its chromosome (or finds no site): the class draws again"""


class _G:
    """the genome as characters, with what the classes look up in it"""

    def __init__(self, genome):
        self.codes = np.asarray(genome.codes, np.uint8)
        self.asc = _ACGT[self.codes]
        self.lo = np.asarray(genome.offsets, np.int64)
        self.hi = self.lo + np.asarray(genome.lengths, np.int64)
        self.total = int(self.hi[-1])
        c = self.codes
        di = c[:-1].astype(np.int16) * 4 + c[1:]
        # intron [s, e): donor dinucleotide at s, acceptor dinucleotide at e-2.  kind 0: GT..AG, kind 1: CT..AC
        self.donor = (np.nonzero(di == 2 * 4 + 3)[0], np.nonzero(di == 1 * 4 + 3)[0])
        self.accept = (np.nonzero(di == 0 * 4 + 2)[0] + 2, np.nonzero(di == 0 * 4 + 1)[0] + 2)
        self._kmers = None
        self._tandems = None
        self._runs = {}

    def chrom(self, p):
        """the chromosome that holds text position p (a position outside the text: the draw does not fit)"""
        if p < 0 or p >= self.total:
            raise _Skip
        return int(np.searchsorted(self.hi, p, side="right"))

    def seq(self, a, b):
        ci = self.chrom(a)
        if a < self.lo[ci] or b > self.hi[ci] or b <= a:
            raise _Skip
        return self.asc[a:b]

    CENSUS = 2000000          # repeats are looked for in the first two million bases (all of the golden genomes; a part of a large one, whose families then count for less than they are)

    def kmer_counts(self):
        """per text position (of the first CENSUS): how often the 32-mer that starts there occurs among them, on either strand"""
        if self._kmers is None:
            K = 32
            n = min(len(self.codes), self.CENSUS) - K + 1
            f = np.zeros(n, np.uint64); r = np.zeros(n, np.uint64)
            for t in range(K):
                w = self.codes[t:t + n].astype(np.uint64)
                f |= w << np.uint64(2 * (K - 1 - t))
                r |= (np.uint64(3) - w) << np.uint64(2 * t)
            canon = np.minimum(f, r)
            _, inv, cnt = np.unique(canon, return_inverse=True, return_counts=True)
            self._kmers = cnt[inv.reshape(-1)]
        return self._kmers

    def family_runs(self, lo, hi, min_len):
        """runs of at least min_len text positions whose 32-mer occurs lo..hi times"""
        if (lo, hi, min_len) not in self._runs:
            cnt = self.kmer_counts()
            self._runs[lo, hi, min_len] = self.runs((cnt >= lo) & (cnt <= hi), min_len)
        return self._runs[lo, hi, min_len]

    def runs(self, mask, min_len):
        """starts and lengths of the runs of True of at least min_len"""
        m = np.concatenate([[False], mask, [False]])
        d = np.diff(m.astype(np.int8))
        s = np.nonzero(d == 1)[0]; e = np.nonzero(d == -1)[0]
        keep = (e - s) >= min_len
        return s[keep], (e - s)[keep]

    def tandems(self):
        """(start, unit, copies) of the exact tandem repeats of unit 11..47 with at least four copies"""
        if self._tandems is None:
            out = []
            c = self.codes[:self.CENSUS]
            for u in range(11, 48):
                s, l = self.runs(c[:-u] == c[u:], 3 * u)
                out += [(int(a), u, int(b) // u + 1) for a, b in zip(s, l)]
            kept, seen = [], set()
            for a, u, k in sorted(out, key=lambda t: t[1]):          # a run of unit u is also one of unit 2u, 3u: the smallest unit is kept
                if not any((a // 64 + d) in seen for d in (-1, 0, 1)):
                    seen.add(a // 64); kept.append((a, u, k))
            self._tandems = kept
        return self._tandems


def _rand(rng, n):
    return _ACGT[rng.integers(0, 4, size=int(n))]


def _pos(rng, G, left, right, ci=None):
    """a position p with [p - left, p + right) inside one chromosome"""
    if ci is None:
        ci = int(rng.integers(0, len(G.lo)))
    if G.hi[ci] - G.lo[ci] < left + right + 2:
        raise _Skip
    return ci, int(rng.integers(G.lo[ci] + left, G.hi[ci] - right))


def _next(arr, p):
    k = int(np.searchsorted(arr, p))
    if k >= len(arr):
        raise _Skip
    return int(arr[k])


def _intron(rng, G, near, kind=None, lo=200, hi=30000):
    """an intron [s, e) whose donor is the first one at or after `near`: (s, e, kind); kind 2 has no motif"""
    if kind is None:
        r = rng.random()
        kind = 2 if r < 0.25 else (0 if r < 0.625 else 1)
    ilen = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
    if kind == 2:
        return near, near + ilen, 2
    s = _next(G.donor[kind], near)
    e = _next(G.accept[kind], s + ilen)
    return s, e, kind


def _acceptor_then_donor(rng, G, s, kind, mlo, mhi, lo=200, hi=30000):
    """an intron [s, e) and a middle exon [e, e + m) with m in mlo..mhi that ends on a donor of the same kind: (e, m)"""
    ilen = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
    if kind == 2:
        return s + ilen, int(rng.integers(mlo, mhi + 1))
    acc, don = G.accept[kind], G.donor[kind]
    k = int(np.searchsorted(acc, s + ilen))
    for e in acc[k:k + 200].tolist():
        j = int(np.searchsorted(don, e + mlo))
        if j < len(don) and don[j] <= e + mhi:
            return e, int(don[j]) - e
    raise _Skip


def _transcript_read(G, rlen, first_donor, head, exons):
    """read of rlen bases: `head` bases that end at first_donor, then the exons [(start, length or None)], the last one open-ended.
    -> (bytes as a uint8 array, leftmost text position, rightmost text position + 1)"""
    parts = [G.seq(first_donor - head, first_donor)]
    left = rlen - head
    end = first_donor
    for a, m in exons:
        m = left if m is None else min(m, left)
        if m <= 0:
            raise _Skip
        parts.append(G.seq(a, a + m)); left -= m; end = a + m
    if left:
        raise _Skip
    if G.chrom(first_donor - head) != G.chrom(end - 1):
        raise _Skip
    return np.concatenate(parts), first_donor - head, end


def _orient(rng, L, R, event_is_left):
    """two forward-strand reads, L left of R -> (mate 1, mate 2 as sequenced, index of the mate that holds the event)"""
    if rng.random() < 0.5:
        return L, rc(R), 0 if event_is_left else 1
    return rc(R), L, 1 if event_is_left else 0


def _with_mate(rng, G, ev, lo, hi, rlen):
    """the event read (forward strand, over text [lo, hi)) and a plain mate 150-300 bases downstream or upstream of it"""
    gap = int(rng.integers(150, 301))
    ci = G.chrom(lo)
    down = rng.random() < 0.5
    if down and hi + gap + rlen > G.hi[ci]: down = False
    if not down and lo - gap - rlen < G.lo[ci]: down = True
    if down:
        return _orient(rng, ev, G.seq(hi + gap, hi + gap + rlen), True)
    return _orient(rng, G.seq(lo - gap - rlen, lo - gap), ev, False)


def _substitute(rng, a, rate=0.01):
    a = a.copy()
    m = rng.random(len(a)) < rate
    for q in np.nonzero(m)[0]:
        a[q] = [c for c in b"ACGT" if c != a[q]][int(rng.integers(0, 3))]
    return a


# ---- the classes: each draws one pair -> (mate 1, mate 2, info) ----
def _two_junctions(rng, G, rlen, k):
    mlo, mhi = MIDDLE_EXON_RANGES[k % 4]
    _, near = _pos(rng, G, rlen + 400, 70000)
    s1, _, kind = _intron(rng, G, near)
    e1, m = _acceptor_then_donor(rng, G, s1, kind, mlo, mhi)
    s2 = e1 + m
    ilen2 = int(np.exp(rng.uniform(np.log(200), np.log(30000))))
    e2 = s2 + ilen2 if kind == 2 else _next(G.accept[kind], s2 + ilen2)
    head = int(rng.integers(20, rlen - m - 20 + 1))
    ev, lo, hi = _transcript_read(G, rlen, s1, head, [(e1, m), (e2, None)])
    m1, m2, who = _with_mate(rng, G, ev, lo, hi, rlen)
    return m1, m2, dict(event_mate=who, middle_exon=m, motif=kind)


def _three_junctions(rng, G, rlen, k):
    """two middle exons, each of 12-15, 16-30 or 31-60 bases (the nine combinations in turn: in four of nine both are at least 16 bases, which the reference
    reports as three N operations)"""
    ra, rb = MIDDLE_EXON_RANGES[1 + k % 3], MIDDLE_EXON_RANGES[1 + (k // 3) % 3]
    _, near = _pos(rng, G, rlen + 400, 100000)
    s1, _, kind = _intron(rng, G, near)
    e1, ma = _acceptor_then_donor(rng, G, s1, kind, *ra)
    e2, mb = _acceptor_then_donor(rng, G, e1 + ma, kind, *rb)
    s3 = e2 + mb
    ilen3 = int(np.exp(rng.uniform(np.log(200), np.log(30000))))
    e3 = s3 + ilen3 if kind == 2 else _next(G.accept[kind], s3 + ilen3)
    head = int(rng.integers(25, rlen - ma - mb - 25 + 1))
    ev, lo, hi = _transcript_read(G, rlen, s1, head, [(e1, ma), (e2, mb), (e3, None)])
    m1, m2, who = _with_mate(rng, G, ev, lo, hi, rlen)
    return m1, m2, dict(event_mate=who, middle_exons=(ma, mb), motif=kind)


def _overhang(rng, G, rlen, k):
    j = k // 2                                      # half of the pairs 1..13 bases (clipped by the reference), half 14..19 (a junction or a clip)
    over, at_start = (1 + j % 13, (j // 13) % 2 == 0) if k % 2 == 0 else (14 + j % 6, (j // 6) % 2 == 0)
    _, near = _pos(rng, G, rlen + 400, 40000)
    s, e, kind = _intron(rng, G, near)
    head = over if at_start else rlen - over
    ev, lo, hi = _transcript_read(G, rlen, s, head, [(e, None)])
    m1, m2, who = _with_mate(rng, G, ev, lo, hi, rlen)
    return m1, m2, dict(event_mate=who, overhang=over, at_start=at_start, motif=kind)


def _junction_in_both_mates(rng, G, rlen, k):
    _, near = _pos(rng, G, rlen + 400, 80000)
    s1, e1, kind = _intron(rng, G, near)
    if k % 2:                                       # the same junction, covered by both mates
        h1 = int(rng.integers(rlen - 40, rlen - 20)); h2 = int(rng.integers(20, 40))
        L, _, _ = _transcript_read(G, rlen, s1, h1, [(e1, None)])
        R, _, _ = _transcript_read(G, rlen, s1, h2, [(e1, None)])
        m1, m2, _ = _orient(rng, L, R, True)
        return m1, m2, dict(event_mate=2, same_junction=True, motif=kind)
    h1 = int(rng.integers(25, rlen - 25))
    L, _, endL = _transcript_read(G, rlen, s1, h1, [(e1, None)])
    s2, e2, _ = _intron(rng, G, endL + int(rng.integers(120, 260)), kind=kind)
    h2 = int(rng.integers(25, rlen - 25))
    if s2 - h2 < endL - 30:
        raise _Skip
    R, _, _ = _transcript_read(G, rlen, s2, h2, [(e2, None)])
    m1, m2, _ = _orient(rng, L, R, True)
    return m1, m2, dict(event_mate=2, same_junction=False, motif=kind)


def _deletion(dlo, dhi):
    def f(rng, G, rlen, k):
        d = int(rng.integers(dlo, dhi + 1))
        j = int(rng.integers(20, rlen - 20 + 1))
        _, a = _pos(rng, G, 400, rlen + d + 400)
        ev = np.concatenate([G.seq(a, a + j), G.seq(a + j + d, a + d + rlen)])
        m1, m2, who = _with_mate(rng, G, ev, a, a + d + rlen, rlen)
        return m1, m2, dict(event_mate=who, deletion=d)
    return f


def _insertion(nlo, nhi):
    def f(rng, G, rlen, k):
        n = int(rng.integers(nlo, nhi + 1))
        j = int(rng.integers(20, rlen - n - 20 + 1))
        _, a = _pos(rng, G, 400, rlen + 400)
        ev = np.concatenate([G.seq(a, a + j), _rand(rng, n), G.seq(a + j, a + rlen - n)])
        m1, m2, who = _with_mate(rng, G, ev, a, a + rlen - n, rlen)
        return m1, m2, dict(event_mate=who, insertion=n)
    return f


def _edit(rng, G, a, rlen, edits):
    """text from a on with edits [(read offset, +n inserted / -n deleted)] in ascending order, cut to rlen -> (read, text end)"""
    parts, have, t = [], 0, a
    for off, n in edits:
        parts.append(G.seq(t, t + off - have)); t += off - have; have = off
        if n > 0:
            parts.append(_rand(rng, n)); have += n
        else:
            t += -n
    parts.append(G.seq(t, t + rlen - have)); t += rlen - have
    ev = np.concatenate(parts)
    if len(ev) != rlen:
        raise _Skip
    return ev, t


def _sign(rng, n):
    return n if rng.random() < 0.5 else -n


def _two_indels(rng, G, rlen, k):
    n1, n2 = _sign(rng, int(rng.integers(1, 6))), _sign(rng, int(rng.integers(1, 6)))
    dist = int(rng.integers(25, 51))
    q1 = int(rng.integers(15, rlen - dist - 25))
    e = [(q1, n1), (q1 + max(n1, 0) + dist, n2)]
    _, a = _pos(rng, G, 400, rlen + 420)
    ev, end = _edit(rng, G, a, rlen, e)
    m1, m2, who = _with_mate(rng, G, ev, a, end, rlen)
    return m1, m2, dict(event_mate=who, indels=e)


def _indel_near_end(rng, G, rlen, k):
    n = _sign(rng, int(rng.integers(1, 4))); dist = int(rng.integers(2, 10))
    q = dist if k % 2 == 0 else rlen - dist - max(n, 0)
    _, a = _pos(rng, G, 400, rlen + 420)
    ev, end = _edit(rng, G, a, rlen, [(q, n)])
    m1, m2, who = _with_mate(rng, G, ev, a, end, rlen)
    return m1, m2, dict(event_mate=who, indel=n, from_end=dist, at_start=k % 2 == 0)


def _indel_beside_junction(rng, G, rlen, k):
    """an indel of 1-3 bases whose nearer edge lies 2-12 read bases in front of the junction, or behind it"""
    _, near = _pos(rng, G, rlen + 400, 40000)
    s, e, kind = _intron(rng, G, near)
    head = int(rng.integers(30, rlen - 30))
    ev, lo, hi = _transcript_read(G, rlen + 8, s, head, [(e, None)])
    n = _sign(rng, int(rng.integers(1, 4))); dist = int(rng.integers(2, 13))
    q = head - dist + min(n, 0) if k % 2 == 0 else head + dist         # (in front: inserted bases end, or deleted text ends, `dist` bases before the junction)
    ev = np.concatenate([ev[:q], _rand(rng, n), ev[q:]]) if n > 0 else np.concatenate([ev[:q], ev[q - n:]])
    ev = ev[:rlen]
    m1, m2, who = _with_mate(rng, G, ev, lo, hi, rlen)
    return m1, m2, dict(event_mate=who, indel=n, from_junction=dist, motif=kind)


def _noise_island(rng, G, rlen, k):
    w = int(rng.integers(20, 41)); j = int(rng.integers(20, rlen - w - 20 + 1))
    _, a = _pos(rng, G, 400, rlen + 400)
    ev = G.seq(a, a + rlen).copy(); ev[j:j + w] = _rand(rng, w)
    m1, m2, who = _with_mate(rng, G, ev, a, a + rlen, rlen)
    return m1, m2, dict(event_mate=who, noise=w)


def _two_noise_islands(rng, G, rlen, k):
    """two short stretches of text, each followed by noise, in front of the read's long stretch (for every second pair: behind it).  The noise
    is up to 2 bases longer or shorter than the text it replaces, so the segment pairs beside the long stretch are generic (unequal) ones."""
    w1, w2 = int(rng.integers(10, 21)), int(rng.integers(10, 21))
    g0, g1 = int(rng.integers(16, 23)), int(rng.integers(16, 23))
    d1, d2 = int(rng.integers(-2, 3)), int(rng.integers(-2, 3))
    rest = rlen - g0 - w1 - g1 - w2
    layout = [(g0, 0), (w1, w1 + d1), (g1, 0), (w2, w2 + d2), (rest, 0)]          # (read bases, text bases skipped when they are noise)
    if k % 2:
        layout = layout[::-1]
    _, a = _pos(rng, G, 400, rlen + 420)
    parts, t = [], a
    for n, skip in layout:
        if skip:
            parts.append(_rand(rng, n)); t += skip
        else:
            parts.append(G.seq(t, t + n)); t += n
    ev = np.concatenate(parts)
    m1, m2, who = _with_mate(rng, G, ev, a, t, rlen)
    return m1, m2, dict(event_mate=who, noise=(w1, w2), long_stretch_first=bool(k % 2))


def _noise_end(head):
    def f(rng, G, rlen, k):
        w = int(rng.integers(15, 41))
        _, a = _pos(rng, G, 400, rlen + 400)
        ev = G.seq(a, a + rlen).copy()
        if head: ev[:w] = _rand(rng, w)
        else: ev[rlen - w:] = _rand(rng, w)
        m1, m2, who = _with_mate(rng, G, ev, a, a + rlen, rlen)
        return m1, m2, dict(event_mate=who, noise=w)
    return f


def _tandem(dup):
    def f(rng, G, rlen, k):
        tr = G.tandems()
        if k % 2 and tr:                             # one of the genome's own tandem repeats: one unit more or one unit less than the text holds
            a0, u, copies = tr[int(rng.integers(0, len(tr)))]
            j = int(rng.integers(20, max(21, rlen - 2 * u - 20)))
            a = a0 + u * int(rng.integers(0, max(1, copies - 2))) - j
            own = True
        else:
            u = int(rng.integers(12, min(40, (rlen - 40) // 2 if dup else 40) + 1))     # (a doubled unit and 20 bases on either side fit the read)
            j = int(rng.integers(20, rlen - (2 * u if dup else 0) - 20 + 1))
            _, a = _pos(rng, G, 400, rlen + 460)
            own = False
        if dup:
            ev = np.concatenate([G.seq(a, a + j + u), G.seq(a + j, a + j + u), G.seq(a + j + u, a + rlen)])[:rlen]
            end = a + rlen - u
        else:
            ev = np.concatenate([G.seq(a, a + j), G.seq(a + j + u, a + u + rlen)])
            end = a + u + rlen
        if len(ev) != rlen:
            raise _Skip
        m1, m2, who = _with_mate(rng, G, ev, a, end, rlen)
        return m1, m2, dict(event_mate=who, unit=u, own_repeat=own)
    return f


def _chimera(kind):
    def f(rng, G, rlen, k):
        h = int(rng.integers(int(0.4 * rlen), int(0.6 * rlen) + 1))
        ci, a = _pos(rng, G, 6000, rlen + 6000)
        first = G.seq(a, a + h)
        if kind == "other_strand":
            _, b = _pos(rng, G, 10, rlen + 10, ci)
            parts = [first, rc(G.seq(b, b + rlen - h))]
        elif kind == "other_chromosome":
            cj = (ci + 1 + int(rng.integers(0, max(1, len(G.lo) - 1)))) % len(G.lo)
            _, b = _pos(rng, G, 10, rlen + 10, cj)
            parts = [first, G.seq(b, b + rlen - h)]
        elif kind == "backwards":
            b = a - int(np.exp(rng.uniform(np.log(200), np.log(5000))))
            parts = [first, G.seq(b, b + rlen - h)]
        else:
            h1 = rlen // 3 + int(rng.integers(-4, 5)); h2 = rlen // 3 + int(rng.integers(-4, 5))
            _, b = _pos(rng, G, 10, rlen + 10); _, c = _pos(rng, G, 10, rlen + 10)
            second = G.seq(b, b + h2)
            parts = [G.seq(a, a + h1), rc(second) if rng.random() < 0.5 else second, G.seq(c, c + rlen - h1 - h2)]
            h = h1
        ev = np.concatenate(parts)
        m1, m2, who = _with_mate(rng, G, ev, a, a + h, rlen)
        return m1, m2, dict(event_mate=who, join=h)
    return f


def _across_boundary(rng, G, rlen, k):
    kk = int(rng.integers(10, rlen - 10 + 1))
    n_chr = len(G.lo)
    if k % 2 == 0 and n_chr > 1:                     # contiguous text across the seam between two chromosomes
        c = 1 + int(rng.integers(0, n_chr - 1))
        p = int(G.lo[c])
        if G.hi[c] - p < rlen + 700 or p - G.lo[c - 1] < rlen + 700:
            raise _Skip
        ev = G.asc[p - kk:p - kk + rlen]
        gap = int(rng.integers(150, 301))
        if rng.random() < 0.5:
            m1, m2, who = _orient(rng, ev, G.seq(p - kk + rlen + gap, p - kk + 2 * rlen + gap), True)
        else:
            m1, m2, who = _orient(rng, G.seq(p - kk - gap - rlen, p - kk - gap), ev, False)
        return m1, m2, dict(event_mate=who, seam="chromosomes", before=kk)
    # the seam of the doubled text: the end of the forward strand, then the start of the reverse strand (the reverse complement of the same end)
    T = G.total
    ev = np.concatenate([G.asc[T - kk:T], rc(G.asc[T - (rlen - kk):T])])
    if k % 4 == 1:                                   # and the text's own two ends: the reverse strand's last bases, then the forward strand's first
        ev = np.concatenate([rc(G.asc[0:kk]), G.asc[0:rlen - kk]])
        gap = int(rng.integers(150, 301))
        m1, m2, who = _orient(rng, ev, G.seq(rlen + gap, 2 * rlen + gap), True)
        return m1, m2, dict(event_mate=who, seam="text ends", before=kk)
    gap = int(rng.integers(150, 301))
    m1, m2, who = _orient(rng, G.seq(T - kk - gap - rlen, T - kk - gap), ev, False)
    return m1, m2, dict(event_mate=who, seam="strands", before=kk)


def _plain_pair(kind):
    def f(rng, G, rlen, k):
        ci, a = _pos(rng, G, 400, 2 * rlen + 800)
        b = a + int(rng.integers(150, 301)) + rlen
        L = G.seq(a, a + rlen)
        info = {}
        if kind == "same_strand":
            R = G.seq(b, b + rlen)
            m1, m2 = (L, R) if k % 2 else (rc(R), rc(L))
        elif kind == "outie":
            R = G.seq(b, b + rlen)
            m1, m2 = (rc(L), R) if k % 2 else (R, rc(L))
        elif kind == "contained":
            n2 = int(rng.integers(40, rlen - 10)); o = int(rng.integers(0, rlen - n2 + 1))
            m1, m2, _ = _orient(rng, L, G.seq(a + o, a + o + n2), True) if k % 2 else (L, rc(G.seq(a + o, a + o + n2)), 0)
        elif kind == "dovetail":
            d = int(rng.integers(5, 61))
            m1, m2 = L, rc(G.seq(a - d, a - d + rlen))
            if k % 2: m1, m2 = m2, m1
        elif kind == "identical_mates":
            m1, m2 = (L, rc(L)) if k % 2 else (L, L.copy())
        elif kind == "other_chromosome":
            cj = (ci + 1 + int(rng.integers(0, max(1, len(G.lo) - 1)))) % len(G.lo)
            _, b = _pos(rng, G, 10, rlen + 10, cj)
            m1, m2, _ = _orient(rng, L, G.seq(b, b + rlen), True)
        elif kind == "far":
            want = (2000, 20000, 600000)[k % 3]      # (600 kb is beyond max_intron's default of 500 kb, but max_intron does not limit a pair's distance: mates pair while mate 2's
                                                     # candidate lies less than 2 000 000 bases downstream of mate 1's, Mapping.cpp:420-429 -- so all three distances pair)
            ci = int(np.argmax(G.hi - G.lo))
            room = int(G.hi[ci] - G.lo[ci]) - 2 * rlen - 40
            dist = min(want, room)                   # a genome whose longest chromosome is shorter than the distance: as far as it goes.  The golden genomes' longest chromosomes
                                                     # are 300 kb and 250 kb, so the committed sets hold 2 kb, 20 kb and about 299.8 kb / 249.5 kb.  A pair beyond the reach of
                                                     # 2 000 000 needs a chromosome longer than that (tests/threshold_inputs.py, ladder E); pair_other_chromosome is these sets' unpairable case
            a = int(rng.integers(G.lo[ci] + 10, G.hi[ci] - dist - 2 * rlen - 10 + 1))
            m1, m2, _ = _orient(rng, G.seq(a, a + rlen), G.seq(a + rlen + dist, a + 2 * rlen + dist), True)
            info = dict(distance=dist)
        elif kind == "mate_noise":
            m1, m2 = L, _rand(rng, rlen)
        elif kind == "swapped_files":
            R = G.seq(b, b + rlen)
            m1, m2 = rc(R), L
        else:
            raise ValueError(kind)
        return m1, m2, dict(event_mate=2, **info)
    return f


def _pair_mate_high_copy(rng, G, rlen, k):
    s, l = G.family_runs(101, 1 << 30, 20)
    if not len(s):
        raise _Skip
    i = int(rng.integers(0, len(s)))
    a = int(s[i]) - max(0, (rlen - int(l[i]) - 31) // 2)       # the family's copy in the middle of the read
    gap = int(rng.integers(150, 301))
    rep = G.seq(a, a + rlen)
    if k % 2:
        m1, m2, who = _orient(rng, rep, G.seq(a + rlen + gap, a + 2 * rlen + gap), True)
    else:
        m1, m2, who = _orient(rng, G.seq(a - gap - rlen, a - gap), rep, False)
    return m1, m2, dict(event_mate=who)


def _pair_both_multi(rng, G, rlen, k):
    s, l = G.family_runs(2, 40, 90)
    if not len(s):
        raise _Skip
    i = int(rng.integers(0, len(s)))
    a = int(s[i]); e = a + int(l[i]) + 31           # the copy of the family is text [a, e)
    n = rlen if e - a >= rlen + 20 else (e - a) * 2 // 3         # (a copy shorter than the read: both mates shorter, still inside it)
    m1, m2, _ = _orient(rng, G.seq(a, a + n), G.seq(e - n, e), True)
    return m1, m2, dict(event_mate=2)


def _pair_unequal_length(rng, G, rlen, k):
    short = (50,) if rlen >= 200 else (36, 14)
    n2 = short[k % len(short)]
    _, a = _pos(rng, G, 400, 2 * rlen + 800)
    b = a + rlen + int(rng.integers(150, 301))
    L, R = G.seq(a, a + rlen), G.seq(b, b + n2)
    if (k // 2) % 2:
        L, R = G.seq(a, a + n2), G.seq(b, b + rlen)
    m1, m2, _ = _orient(rng, L, R, True)
    return m1, m2, dict(event_mate=2, lengths=(len(m1), len(m2)))


NEEDS_REPEATS = ("pair_mate_high_copy", "pair_both_multi")        # the classes a genome without such families (synth.make_genome at repeat_scale 0) cannot serve


def class_names(rlen):
    """the names of the classes for reads of rlen bases, in the order `make` returns them"""
    return list(_classes(rlen))


def _classes(rlen):
    c = {"two_junctions": _two_junctions}
    if rlen >= 200:
        c["three_junctions"] = _three_junctions
    c.update({"overhang": _overhang, "junction_in_both_mates": _junction_in_both_mates, "del_4_30": _deletion(4, 30), "del_31_120": _deletion(31, 120),
              "ins_4_30": _insertion(4, 30)})
    if rlen >= 200:
        c["ins_31_80"] = _insertion(31, 80)
    c.update({"two_indels": _two_indels, "indel_near_end": _indel_near_end, "indel_beside_junction": _indel_beside_junction,
              "noise_island": _noise_island, "two_noise_islands": _two_noise_islands, "noise_head": _noise_end(True), "noise_tail": _noise_end(False),
              "tandem_dup_in_read": _tandem(True), "tandem_loss_in_read": _tandem(False),
              "chimera_other_strand": _chimera("other_strand"), "chimera_other_chromosome": _chimera("other_chromosome"),
              "chimera_backwards": _chimera("backwards"), "chimera_three_parts": _chimera("three_parts"),
              "across_chromosome_boundary": _across_boundary})
    for kind in ("same_strand", "outie", "contained", "dovetail", "identical_mates", "other_chromosome", "far", "mate_noise"):
        c["pair_" + kind] = _plain_pair(kind)
    c.update({"pair_mate_high_copy": _pair_mate_high_copy, "pair_both_multi": _pair_both_multi, "pair_unequal_length": _pair_unequal_length,
              "pair_swapped_files": _plain_pair("swapped_files")})
    return c


def make_with_info(genome, seed: int, rlen: int = 101, n_per_class: int = 100, only=None):
    """-> ({class: [(mate 1 bytes, mate 2 bytes)]}, {class: [what was planted, per pair]})"""
    if rlen < 100:
        raise ValueError("the classes need reads of at least 100 bases")
    G = _G(genome)
    pairs, infos = {}, {}
    for ci, (name, fn) in enumerate(_classes(rlen).items()):
        if only is not None and name not in only:
            continue
        rng = np.random.default_rng([seed, rlen, ci])
        out, inf, tries = [], [], 0
        while len(out) < n_per_class and tries < 60 * n_per_class:
            tries += 1
            try:
                m1, m2, info = fn(rng, G, rlen, len(out))
            except _Skip:
                continue
            info["sub"] = name in SPLICED_AND_INDEL and bool(rng.random() < 0.5)
            if info["sub"]:
                m1, m2 = _substitute(rng, m1), _substitute(rng, m2)
            out.append((np.ascontiguousarray(m1).tobytes(), np.ascontiguousarray(m2).tobytes())); inf.append(info)
        if out:                                      # (a genome without what a class needs -- a single chromosome, no repeat family -- has no such class)
            pairs[name], infos[name] = out, inf
    return pairs, infos


def make(genome, seed: int, rlen: int = 101, n_per_class: int = 100, only=None):
    return make_with_info(genome, seed, rlen, n_per_class, only)[0]


def as_reads(pairs):
    """[(mate 1, mate 2 as sequenced)] -> the batch's reads: mate 1, then mate 2 reverse-complemented as the loader does"""
    out = []
    for m1, m2 in pairs:
        out.append(m1)
        out.append(_COMP[np.frombuffer(m2, np.uint8)[::-1]].tobytes())
    return out


def all_pairs(classes):
    """every class's pairs in one list, in class order, and the class of each pair"""
    pairs, names = [], []
    for name, ps in classes.items():
        pairs += ps; names += [name] * len(ps)
    return pairs, names


def write_fastq(path1, path2, pairs):
    with open(path1, "w") as f1, open(path2, "w") as f2:
        for i, (m1, m2) in enumerate(pairs):
            f1.write("@p%d\n%s\n+\n%s\n" % (i, m1.decode(), "I" * len(m1)))
            f2.write("@p%d\n%s\n+\n%s\n" % (i, m2.decode(), "I" * len(m2)))


def digest(classes) -> str:
    import hashlib
    h = hashlib.sha256()
    for name, ps in classes.items():
        h.update(name.encode())
        for m1, m2 in ps:
            h.update(m1 + b"/" + m2 + b"\n")
    return h.hexdigest()
