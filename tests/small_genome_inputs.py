"""Inputs of the small-genome parity tests (CPU: tests/test_small_genomes_oracle.py, GPU: tests/test_gpu_small_genomes.py, fixtures:
tests/golden/make_small_genomes.py): genomes of 32 b to 130 kb at the seams of the index -- one or two Occ blocks, a 64-symbol window that
fits a strand never / once / twice, the builder's 4096-pair tile, the prefix table's K going 8 -> 9 -> 10 -- and about 500 reads per genome
of the kinds a phage, plasmid or amplicon job sees: reads longer than a contig or than the whole text, reads over contig seams and over the
junction of a circular genome, long gaps whose re-seeding windows the genome clips.  Everything is a pure function of the genome's name."""
from __future__ import annotations

import hashlib
import os
import numpy as np
from dart_amd import synth, host

# forward-strand lengths; a list = several contigs
GENOMES = [
    ("g32", [32]),                          # the smallest the builder accepts; one Occ block; no fast comparison at all
    ("g63", [63]), ("g64", [64]), ("g65", [65]),        # a 64-symbol window fits a strand never / exactly once / twice
    ("g128", [128]), ("g129", [129]),       # text of exactly two Occ blocks / one symbol more
    ("g2047", [2047]), ("g2048", [2048]),   # N = n + 1 of 4095 / 4097 around the builder's 4096 tile
    ("g5386", [5386]), ("g16569", [16569]),             # phage and mitochondrion size
    ("g32767", [32767]), ("g32768", [32768]), ("g32769", [32769]),      # seq_len around 4^8: K goes 8 -> 9
    ("g131072", [131072]), ("g131073", [131073]),       # seq_len around 4^9: K goes 9 -> 10
    ("c5", [300, 64, 33, 1000, 129]),       # contigs shorter than a read or a seed
    ("plasmids", [4361, 2686, 48502]),
]
NAMES = [n for n, _ in GENOMES]
LENGTHS = dict(GENOMES)
READ_LENGTHS = (20, 36, 50, 76, 101, 150, 250)
SE_FLAGS = ([], ["-mis", "5"], ["-mis", "5", "-m", "-max_dup", "1000"])
PE_FLAGS = (["-mis", "5"],)
LONG_GAP_MIN = 4096                         # genomes from this size on get long-gap reads: re-seeding and junctions must run on them
INDEX_EXT = ("amb", "ann", "bwt", "pac", "sa")

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = np.full(256, ord("N"), np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    _COMP[_a] = _b


def l_pac(name: str) -> int:
    return sum(LENGTHS[name])


def expected_k(name: str) -> int:
    """the prefix table's K: the smallest K in 8..16 with 4^K >= seq_len = 2 l_pac"""
    K = 8
    while K < 16 and 4 ** K < 2 * l_pac(name):
        K += 1
    return K


def has_pairs(name: str) -> bool:
    """a pair of 36-base mates needs a 41-base fragment inside one contig"""
    return max(LENGTHS[name]) >= 41


def _seed(name: str, salt: int) -> int:
    return 52000 + 10 * NAMES.index(name) + salt


def revcomp(s: bytes) -> bytes:
    return _COMP[np.frombuffer(s, np.uint8)[::-1]].tobytes()


_genomes = {}


def make_genome(name: str) -> synth.Genome:
    """random codes; a tandem repeat (unit 11-47 bases, 4-8 copies) where l_pac >= 1000; from LONG_GAP_MIN on 40 exon chains (60 bases, a
    skip of 300 .. l_pac / 2, 60 bases; every second one with a 24-base exon in the middle, which no 16-base seed finds once it carries
    a substitution), half of the skips with GT..AG at their ends; one exact 60-base repeat where the genome has room.  The chains are
    kept in g.long_gaps as lists of (start, length); g.introns holds (start, length, has_motif) of every skip."""
    if name in _genomes:
        return _genomes[name]
    lens = LENGTHS[name]
    rng = np.random.default_rng(_seed(name, 0))
    total = sum(lens)
    codes = rng.integers(0, 4, size=total, dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    if total >= 1000:
        u = rng.integers(0, 4, size=int(rng.integers(11, 48)), dtype=np.uint8)
        k = int(rng.integers(4, 9))
        p = int(rng.integers(0, total - len(u) * k))
        codes[p:p + len(u) * k] = np.tile(u, k)
    chains, introns = [], []
    if total >= LONG_GAP_MIN:
        big = [i for i, l in enumerate(lens) if l >= 2 * 300 + 150]
        for j in range(40):
            ci = big[int(rng.integers(0, len(big)))]
            co, cl = int(offs[ci]), int(lens[ci])
            if j % 2 == 0:
                skips = [int(rng.integers(300, min(total // 2, cl - 120) + 1))]
                exons = [60, 60]
            else:
                hi = min(total // 2, (cl - 144) // 2)
                skips = [int(rng.integers(300, hi + 1)), int(rng.integers(300, hi + 1))]
                exons = [60, 24, 60]
            span = sum(skips) + sum(exons)
            a = co + int(rng.integers(0, cl - span + 1))
            chain = []
            for e, ex in enumerate(exons):
                chain.append((a, ex))
                a += ex
                if e < len(skips):
                    motif = int(rng.random() < 0.5)
                    if motif:
                        if rng.random() < 0.5:
                            codes[a:a + 2] = (2, 3); codes[a + skips[e] - 2:a + skips[e]] = (0, 2)        # GT..AG
                        else:
                            codes[a:a + 2] = (1, 3); codes[a + skips[e] - 2:a + skips[e]] = (0, 1)        # CT..AC: GT..AG of the other strand
                    introns.append((a, skips[e], motif))
                    a += skips[e]
            chains.append(chain)
    if total >= 200:
        a = int(rng.integers(0, total // 2 - 60)); b = int(rng.integers(total // 2, total - 60))
        codes[b:b + 60] = codes[a:a + 60]
    g = synth.Genome(["s%d" % (i + 1) for i in range(len(lens))], lens, codes, np.asarray(introns, np.int64).reshape(-1, 3))
    g.long_gaps = chains
    _genomes[name] = g
    return g


def codes_sha256(name: str) -> str:
    return hashlib.sha256(make_genome(name).codes.tobytes()).hexdigest()


def _lengths_for(total: int):
    return sorted({min(L, total - 3) for L in READ_LENGTHS})


def _mutate(rng, kind: str, text: np.ndarray, p: int, L: int) -> bytes:
    """one read of `kind` whose source starts at p of the ASCII forward text"""
    total = len(text)
    if kind == "del2":                                   # L + 2 bases of the genome (or what it has) without two in the middle
        src = text[p:p + min(L + 2, total - p)].copy()
        q = int(rng.integers(len(src) // 3, 2 * len(src) // 3))
        return np.concatenate([src[:q], src[q + 2:]]).tobytes()
    if kind == "ins2":
        src = text[p:p + L - 2]
        q = int(rng.integers(len(src) // 3, 2 * len(src) // 3 + 1))
        return np.concatenate([src[:q], _ACGT[rng.integers(0, 4, 2)], src[q:]]).tobytes()
    src = text[p:p + L].copy()
    if kind == "sub":
        q = int(rng.integers(0, L))
        src[q] = _ACGT[(int(np.nonzero(_ACGT == src[q])[0][0]) + int(rng.integers(1, 4))) & 3]
    elif kind == "tail30":
        src = np.concatenate([src, _ACGT[rng.integers(0, 4, 30)]])
    return src.tobytes()


def _chain_read(text: np.ndarray, chain, rng) -> bytes:
    parts = [text[a:a + l].copy() for a, l in chain]
    if len(parts) == 3:                                  # the middle exon: 11 + 12 matching bases around a substitution
        parts[1][11] = _ACGT[(int(np.nonzero(_ACGT == parts[1][11])[0][0]) + int(rng.integers(1, 4))) & 3]
    return np.concatenate(parts).tobytes()


_single = {}


def single_reads(name: str):
    """-> list of bytes: about 500 reads, half from each strand"""
    if name in _single:
        return _single[name]
    g = make_genome(name)
    rng = np.random.default_rng(_seed(name, 1))
    text = g.ascii()
    total = g.total
    Ls = _lengths_for(total)
    out = []
    for kind in ("exact", "sub", "del2", "ins2", "wrap", "tail30"):
        for k in range(70):
            L = Ls[k % len(Ls)]
            if kind == "wrap":                           # the junction of a circular genome: the text's end, then its start
                a = int(rng.integers(L // 4, 3 * L // 4 + 1))
                out.append(np.concatenate([text[total - a:], text[:L - a]]).tobytes())
            else:
                out.append(_mutate(rng, kind, text, int(rng.integers(0, total - L + 1)), L))
    ends = np.cumsum(g.lengths)
    for b in ends[:-1].tolist():                         # reads centred on every contig seam
        for L in (40, 100):
            out.append(text[max(0, b - L // 2):min(total, b + L // 2)].tobytes())
            out.append(text[max(0, b - L // 2 + 3):min(total, b + L // 2 + 3)].tobytes())
    for off, ln in zip(g.offsets[:-1].tolist(), g.lengths[:-1].tolist()):
        if ln <= 900:                                    # a whole contig and its neighbour's first bases (reads hold up to 1000 bases)
            out.append(text[off:off + ln + 20].tobytes()); out.append(text[off:off + ln + 20].tobytes())
    for chain in g.long_gaps:
        out.append(_chain_read(text, chain, rng))
    out.append(b"N" * 50); out.append(b"N" * 50)
    p = int(rng.integers(0, total - 12))
    out.append(text[p:p + 12].tobytes()); out.append(text[p:p + 12].tobytes())          # shorter than a seed
    out = [revcomp(s) if i % 2 else s for i, s in enumerate(out)]
    _single[name] = out
    return out


_paired = {}


def paired_reads(name: str):
    """-> (mate 1 list, mate 2 list) as sequenced (mate 2 not yet reverse-complemented), or None where no 41-base fragment fits a contig"""
    if not has_pairs(name):
        return None
    if name in _paired:
        return _paired[name]
    g = make_genome(name)
    rng = np.random.default_rng(_seed(name, 2))
    text = g.ascii()
    total = g.total
    lens, offs = g.lengths.tolist(), g.offsets.tolist()
    Ls = [L for L in READ_LENGTHS if L + 5 <= max(lens)]
    frags = []                                           # (mate 1 source, mate 2 source): both in the fragment's direction

    def fragment(L):
        ci = int(rng.choice([i for i, l in enumerate(lens) if l >= L + 5]))
        flen = int(rng.integers(L + 5, min(lens[ci], L + 5 + 300) + 1))
        s = offs[ci] + int(rng.integers(0, lens[ci] - flen + 1))
        return s, flen

    for kind in ("exact", "sub", "del2", "ins2", "wrap", "tail30"):
        for k in range(36):
            L = Ls[k % len(Ls)]
            s, flen = fragment(L)
            if kind == "wrap":
                flen = min(flen, total)
                a = int(rng.integers(L // 4, flen - L // 4))
                frag = np.concatenate([text[total - a:], text[:flen - a]])
                frags.append((frag[:L].tobytes(), frag[flen - L:].tobytes()))
            elif kind == "exact":
                frags.append((text[s:s + L].tobytes(), text[s + flen - L:s + flen].tobytes()))
            elif kind == "tail30":
                frags.append((text[s:s + L].tobytes(), _mutate(rng, kind, text, s + flen - L, L)))
            elif kind == "sub":
                frags.append((_mutate(rng, kind, text, s, L), _mutate(rng, kind, text, s + flen - L, L)))
            else:
                frags.append((_mutate(rng, kind, text, s, min(L, flen - 2)), text[s + flen - L:s + flen].tobytes()))
    ends = np.cumsum(g.lengths)
    for b in ends[:-1].tolist():                         # fragments over every contig seam
        for L in (36, 50):
            lo, hi = max(0, b - L - 10), min(total, b + L + 10)
            if hi - lo >= L + 5:
                frags.append((text[lo:lo + L].tobytes(), text[hi - L:hi].tobytes()))
                frags.append((text[b - L // 2:b - L // 2 + L].tobytes(), text[hi - L:hi].tobytes()))
    cend = {int(o): int(o + l) for o, l in zip(offs, lens)}
    for chain in g.long_gaps:                            # mate 1 over the long gaps, mate 2 behind the last exon
        a, l = chain[-1]
        ce = max(e for o, e in cend.items() if o <= a)
        if a + l + 20 + 60 <= ce:
            frags.append((_chain_read(text, chain, rng), text[a + l + 20:a + l + 80].tobytes()))
    s, flen = fragment(36)
    frags.append((b"N" * 36, text[s + flen - 36:s + flen].tobytes()))
    frags.append((text[s:s + 36].tobytes(), text[s + flen - 12:s + flen].tobytes()))             # a mate shorter than a seed
    m1, m2 = [], []
    for i, (a, b) in enumerate(frags):                   # every second fragment comes from the reverse strand
        if i % 2:
            m1.append(revcomp(b)); m2.append(a)
        else:
            m1.append(a); m2.append(revcomp(b))
    _paired[name] = (m1, m2)
    return m1, m2


def stored_pairs(m1, m2):
    """the batch as the loader stores it: mate 1, then mate 2 reverse-complemented (GetData.cpp:157-162), alternating"""
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
    """[(run label, paired, flags of the mapping)]: the label is the key of tests/golden/small_genomes.json"""
    out = [("%s se: %s" % (name, " ".join(f)), False, list(f)) for f in SE_FLAGS]
    if has_pairs(name):
        out += [("%s pe: %s" % (name, " ".join(f)), True, list(f)) for f in PE_FLAGS]
    return out


def write_inputs(name: str, d: str):
    """d/g.fa, d/a.fq (single-end), d/p1.fq + d/p2.fq (pairs) -> the file arguments of the single-end and of the paired run"""
    os.makedirs(d, exist_ok=True)
    make_genome(name).write_fasta(os.path.join(d, "g.fa"))
    write_fastq(os.path.join(d, "a.fq"), single_reads(name))
    pe = paired_reads(name)
    if pe:
        write_fastq(os.path.join(d, "p1.fq"), pe[0], 1); write_fastq(os.path.join(d, "p2.fq"), pe[1], 2)
    return ["-f", "a.fq"], (["-f", "p1.fq", "-f2", "p2.fq"] if pe else None)


def batch(name: str, paired: bool):
    """(seq_off, rlen, flat) of a run's reads, as host.pack_reads gives them"""
    return host.pack_reads(stored_pairs(*paired_reads(name)) if paired else single_reads(name))
