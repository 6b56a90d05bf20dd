"""Helpers of the transcript-expression tests: the sequential Python twin of the definition in dart_amd/csrc/dg_txquant.h (compatibility unit by unit over the
(reads, reports, cigar) record arrays, the class dictionary, the EM in Python ints and floats one operation at a time, the text), a second, independent
statement of compatibility (a per-base painter of a transcript's exonic bases and its intron set), annotation builders and the native program
tests/native/txquant_checks.hip.  The definition is the header's comment: no RSEM, Salmon or kallisto exists where these tests run."""
from __future__ import annotations

import math, os, random, struct, subprocess
import numpy as np
import common
import genecount_inputs as gci
from dart_amd import host

M, I, D, N, S, H, P, EQ, X = range(9)
UNMAPPED, MULTI, INCOMPAT, COUNTED = range(4)
F = 1 << 20
Records = gci.Records


# ---- annotations: a list of transcripts (chr, strand, [(start, end), ...]) ----
def annot_arrays(transcripts):
    """-> (RNA_TX array, RNA_EXON array), the exons in the order given"""
    tx = np.zeros(len(transcripts), host.RNA_TX); ex = []
    for t, (c, st, exons) in enumerate(transcripts):
        tx[t] = (c, st, 0, 0, 0, len(exons), len(ex))
        ex += [(int(s), int(e)) for s, e in exons]
    return tx, np.array(ex, host.RNA_EXON) if ex else np.zeros(0, host.RNA_EXON)


def merged(exons):
    out = []
    for s, e in sorted((int(s), int(e)) for s, e in exons):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return [tuple(x) for x in out]


def lengths(transcripts):
    return [sum(e - s for s, e in merged(ex)) for _, _, ex in transcripts]


# ---- a read ----
def pieces(rep, cigar, n_chr: int):
    """-> (pieces [(start, end)], block span (lo, hi) or None); no blocks: ([], None)"""
    pos, c = int(rep["pos"]), int(rep["chr"])
    if pos < 1 or not 0 <= c < n_chr:
        return [], None
    out, cur, p, lo, hi = [], None, pos - 1, None, None
    for w in cigar[int(rep["cigar_off"]):int(rep["cigar_off"]) + int(rep["n_cigar"])].tolist():
        op, ln = w & 15, w >> 4
        if op in (M, EQ, X):
            if ln:
                cur = [p, p + ln] if cur is None else [cur[0], p + ln]
                lo = p if lo is None else min(lo, p); hi = p + ln if hi is None else max(hi, p + ln)
            p += ln
        elif op == D:
            p += ln
        elif op == N:
            p += ln
            if cur is not None:
                out.append(tuple(cur)); cur = None
    if cur is not None:
        out.append(tuple(cur))
    return out, (None if lo is None else (lo, hi))


def strand_of(rep) -> int:
    return (int(rep["flag"]) >> 4 & 1) ^ (int(rep["flag"]) >> 7 & 1)


def compatible(pcs, mex) -> bool:
    """the definition: pieces against a transcript's merged exons"""
    if not pcs:
        return False
    prev = None
    for ps, pe in pcs:
        e = next((k for k, (s, t) in enumerate(mex) if s <= ps < t), None)
        if e is None or pe > mex[e][1]:
            return False
        if prev is not None and not (prev[1] == mex[prev[0]][1] and e == prev[0] + 1 and ps == mex[e][0]):
            return False
        prev = (e, pe)
    return True


def compatible_painted(pcs, exons) -> bool:
    """the independent statement: the transcript's exonic bases painted exon by exon (as given, unmerged) and its introns read off the painting: the read is
    compatible iff every base of its pieces is exonic, and every gap between two consecutive pieces is exactly one intron (a maximal run of unpainted bases
    with painted bases on either side)"""
    if not pcs:
        return False
    lo = min(min(s for s, _ in exons), min(s for s, _ in pcs)); hi = max(max(e for _, e in exons), max(e for _, e in pcs))
    if hi - lo > 1 << 22:          # far-apart coordinates: paint only around what matters
        return compatible(pcs, merged(exons))
    paint = np.zeros(hi - lo + 2, bool)
    for s, e in exons:
        paint[s - lo + 1:e - lo + 1] = True
    edge = np.flatnonzero(paint[1:] != paint[:-1])          # boundaries: painted runs are [edge[2k], edge[2k + 1])
    introns = {(int(edge[k]) + lo, int(edge[k + 1]) + lo) for k in range(1, len(edge) - 1, 2)}
    for s, e in pcs:
        if not paint[s - lo + 1:e - lo + 1].all():
            return False
    return all((a[1], b[0]) in introns for a, b in zip(pcs, pcs[1:]))


def toff(mex, g):
    before = 0
    for s, e in mex:
        if s <= g < e:
            return before + g - s
        before += e - s
    raise AssertionError("position outside the transcript")


# ---- a unit ----
def unit_outcome(transcripts, mexs, by_chr, n_chr, reads, reports, cigar, unit, n_pair_mode, min_mapq, strand_mode, check_painted=False):
    """-> (outcome, ids tuple, fl or None)"""
    al = [(k, gci.alignment(reads, reports, k, k < n_pair_mode)) for k in unit]
    al = [(k, a) for k, a in al if a is not None]
    if not al:
        return UNMAPPED, (), None
    if any(int(reads[k]["mapq"]) < min_mapq for k, _ in al):
        return MULTI, (), None
    cand = None
    spans = []
    for _, a in al:
        rep = reports[a]
        pcs, span = pieces(rep, cigar, n_chr)
        s = strand_of(rep)
        ok = set()
        for t in (by_chr.get(int(rep["chr"]), []) if pcs else []):
            st = transcripts[t][1]
            if (strand_mode == 1 and st != s) or (strand_mode == 2 and st == s):
                continue
            c = compatible(pcs, mexs[t])
            if check_painted:
                assert c == compatible_painted(pcs, transcripts[t][2]), (pcs, transcripts[t])
            if c:
                ok.add(t)
        cand = ok if cand is None else cand & ok
        spans.append(span)
    if not cand:
        return INCOMPAT, (), None
    ids = tuple(sorted(cand))
    fl = None
    if len(al) == 2:
        lo, hi = min(s[0] for s in spans), max(s[1] for s in spans)
        fl = toff(mexs[ids[0]], hi - 1) + 1 - toff(mexs[ids[0]], lo)
    return COUNTED, ids, fl


def twin(transcripts, n_chr, reads, reports, cigar, n_pair_mode, min_mapq, strand_mode=0, check_painted=False, want_units=False):
    """-> (classes {ids tuple: count}, words [8]) (and the per-unit outcomes)"""
    mexs = [merged(ex) for _, _, ex in transcripts]
    by_chr = {}
    for t, (c, _, _) in enumerate(transcripts):
        by_chr.setdefault(int(c), []).append(t)
    classes, words, units = {}, [0] * 8, []
    for unit in gci.units_of(len(reads), n_pair_mode):
        o, ids, fl = unit_outcome(transcripts, mexs, by_chr, n_chr, reads, reports, cigar, unit, n_pair_mode, min_mapq, strand_mode, check_painted)
        units.append((o, ids, fl))
        words[0] += 1; words[1 + o] += 1
        if o == COUNTED:
            classes[ids] = classes.get(ids, 0) + 1
        if fl is not None:
            words[5] += fl; words[6] += 1
    assert words[0] == sum(words[1:5])
    return (classes, words, units) if want_units else (classes, words)


def add_tables(a, b):
    ca, wa = a; cb, wb = b
    out = dict(ca)
    for k, v in cb.items():
        out[k] = out.get(k, 0) + v
    return out, [x + y for x, y in zip(wa, wb)]


def table_dict(off, ids, cnt):
    """a downloaded CSR table as the twin's dictionary; every list ascending, no list twice"""
    out = {}
    for i in range(len(cnt)):
        k = tuple(int(x) for x in ids[int(off[i]):int(off[i + 1])])
        assert k and all(a < b for a, b in zip(k, k[1:])) and k not in out, k
        out[k] = int(cnt[i])
    return out


def table_csr(classes):
    off, ids, cnt = [0], [], []
    for k, v in classes.items():
        ids += list(k); off.append(len(ids)); cnt.append(v)
    return np.array(off, np.uint64), np.array(ids, np.uint32), np.array(cnt, np.uint64)


# ---- the EM: Python ints and floats, one operation at a time ----
def eff_len(L: int, mean: int) -> int:
    return L - mean + 1 if L >= mean else L


def em(classes, words, L, frag_mean, max_rounds, strand_mode=0, want_trace=False, start=None):
    """-> the result words [n_tx + 16] (and S after every round); start: S to begin from instead of the definition's (a test's way into states the start
    values do not reach)"""
    n_tx = len(L)
    order = sorted(classes)
    Ntot = sum(classes.values())
    assert Ntot < 1 << 33
    active = sorted({t for k in classes for t in k})
    Mact = len(active)
    mean = words[5] // words[6] if words[6] else frag_mean
    eff = [eff_len(x, mean) for x in L]
    Sv = [0] * n_tx
    for t in active:
        Sv[t] = Ntot * F // Mact
    if start is not None:
        Sv = list(start)
    rounds, conv, trace = 0, (1 if Mact == 0 else 0), []
    while Mact and rounds < max_rounds:
        theta = []
        for t in range(n_tx):
            alpha = float(Sv[t]) / float(F)
            theta.append(alpha / float(eff[t]))
        new = [0] * n_tx
        for k in order:
            Dsum = 0.0
            for t in k:
                Dsum = Dsum + theta[t]
            if Dsum == 0.0:
                continue
            for t in k:
                q = theta[t] / Dsum
                x = float(classes[k]) * q
                y = x * 1048576.0
                new[t] += int(math.floor(y))
        conv = 1
        for t in range(n_tx):
            if new[t] >= F and 100 * abs(new[t] - Sv[t]) > new[t]:
                conv = 0
        Sv = new; rounds += 1; trace.append(list(Sv))
        if conv and rounds % 16 == 0:
            break
    res = Sv + [words[0], words[1], words[2], words[3], words[4], len(classes), sum(len(k) for k in classes), Mact, rounds, conv, words[5], words[6], mean, strand_mode, 0, 0]
    return (res, trace) if want_trace else res


WORD_NAMES = ["units", "unmapped", "multimapping", "incompatible", "counted", "classes", "members", "active", "rounds", "converged", "fl_sum", "fl_n", "frag_mean",
              "strand_mode", "reserved0", "reserved1"]


def text(res, L, names) -> bytes:
    n_tx = len(L)
    w = res[n_tx:]
    out = ["# %s\t%d\n" % (n, v) for n, v in zip(WORD_NAMES, w)]
    out.append("transcript_id\tlength\teff_length\test_counts\ttpm\n")
    eff = [eff_len(x, w[12]) for x in L]
    rate = [res[t] * 1024 // eff[t] for t in range(n_tx)]
    R = sum(rate)
    for t in range(n_tx):
        est = res[t] * 1000 // F
        tpm = rate[t] * 10 ** 9 // R if R else 0
        out.append("%s\t%d\t%d\t%d.%03d\t%d.%03d\n" % (names[t], L[t], eff[t], est // 1000, est % 1000, tpm // 1000, tpm % 1000))
    return "".join(out).encode()


# ---- annotation builders ----
def locus_isoforms(chrom, strand, exons, rng=None):
    """the three isoforms of a multi-exon locus: full, one exon skipped (an inner one where there is one), one intron retained"""
    out = [(chrom, strand, list(exons))]
    if len(exons) >= 2:
        k = (rng.randrange(1, len(exons) - 1) if rng else 1) if len(exons) >= 3 else (rng.randrange(2) if rng else 0)
        out.append((chrom, strand, exons[:k] + exons[k + 1:]))
        j = rng.randrange(len(exons) - 1) if rng else 0
        out.append((chrom, strand, exons[:j] + [(exons[j][0], exons[j + 1][1])] + exons[j + 2:]))
    return out


def case_annotation(case, seed):
    """transcripts over a golden case's genome whose introns are the genome's planted introns (which are long and lie across one another, so the loci do too):
    an intron and up to three that begin shortly behind its end make a locus of two to five exons on a random strand, with three isoforms (full, one exon
    skipped, one intron retained) whose exons are given in shuffled order; over some loci's tails a single-exon transcript on a strand of its own; and
    single-exon transcripts over stretches of the rest of the chromosome -> the transcripts"""
    g = case["genome"]
    rng = random.Random(seed)
    lens = [int(x) for x in g.lengths]
    cuts = [[] for _ in lens]
    for s, ln, _ in np.asarray(g.introns).tolist():
        c = int(np.searchsorted(g.offsets, s, side="right")) - 1
        cuts[c].append((int(s - g.offsets[c]), int(s - g.offsets[c] + ln)))
    out = []
    for c, L in enumerate(lens):
        iv = sorted(set(cuts[c])); used = set()
        for i in range(len(iv)):
            if i in used:
                continue
            grp = [i]
            while len(grp) < 4:
                nxt = [j for j in range(len(iv)) if j not in used and j not in grp and iv[grp[-1]][1] + 60 < iv[j][0] < iv[grp[-1]][1] + 700]
                if not nxt or rng.random() < 0.2:
                    break
                grp.append(rng.choice(nxt))
            used.update(grp)
            first = max(0, iv[grp[0]][0] - rng.randrange(80, 400)); last = min(L - 1, iv[grp[-1]][1] + rng.randrange(80, 400))
            bounds = [first] + [x for j in grp for x in iv[j]] + [last]
            exons = [(bounds[2 * j], bounds[2 * j + 1]) for j in range(len(grp) + 1)]
            if any(s >= e for s, e in exons):
                continue
            strand = rng.randrange(2)
            for iso in locus_isoforms(c, strand, exons, rng):
                ex = list(iso[2]); rng.shuffle(ex)
                out.append((iso[0], iso[1], ex))
            if rng.random() < 0.4 and last - iv[grp[-1]][1] > 60:
                out.append((c, rng.randrange(2), [(last - rng.randrange(20, last - iv[grp[-1]][1] - 20), min(L - 1, last + rng.randrange(100, 500)))]))
        at = rng.randrange(50, 500)
        while at < L - 3500:
            ln = rng.randrange(500, 3000)
            if rng.random() < 0.5:
                out.append((c, rng.randrange(2), [(at, at + ln)]))
            at += ln + rng.randrange(50, 1500)
    return out


def random_annotation(rng, lengths, n_loci=12):
    """loci of one to five exons with up to four isoforms each (subsets of the exons, retained introns, alternative ends), some loci overlapping, some exons
    touching or overlapping inside a transcript -> the transcripts"""
    out = []
    for c, L in enumerate(lengths):
        at = rng.randrange(20, 200)
        for _ in range(n_loci):
            n_ex = rng.randrange(1, 6); exons = []; p = at
            for _ in range(n_ex):
                e = p + rng.randrange(15, 120); exons.append((p, e)); p = e + rng.randrange(10, 90)
            if p >= L:
                break
            strand = rng.randrange(2)
            isos = locus_isoforms(c, strand, exons, rng)
            if rng.random() < 0.5 and len(exons) >= 2:      # an alternative end: the last exon shorter or longer
                alt = exons[:-1] + [(exons[-1][0], exons[-1][1] + rng.randrange(-10, 30))]
                isos.append((c, rng.randrange(2), alt))
            if rng.random() < 0.4:                          # touching and overlapping pieces of one exon
                s, e = exons[0]; m = (s + e) // 2
                isos.append((c, strand, [(s, m), (m, e)] + exons[1:] + [(s + 2, m + 3)]))
            for iso in isos:
                ex = list(iso[2]); rng.shuffle(ex); out.append((iso[0], iso[1], ex))
            at = p - rng.randrange(0, 60) if rng.random() < 0.3 else p + rng.randrange(20, 300)
    return out


def random_units(rng, transcripts, n_chr, n_units, pair_frac=0.5):
    """units drawn from the transcripts (a fragment of a transcript, cut into blocks at its introns), some moved by a base, some with I, D, S ops, some
    unaligned, some with a low MAPQ, pairs first -> (reads, reports, cigar, n_pair_mode)"""
    mexs = [merged(ex) for _, _, ex in transcripts]

    def fragment(t, a, b):
        """transcript offsets [a, b) as (pos 1-based, ops)"""
        ops, pos, before, last = [], None, 0, None
        for s, e in mexs[t]:
            lo, hi = max(a - before, 0) + s, min(b - before, e - s) + s
            if lo < hi:
                if pos is None:
                    pos = lo + 1
                else:
                    ops.append((lo - last, N))
                ops.append((hi - lo, M)); last = hi
            before += e - s
        return pos, ops

    def one_read(rec, t, a, b, flag, mapq):
        kind = rng.random()
        if kind < 0.08:
            rec.read(); return
        pos, ops = fragment(t, a, b)
        if kind < 0.2:
            pos += rng.choice((-1, 1))
        elif kind < 0.3 and ops[0][0] > 6:
            ln = ops[0][0]; ops = [(3, S), (ln - 4, M), (2, I), (1, D), (3, M)] + ops[1:]
        elif kind < 0.35:
            ops = [(0, M), (0, N)] + ops + [(5, H)]
        rec.read(reports=[(transcripts[t][0], pos, flag, ops, 100)], mapq=mapq)

    rec = Records()
    n_pairs = int(n_units * pair_frac)
    L = [sum(e - s for s, e in m) for m in mexs]
    for u in range(n_units):
        t = rng.randrange(len(transcripts))
        mapq = 50 if rng.random() > 0.1 else rng.choice((0, 1, 3))
        if u < n_pairs:
            a = rng.randrange(0, max(L[t] - 10, 1)); b = min(L[t], a + rng.randrange(20, 200))
            rl = max(5, min(40, (b - a) // 2 + 1))
            first_rev = rng.random() < 0.5
            one_read(rec, t, a, min(a + rl, b), 0x41 | (0x10 if first_rev else 0x20), mapq)
            t2 = t if rng.random() > 0.1 else rng.randrange(len(transcripts))
            one_read(rec, t2, max(min(b, L[t2]) - rl, 0), min(b, L[t2]), 0x81 | (0x20 if first_rev else 0x10), mapq)
        else:
            a = rng.randrange(0, max(L[t] - 5, 1)); b = min(L[t], a + rng.randrange(5, 120))
            one_read(rec, t, a, b, 0x10 if rng.random() < 0.5 else 0, mapq)
    rd, rp, cg = rec.arrays()
    return rd, rp, cg, 2 * n_pairs


def ladder(n_tx: int):
    """transcript t: one plus-strand exon [100 + 20 t, 110 + 20 t) on chromosome 0 -> (RNA_TX, RNA_EXON)"""
    tx = np.zeros(n_tx, host.RNA_TX); ex = np.zeros(n_tx, host.RNA_EXON)
    tx["n_exons"] = 1; tx["first_exon"] = np.arange(n_tx)
    ex["start"] = 100 + 20 * np.arange(n_tx, dtype=np.int64); ex["end"] = ex["start"] + 10
    return tx, ex


def ladder_units(ts):
    """single forward reads of ten bases, unit k on transcript ts[k] of ladder() (-1: in the gap behind transcript 0)"""
    return gci.ladder_units(ts)


def fan(n_iso: int, chrom=0, at=1000):
    """n_iso isoforms that share a first exon [at, at + 50) and have a second exon of their own -> the transcripts"""
    return [(chrom, 0, [(at, at + 50), (at + 100 + 30 * k, at + 120 + 30 * k)]) for k in range(n_iso)]


# ---- `dart`: the annotation as a GTF file ----
def write_gtf(path, transcripts, chr_names, rng=None):
    """exon lines, one transcript after the other (rng: the lines of all transcripts shuffled behind each transcript's first line, a line of another feature,
    one on a sequence the index lacks and one without a strand among them) -> the transcripts' names, T<index>"""
    names = ["T%05d" % t for t in range(len(transcripts))]
    line = lambda c, s, e, st, t, feat="exon": "%s\ttest\t%s\t%d\t%d\t.\t%s\t.\tgene_id \"G%05d\"; transcript_id \"%s\";\n" % (c, feat, s + 1, e, st, t // 3, names[t])
    first, rest = [], []
    for t, (c, st, exons) in enumerate(transcripts):
        rows = [line(chr_names[c], s, e, "-" if st else "+", t) for s, e in exons]
        first.append(rows[0]); rest += rows[1:]
    if rng is not None:
        rest += [line(chr_names[0], 10, 20, "+", 0, feat="gene"), line("elsewhere", 10, 20, "+", 0), line(chr_names[0], 10, 20, ".", 0)]
        rng.shuffle(rest)
    with open(path, "w") as f:
        f.write("# a test annotation\n" + "".join(first) + "".join(rest))
    return names


# ---- the golden cases ----
CASE_SEEDS = {"se100": 1, "pe101_spliced": 1, "pe151_spliced": 1}      # chosen on the CPU oracle's records of genecount_inputs.case_batch: rich_enough holds
MIN_MAPQ = 4


def rich_enough(transcripts, classes, words, paired):
    """what a golden case's annotation is chosen for, by the twin alone: at least 10 units in each of the four outcomes, at least 20 classes of two or more
    members and 10 of one, counted units on transcripts of both strands, FL_N >= 100 on the paired cases"""
    strands = {transcripts[t][1] for k in classes for t in k}
    return (min(words[1:5]) >= 10 and sum(1 for k in classes if len(k) >= 2) >= 20 and sum(1 for k in classes if len(k) == 1) >= 10 and strands == {0, 1}
            and (not paired or words[6] >= 100))


# ---- the native program ----
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "txquant_checks_san" if sanitize else "txquant_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "txquant_checks.hip")])
    return exe


def run_program(exe, workdir, tag, n_chr, transcripts, reads, reports, cigar, n_pair_mode, min_mapq=MIN_MAPQ, strand_mode=0, hash_bits=64, frag_mean=200, max_rounds=1000, scale=1,
                arrays=None, start=None):
    """-> dict(err, L, n_ex, segs = per chromosome [(start, ids)], bad, units = [(outcome, ids, fl)], collision, classes, words, range, res, text)"""
    src = os.path.join(workdir, "tx_%s.in" % tag); txt = os.path.join(workdir, "tx_%s.txt" % tag); tab = os.path.join(workdir, "tx_%s.tab" % tag)
    tx, ex = annot_arrays(transcripts) if arrays is None else arrays
    pad = lambda b: b + bytes(-len(b) % 8)
    with open(src, "wb") as f:
        f.write(struct.pack("<16q", n_chr, len(tx), len(ex), len(reads), n_pair_mode, min_mapq, len(reports), len(cigar), strand_mode, hash_bits, frag_mean, max_rounds, scale, 0 if start is None else len(start), 0, 0))
        for a in (tx, ex, np.ascontiguousarray(reads), np.ascontiguousarray(reports), np.ascontiguousarray(cigar, np.uint32)):
            f.write(pad(a.tobytes()))
        if start is not None:                                          # the S the EM begins from, instead of the definition's start values
            f.write(np.asarray(start, np.uint64).tobytes())
    for p in (txt, tab):
        if os.path.exists(p):
            os.remove(p)
    r = subprocess.run([exe, src, txt, tab], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    res = dict(err=None, L=[], n_ex=[], segs=[[] for _ in range(max(n_chr, 0))], bad=None, units=[], collision=None, classes={}, words=None, range=False, res=None, text=None)
    for line in open(txt).read().splitlines():
        w = line.split(" ", 1)
        if w[0] == "err":
            res["err"] = w[1]
            continue
        if w[0] == "range":
            res["range"] = True
            continue
        v = [int(x) for x in w[1].split()]
        if w[0] == "tx":
            res["L"].append(v[1]); res["n_ex"].append(v[2])
        elif w[0] == "seg":
            res["segs"][v[0]].append((v[1], tuple(v[2:])))
        elif w[0] == "bad":
            res["bad"] = v[0]
        elif w[0] == "unit":
            res["units"].append((v[1], tuple(v[4:]), v[3] if v[2] else None))
        elif w[0] == "collision":
            res["collision"] = v[0]
        elif w[0] == "class":
            assert tuple(v[1:]) not in res["classes"]
            res["classes"][tuple(v[1:])] = v[0]
        elif w[0] == "words":
            res["words"] = v
        elif w[0] == "res":
            res["res"] = v
    if os.path.exists(tab):
        res["text"] = open(tab, "rb").read()
    return res


def segments_twin(transcripts, n_chr):
    """the segment table: per chromosome [(start, ids)], neighbours differ, the last one empty"""
    out = []
    for c in range(n_chr):
        ev = set()
        mex = {t: merged(ex) for t, (cc, _, ex) in enumerate(transcripts) if cc == c}
        for m in mex.values():
            for s, e in m:
                ev.add(s); ev.add(e)
        segs = []
        for pos in sorted(ev):
            ids = tuple(t for t in sorted(mex) if any(s <= pos < e for s, e in mex[t]))
            if not segs or segs[-1][1] != ids:
                segs.append((pos, ids))
        assert not segs or segs[-1][1] == ()
        out.append(segs)
    return out


# ---- crafted records on the kernels' seams: run by the GPU suite in its own process, and again in a child under DG_TX_HASH_BITS ----
SEAM_TX = 100000


def seam_sequences(granule: int, wave: int):
    """tag -> the ladder transcripts of single-read units (-1: between two transcripts)"""
    seqs = {"n=%d" % n: [(7 * k) % 50 - 1 for k in range(n)] for n in (granule - 1, granule, granule + 1, 1, 0)}
    seqs["one class"] = [3] * 100000
    seqs["every unit its own class"] = list(range(100000))
    # runs of equal classes that begin and end on wave and workgroup seams, one lane in front of them and one behind
    seqs["seams"] = [5] * wave + [6] + [7] * (wave - 1) + [8] * (2 * wave) + [9] * (wave // 2) + [10] * (wave // 2) + [-1] + [11] * (wave - 1) + [12] * (wave + 1) + [13] * (wave - 1) \
        + [14] * (granule - wave) + [15] * granule + [16] * (granule + 1) + [-1] * (wave - 1) + [17, 18] * wave + [19]
    return seqs


def ladder_expected(ts):
    t = np.asarray(ts, np.int64)
    ids, cnt = np.unique(t[t >= 0], return_counts=True)
    n_bad = int((t < 0).sum())
    return {(int(i),): int(c) for i, c in zip(ids, cnt)}, [len(t), 0, 0, n_bad, len(t) - n_bad, 0, 0, 0]


def fan_records(granule: int):
    """units over fan(300): most on the shared first exon (a list of 300), some spliced into one isoform, pairs in front
    -> (reads, reports, cigar, n_pair_mode)"""
    rec = Records()
    for k in range(40):                                             # pairs: first exon and the isoform's own exon
        iso = (11 * k) % 300
        rec.read(reports=[(0, 1011 + k % 20, 0x61, [(20, M)])]); rec.read(reports=[(0, 1000 + 100 + 30 * iso + 1, 0x91, [(15, M)])])
    for k in range(granule + 37):
        rec.read(reports=[(0, 1001 + k % 21, 0, [(30, M)])])
    for k in range(90):
        iso = (7 * k) % 300
        rec.read(reports=[(0, 1041, 0, [(10, M), (100 + 30 * iso - 50, N), (10 + k % 3, M)])])
    rd, rp, cg = rec.arrays()
    return rd, rp, cg, 80


def seam_tables(gpu):
    """every crafted run on a context -> [(tag, classes dict, the eight words, dg_tx_finish's words at 16 rounds)]"""
    out = []
    granule, wave = gpu.tx_granules()

    def take(tag):
        off, ids, cnt, words = gpu.tx_classes()
        out.append((tag, table_dict(off, ids, cnt), [int(x) for x in words], [int(x) for x in gpu.tx_finish(200, 16)]))

    gpu.tx_set_annotation(*ladder(SEAM_TX))
    seqs = seam_sequences(granule, wave)
    for tag in seqs:
        gpu.tx_reset()
        rd, rp, cg = ladder_units(seqs[tag])
        assert gpu.tx_count_records(rd, rp, cg, 0, MIN_MAPQ) == len(seqs[tag]), tag
        take(tag)
    # the seams again in two calls: the second call's classes meet the table's
    gpu.tx_reset()
    for part in (seqs["seams"][:granule + 5], seqs["seams"][granule + 5:]):
        gpu.tx_count_records(*ladder_units(part), 0, MIN_MAPQ)
    take("seams in two calls")
    # pairs: the same sequence as mates (2i, 2i + 1)
    rd, rp, cg = ladder_units(seqs["seams"][:2 * granule + 2])
    rp["flag"] = np.where(np.arange(len(rp)) & 1, 0x91, 0x61)
    gpu.tx_reset(); gpu.tx_count_records(rd, rp, cg, len(rd), MIN_MAPQ)
    take("pairs")
    gpu.tx_set_annotation(*annot_arrays(fan(300)))
    gpu.tx_reset()
    rd, rp, cg, npm = fan_records(granule)
    gpu.tx_count_records(rd, rp, cg, npm, MIN_MAPQ)
    take("fan")
    return out


if __name__ == "__main__":          # the child of the GPU suite: <index prefix> <output.json>; the environment (DG_TX_HASH_BITS) is the parent's choice
    import json, sys
    ix = host.Index(sys.argv[1])
    gpu = host.DartGPU(ix, host.default_params(paired=0, max_mismatch=5))
    try:
        tabs = seam_tables(gpu)
    finally:
        gpu.close()
    with open(sys.argv[2], "w") as f:
        json.dump([(tag, sorted((list(k), v) for k, v in cl.items()), words, res) for tag, cl, words, res in tabs], f)
