"""Helpers of the gene-count tests: the sequential Python twin of the definition in dart_amd/csrc/dg_genecount.h (the flattening as a sweep over sorted
breakpoints with one dictionary per gene set; the count unit by unit over the (reads, reports, cigar) record arrays), a second, independent check of the
flattening (a per-base painter), a builder of crafted records, a random annotation generator and the native program tests/native/genecount_checks.hip.
The definition is the header's comment: no htseq-count, featureCounts or STAR exists where these tests run."""
from __future__ import annotations

import bisect, os, struct, subprocess
import numpy as np
import common
from dart_amd import host

NONE, AMBIG = 0xFFFFFFFF, 0xFFFFFFFE
ROW_UNMAPPED, ROW_MULTI, ROW_NOFEATURE, ROW_AMBIG, ROW_GENE0 = 0, 1, 2, 3, 4
EXON = np.dtype([("chr", "<i4"), ("start", "<u4"), ("end", "<u4"), ("strand", "<u4"), ("gene", "<u4")])
PAINT_LIMIT = 1 << 20
M, I, D, N, S, H, P, EQ, X = range(9)


def exon_array(exons) -> np.ndarray:
    rows = list(exons)
    a = np.zeros(len(rows), EXON)
    for k, (c, s, e, st, g) in enumerate(rows):
        a[k] = (c, s, e, st, g)
    return a


# ---- the flattening ----
def _label(active: dict) -> int:
    return NONE if not active else next(iter(active)) if len(active) == 1 else AMBIG


def flatten(n_chr: int, exons):
    """-> per chromosome a list of (start, any, plus, minus), ascending, neighbours differ, the last one all NONE; a chromosome without exons: []"""
    per = [[] for _ in range(n_chr)]
    for c, s, e, st, g in exons:
        per[int(c)].append((int(s), int(e), int(st), int(g)))
    out = []
    for rows in per:
        ev = {}
        for s, e, st, g in rows:
            ev.setdefault(s, []).append((1, st, g)); ev.setdefault(e, []).append((-1, st, g))
        act = ({}, {}, {})
        segs = []
        for pos in sorted(ev):
            for d, st, g in ev[pos]:
                for m in (act[0], act[1 + st]):
                    m[g] = m.get(g, 0) + d
                    if m[g] == 0:
                        del m[g]
            lab = (_label(act[0]), _label(act[1]), _label(act[2]))
            if not segs or segs[-1][1:] != lab:
                segs.append((pos,) + lab)
        assert not segs or segs[-1][1:] == (NONE, NONE, NONE)
        out.append(segs)
    return out


def paint(n_chr: int, n_genes: int, exons, limit=PAINT_LIMIT):
    """the independent check: per chromosome and gene set a per-base label array over [0, limit).  Per gene a boolean cover array is painted exon by exon;
    a count array says how many genes cover a base and a last-gene array which one did last; the label comes from the count."""
    count = np.zeros((n_chr, 3, limit), np.int32); last = np.full((n_chr, 3, limit), -1, np.int64)
    by_gene = {}
    for c, s, e, st, g in exons:
        by_gene.setdefault(int(g), []).append((int(c), int(s), int(e), int(st)))
    for g in sorted(by_gene):
        for c in sorted({r[0] for r in by_gene[g]}):
            rows = [r for r in by_gene[g] if r[0] == c]
            lo, hi = min(r[1] for r in rows), min(max(r[2] for r in rows), limit)
            if lo >= hi:
                continue
            cover = np.zeros((3, hi - lo), bool)
            for _, s, e, st in rows:
                cover[0, s - lo:max(min(e, limit) - lo, 0)] = True
                cover[1 + st, s - lo:max(min(e, limit) - lo, 0)] = True
            for k in range(3):
                count[c, k, lo:hi] += cover[k]
                last[c, k, lo:hi][cover[k]] = g
    lab = np.where(count == 0, NONE, np.where(count == 1, last, AMBIG)).astype(np.int64)
    return lab


def expand(segs, limit=PAINT_LIMIT):
    """the twin's segments of one chromosome as per-base labels [3, limit]"""
    out = np.full((3, limit), NONE, np.int64)
    for k, seg in enumerate(segs):
        s = min(seg[0], limit); e = min(segs[k + 1][0], limit) if k + 1 < len(segs) else limit
        for j in range(3):
            out[j, s:e] = seg[1 + j]
    return out


def assert_painter_agrees(n_chr, n_genes, exons, segs=None, limit=PAINT_LIMIT):
    segs = flatten(n_chr, exons) if segs is None else segs
    lab = paint(n_chr, n_genes, exons, limit)
    for c in range(n_chr):
        assert np.array_equal(lab[c], expand(segs[c], limit)), "chromosome %d" % c


# ---- the count ----
def combine(a: int, b: int) -> int:
    return b if a == NONE else a if (b == NONE or a == b) else AMBIG


def row_of(label: int) -> int:
    return ROW_NOFEATURE if label == NONE else ROW_AMBIG if label == AMBIG else ROW_GENE0 + label


def alignment(reads, reports, k: int, pair: bool):
    """the index (inside `reports`) of read k's first shown report, or None"""
    r = reads[k]
    if int(r["score"]) <= 0:
        return None
    for j in range(int(r["best"]), int(r["n_rep"])):
        a = int(reports[int(r["rep_off"]) + j]["aln_score"])
        if (a > 0) if pair else (a == int(r["score"])):
            return int(r["rep_off"]) + j
    return None


def blocks(rep, cigar, n_chr: int):
    pos, c = int(rep["pos"]), int(rep["chr"])
    if pos < 1 or not 0 <= c < n_chr:
        return []
    out, p = [], pos - 1
    for w in cigar[int(rep["cigar_off"]):int(rep["cigar_off"]) + int(rep["n_cigar"])].tolist():
        op, ln = w & 15, w >> 4
        if op in (M, EQ, X):
            if ln:
                out.append((p, p + ln))
            p += ln
        elif op in (D, N):
            p += ln
    return out


def units_of(n_reads: int, n_pair_mode: int):
    return [(2 * i, 2 * i + 1) for i in range(n_pair_mode // 2)] + [(k,) for k in range(n_pair_mode, n_reads)]


def unit_rows(segs, starts, n_chr, reads, reports, cigar, unit, n_pair_mode, min_mapq):
    al = [(k, alignment(reads, reports, k, k < n_pair_mode)) for k in unit]
    al = [(k, a) for k, a in al if a is not None]
    if not al:
        return (ROW_UNMAPPED,) * 3
    if any(int(reads[k]["mapq"]) < min_mapq for k, _ in al):
        return (ROW_MULTI,) * 3
    acc = [NONE, NONE, NONE]
    for _, a in al:
        rep = reports[a]
        s = (int(rep["flag"]) >> 4 & 1) ^ (int(rep["flag"]) >> 7 & 1)
        sg, st = segs[int(rep["chr"])] if 0 <= int(rep["chr"]) < n_chr else [], starts[int(rep["chr"])] if 0 <= int(rep["chr"]) < n_chr else []
        for b0, b1 in blocks(rep, cigar, n_chr):
            i = max(bisect.bisect_right(st, b0) - 1, 0)
            while i < len(sg) and sg[i][0] < b1:
                _, any_, plus, minus = sg[i]
                acc[0] = combine(acc[0], any_); acc[1] = combine(acc[1], minus if s else plus); acc[2] = combine(acc[2], plus if s else minus)
                i += 1
    return tuple(row_of(x) for x in acc)


def twin(n_chr, n_genes, exons, reads, reports, cigar, n_pair_mode, min_mapq, segs=None, want_rows=False):
    """-> counts uint64 [4 + n_genes, 3] (and the per-unit rows)"""
    segs = flatten(n_chr, exons) if segs is None else segs
    starts = [[s[0] for s in sg] for sg in segs]
    counts = np.zeros((4 + n_genes, 3), np.uint64)
    rows = []
    for unit in units_of(len(reads), n_pair_mode):
        r = unit_rows(segs, starts, n_chr, reads, reports, cigar, unit, n_pair_mode, min_mapq)
        rows.append(r)
        for col in range(3):
            counts[r[col], col] += np.uint64(1)
    assert (counts.sum(axis=0) == len(rows)).all()
    return (counts, rows) if want_rows else counts


def gene_names(n_genes):
    return ["G%05d" % g for g in range(n_genes)]


# ---- crafted records ----
class Records:
    """builds (reads, reports, cigar) arrays read by read"""

    def __init__(self):
        self.reads, self.reports, self.cigar = [], [], []

    def read(self, reports=(), score=None, mapq=50, best=0):
        """reports: (chr, pos (1-based), flag, [(len, op)], aln_score = 100) tuples; no reports: an unmapped read (score 0, one empty report with flag 4)"""
        reports = [tuple(r) + (100,) * (5 - len(r)) for r in reports]
        if not reports:
            self.reads.append((0, 0, 0, 0, 1, 0, len(self.reports), 0, 0))
            self.reports.append((0, -1, 4, -1, -1, 0, 0, len(self.cigar), 0))
            return self
        sc = reports[best][4] if score is None else score
        self.reads.append((sc, 0, 0, mapq, len(reports), best, len(self.reports), 0, 0))
        for c, pos, flag, ops, a in reports:
            self.reports.append((a, -1, flag, -1, c, 0, pos, len(self.cigar), len(ops)))
            self.cigar += [ln << 4 | op for ln, op in ops]
        return self

    def arrays(self):
        rd = np.array(self.reads, dtype=host.READ_OUT) if self.reads else np.zeros(0, host.READ_OUT)
        rp = np.zeros(len(self.reports), host.REPORT_OUT)
        for k, (a, sj, flag, pj, c, bdir, pos, off, n) in enumerate(self.reports):
            rp[k]["aln_score"], rp[k]["sj_type"], rp[k]["flag"], rp[k]["paired_idx"], rp[k]["chr"], rp[k]["bdir"] = a, sj, flag, pj, c, bdir
            rp[k]["pos"], rp[k]["cigar_off"], rp[k]["n_cigar"] = pos, off, n
        return rd, rp, np.asarray(self.cigar, np.uint32)


def random_annotation(rng, lengths, introns=None, offsets=None, cover=0.5, overlap=0.15):
    """genes of 1-6 exons, some overlapping a neighbour on the same strand and some on the opposite one, some exon ends on the genome's planted introns,
    roughly `cover` of the genome covered -> (n_genes, exon rows)"""
    exons, g = [], 0
    cuts = [[] for _ in lengths]
    if introns is not None and len(introns):
        for s, ln, _ in np.asarray(introns).tolist():
            c = int(np.searchsorted(offsets, s, side="right")) - 1
            cuts[c].append((int(s - offsets[c]), int(s - offsets[c] + ln)))
    for c, L in enumerate(lengths):
        L = int(L); covered = 0; at = rng.randrange(50, 400)
        while covered < cover * L and at < L - 4000:
            strand = rng.randrange(2)
            n_ex = rng.randrange(1, 7)
            p = at; first = p; last = p
            for k in range(n_ex):
                ln = rng.randrange(40, 700)
                e = min(p + ln, L - 1)
                near = [q for q in cuts[c] if p + 30 < q[0] <= e + 300]
                if near and rng.random() < 0.6:          # the exon ends on an intron's first base, the next begins behind its last
                    e = near[0][0]
                if e <= p:
                    break
                exons.append((c, p, e, strand, g)); covered += e - p; last = max(last, e)
                if rng.random() < 0.05:
                    exons.append((c, p, e, strand, g))      # a repeated exon
                gap = rng.randrange(60, 900)
                hit = [q for q in cuts[c] if q[0] == e]
                p = hit[0][1] if hit else e + gap
                if p >= L - 800:
                    break
            g += 1
            kind = rng.random()
            if kind < overlap:
                at = max(first + 20, last - rng.randrange(30, 200))      # the next gene overlaps this one's tail (its strand is its own: same or opposite)
            else:
                at = last + rng.randrange(100, 1500)
    rng.shuffle(exons)
    return max(g, 1), exons


def case_annotation(case, seed):
    """a random annotation over a golden case's genome, some exon ends on its planted introns -> (n_genes, exon rows)"""
    import random
    g = case["genome"]
    return random_annotation(random.Random(seed), [int(x) for x in g.lengths], g.introns, g.offsets, overlap=0.45)


# pairs of the golden sets that fall into their genome's repeats (MAPQ below 4 at -mis 5, by the CPU oracle)
MULTI_PAIRS = {"pe101_spliced": [381, 922, 1430], "pe151_spliced": [312, 483, 574, 814, 940]}


def case_batch(case):
    """the batch the gene-count tests map for a golden case -> (reads uint8 [n, rlen], n_pair_mode).  se100 as it is.  The paired sets hold no pair without
    an alignment and three to five in repeats, so theirs are the golden reads with an appendix: each pair of MULTI_PAIRS four more times, and sixteen pairs
    of random bases."""
    arr = case["reads"]
    if not case["spec"]["paired"]:
        return arr, 0
    rep = np.concatenate([arr[2 * i:2 * i + 2] for i in MULTI_PAIRS[case["name"]]] * 4)
    rnd = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(5).integers(0, 4, (32, arr.shape[1]))]
    out = np.ascontiguousarray(np.concatenate([arr, rep, rnd]))
    return out, len(out)


CASE_SEEDS = {"se100": 14, "pe101_spliced": 3, "pe151_spliced": 5}      # chosen on the CPU oracle's records of case_batch: rich_enough holds


def ladder_annotation(n_genes: int):
    """gene g: one plus-strand exon [100 + 20 g, 110 + 20 g) on chromosome 0"""
    a = np.zeros(n_genes, EXON)
    a["start"] = 100 + 20 * np.arange(n_genes, dtype=np.int64); a["end"] = a["start"] + 10; a["gene"] = np.arange(n_genes)
    return a


def ladder_units(genes):
    """single forward reads of ten bases, unit k on gene genes[k] of ladder_annotation (-1: in the gap in front of gene 0's neighbour) -> (reads, reports,
    cigar, the expected table's columns as (rows, col 0 = col 1 counts, N_noFeature of col 2))"""
    g = np.asarray(genes, np.int64)
    n = len(g)
    reads = np.zeros(n, host.READ_OUT); reports = np.zeros(n, host.REPORT_OUT)
    reads["score"], reads["mapq"], reads["n_rep"], reads["rep_off"] = 100, 50, 1, np.arange(n)
    reports["aln_score"], reports["sj_type"], reports["paired_idx"] = 100, -1, -1
    reports["pos"] = np.where(g >= 0, 101 + 20 * g, 111)
    reports["cigar_off"], reports["n_cigar"] = np.arange(n), 1
    return reads, reports, np.full(n, 10 << 4 | M, np.uint32)


def ladder_expected(genes, n_genes):
    g = np.asarray(genes, np.int64)
    out = np.zeros((4 + n_genes, 3), np.uint64)
    out[4:, 0] = out[4:, 1] = np.bincount(g[g >= 0], minlength=n_genes).astype(np.uint64)
    out[ROW_NOFEATURE, 0] = out[ROW_NOFEATURE, 1] = np.uint64((g < 0).sum())
    out[ROW_NOFEATURE, 2] = np.uint64(len(g))
    return out


def gene_strands(n_genes, exons):
    st = [None] * n_genes
    for _, _, _, s, g in exons:
        st[g] = s
    return st


def rich_enough(counts, n_genes, exons):
    """what a golden case's annotation is chosen for: each of the five outcomes at least ten times in every column, and in each of columns 1 and 2 units
    counted for genes of both strands"""
    st = gene_strands(n_genes, exons)
    ok = all(min(p) >= 10 for p in outcome_profile(counts))
    for col in (1, 2):
        ok = ok and {st[g] for g in range(n_genes) if counts[4 + g, col]} >= {0, 1}
    return ok


def outcome_profile(counts):
    """per column (unmapped, multimapping, nofeature, ambiguous, counted)"""
    return [(int(counts[0, c]), int(counts[1, c]), int(counts[2, c]), int(counts[3, c]), int(counts[4:, c].sum())) for c in range(3)]


# ---- the native program ----
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "genecount_checks_san" if sanitize else "genecount_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "genecount_checks.hip")])
    return exe


def run_program(exe, workdir, tag, n_chr, n_genes, exons, reads, reports, cigar, n_pair_mode, min_mapq):
    """-> dict(err = the flattening's refusal or None, segs = per chromosome [(start, any, plus, minus)], bad = the first bad read or None, rows = per unit
    (r0, r1, r2), counts = uint64 [4 + n_genes, 3])"""
    src = os.path.join(workdir, "gc_%s.in" % tag); txt = os.path.join(workdir, "gc_%s.txt" % tag)
    ex = exon_array(exons) if not isinstance(exons, np.ndarray) else exons
    pad = lambda b: b + bytes(-len(b) % 8)
    with open(src, "wb") as f:
        f.write(struct.pack("<9q", n_chr, n_genes, len(ex), len(reads), n_pair_mode, min_mapq, len(reports), len(cigar), 0))
        for a in (ex, np.ascontiguousarray(reads), np.ascontiguousarray(reports), np.ascontiguousarray(cigar, np.uint32)):
            f.write(pad(a.tobytes()))
    r = subprocess.run([exe, src, txt], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    res = dict(err=None, segs=[[] for _ in range(max(n_chr, 0))], bad=None, rows=[], counts=np.zeros((4 + max(n_genes, 0), 3), np.uint64))
    for line in open(txt).read().splitlines():
        w = line.split(" ", 1)
        if w[0] == "err":
            res["err"] = w[1]
            continue
        v = [int(x) for x in w[1].split()]
        if w[0] == "seg":
            res["segs"][v[0]].append(tuple(v[1:]))
        elif w[0] == "bad":
            res["bad"] = v[0]
        elif w[0] == "unit":
            res["rows"].append(tuple(v[1:]))
        elif w[0] == "row":
            res["counts"][v[0]] = v[1:]
    return res


# ---- `dart`: the annotation as a GTF file, and the twin's records from the SAM file a run wrote ----
def write_gtf(path, exons, chr_names):
    """one exon line per row, in the rows' order -> the gene indices in the order of their first appearance (the order of the table's rows)"""
    order, seen = [], set()
    with open(path, "w") as f:
        f.write("# a test annotation\n")
        for c, s, e, st, g in exons:
            if g not in seen:
                seen.add(g); order.append(g)
            f.write("%s\ttest\texon\t%d\t%d\t.\t%s\t.\tgene_id \"G%05d\"; transcript_id \"T%05d.1\";\n" % (chr_names[c], s + 1, e, "-" if st else "+", g, g))
            if len(order) % 7 == 0:
                f.write("%s\ttest\tgene\t%d\t%d\t.\t%s\t.\tgene_id \"other_feature\";\n" % (chr_names[c], s + 1, e, "-" if st else "+"))
    return order


def table_in_file_order(counts, order):
    """the twin's table with its gene rows in the GTF's order of first appearance, and the names of those rows"""
    rows = np.concatenate([counts[:4], counts[4:][order]]) if len(order) else counts[:4]
    return ["G%05d" % g for g in order], rows


def sam_records(sam_text: str, n_reads: int, paired: bool, chr_names, unique: bool):
    """the (reads, reports, cigar) arrays of the SAM file's first line per read, reads in input order (mate 1 in front of mate 2); names are r<k>.  A read that
    `-unique` left out of the file is one with an alignment and a MAPQ of at most 3: it is put back as such, without blocks -> (arrays, n_pair_mode)"""
    first = {}
    for line in sam_text.splitlines():
        if line.startswith("@"):
            continue
        w = line.split("\t")
        flag = int(w[1])
        key = (w[0], 1 if flag & 0x80 else 0) if flag & 1 else (w[0], 0)
        assert bool(flag & 1) == paired
        first.setdefault(key, w)
    chr_of = {n: i for i, n in enumerate(chr_names)}
    rec = Records()
    n_units = n_reads // 2 if paired else n_reads
    for u in range(n_units):
        for mate in ((0, 1) if paired else (0,)):
            w = first.get(("r%d" % u, mate))
            if w is None:
                assert unique
                rec.read(reports=[(0, 0, 0, [], 1)], score=1, mapq=0)
                continue
            flag = int(w[1])
            if flag & 4:
                rec.read()
                continue
            ops, num = [], ""
            for ch in w[5]:
                if ch.isdigit():
                    num += ch
                else:
                    ops.append((int(num), "MIDNS".index(ch))); num = ""
            score = int([t for t in w[11:] if t.startswith("AS:i:")][0][5:])
            rec.read(reports=[(chr_of[w[2]], int(w[3]), flag, ops, score)], score=score, mapq=int(w[4]))
    return rec.arrays(), (n_reads if paired else 0)
