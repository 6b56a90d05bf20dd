"""GPU suite (-m gpu): gene-level read counts on the device (dg_gene_*, dart_amd/csrc/dg_genecount.h) against the sequential Python twin of
tests/genecount_inputs.py over the records downloaded the old way.  The table is the definition in the header's comment; no counting tool is run."""
import ctypes as C
import numpy as np
import pytest
import common
import genecount_inputs as gci
from dart_amd import host

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_CAPACITY = -3, -4
MIN_MAPQ = 4
CASES = ["se100", "pe101_spliced", "pe151_spliced"]


def _params(c):
    return host.default_params(paired=1 if c["spec"]["paired"] else 0, max_mismatch=5)


@pytest.fixture(scope="module")
def small(workdir):
    """the smallest golden index: a root context and two clones"""
    c = common.build_case("se100", workdir)
    ix = host.Index(c["prefix"])
    gpu = host.DartGPU(ix, _params(c))
    yield c, ix, gpu, gpu.clone(), gpu.clone()
    gpu.close()


@pytest.mark.parametrize("name", CASES)
def test_mapped_batches_equal_the_twin_whatever_the_split(name, workdir):
    c = common.build_case(name, workdir)
    n_chr = len(c["genome"].lengths)
    n_genes, exons = gci.case_annotation(c, gci.CASE_SEEDS[name])
    arr, npm = gci.case_batch(c)
    ix = host.Index(c["prefix"])
    gpu = host.DartGPU(ix, _params(c))
    try:
        segs = gci.flatten(n_chr, exons)
        assert gpu.gene_set_annotation(n_genes, exons) == sum(len(s) for s in segs)
        # one batch
        res = gpu.map_batch(*host.pack_reads(arr))
        n_units = gpu.accumulate_genes(npm, MIN_MAPQ)
        one = gpu.gene_counts()
        want = gci.twin(n_chr, n_genes, exons, res.reads, res.reports, res.cigar, npm, MIN_MAPQ, segs=segs)
        prof = gci.outcome_profile(want)
        print(name, "units", n_units, "profile", prof, "device ms", gpu.gene_device_ms)
        assert gci.rich_enough(want, n_genes, exons), prof          # by the twin alone: every outcome at least ten times in every column, both strands' genes counted in columns 1 and 2
        assert n_units == len(gci.units_of(len(arr), npm)) == int(one[:, 0].sum())
        assert np.array_equal(one, want), np.argwhere(one != want)[:5]
        # three batches over a root and two clones (which count with the root's annotation), merged
        ctxs = [gpu, gpu.clone(), gpu.clone()]
        gpu.gene_reset()
        cut = [0, len(arr) // 3 // 2 * 2, len(arr) // 3 // 2 * 4 + 2, len(arr)]
        for g, lo, hi in zip(ctxs[::-1], cut[:-1], cut[1:]):
            g.set_params(_params(c))
            g.map_batch(*host.pack_reads(arr[lo:hi]))
            g.accumulate_genes(hi - lo if npm else 0, MIN_MAPQ)
        gpu.gene_merge(ctxs[2]); gpu.gene_merge(ctxs[1])
        assert np.array_equal(gpu.gene_counts(), want)
        assert ctxs[1].gene_counts().sum() == 0 and ctxs[2].gene_counts().sum() == 0      # after the merge the source is empty
        # the downloaded records fed back through dg_gene_count_records, on a clone
        assert ctxs[1].gene_count_records(res.reads, res.reports, res.cigar, npm, MIN_MAPQ) == n_units
        assert np.array_equal(ctxs[1].gene_counts(), want)
        # another min_mapq moves units between N_multimapping and the rest
        gpu.gene_reset()
        gpu.gene_count_records(res.reads, res.reports, res.cigar, npm, 0)
        zero = gpu.gene_counts()
        assert zero[1].sum() == 0 and np.array_equal(zero, gci.twin(n_chr, n_genes, exons, res.reads, res.reports, res.cigar, npm, 0, segs=segs))
        # the text
        text = common.sam.gene_table(gci.gene_names(n_genes), want)
        lines = text.decode().splitlines()
        assert len(lines) == 4 + n_genes and lines[0] == "N_unmapped\t%d\t%d\t%d" % tuple(int(x) for x in want[0]) and lines[3].startswith("N_ambiguous\t")
        assert lines[4] == "G00000\t%d\t%d\t%d" % tuple(int(x) for x in want[4])
    finally:
        gpu.close()


def test_packed_upload_and_a_batch_of_no_reads(small):
    c, ix, gpu, cl1, _ = small
    n_genes, exons = gci.case_annotation(c, gci.CASE_SEEDS["se100"])
    gpu.gene_set_annotation(n_genes, exons); gpu.gene_reset()
    reads = c["reads"][:600]
    res = gpu.map_batch(*host.pack_reads(reads))
    want = gci.twin(1, n_genes, exons, res.reads, res.reports, res.cigar, 0, MIN_MAPQ)
    words, nlist = host.pack_reads_2bit(reads)
    cl1.set_params(_params(c)); cl1.gene_reset()
    cl1.map_batch_packed(words, nlist, reads.shape[1])                    # no bases are needed: a packed batch counts
    assert cl1.accumulate_genes(0, MIN_MAPQ) == 600 and np.array_equal(cl1.gene_counts(), want)
    cl1.upload(*host.pack_reads(reads[:0])); cl1.run()
    assert cl1.accumulate_genes(0, MIN_MAPQ) == 0 and np.array_equal(cl1.gene_counts(), want)      # a batch of 0 reads adds nothing


def test_crafted_records_on_the_kernels_seams(small):
    c, ix, gpu, _, _ = small
    granule, wave = gpu.gene_granules()
    assert granule >= wave >= 32 and granule % wave == 0
    n_genes = 100000
    ann = gci.ladder_annotation(n_genes)
    assert gpu.gene_set_annotation(n_genes, ann.view(host.GENE_EXON)) == 2 * n_genes
    exons = [tuple(int(x) for x in e) for e in ann[:400]]
    def run(genes, tag):
        gpu.gene_reset()
        rd, rp, cg = gci.ladder_units(genes)
        assert gpu.gene_count_records(rd, rp, cg, 0, MIN_MAPQ) == len(genes), tag
        got = gpu.gene_counts()
        want = gci.ladder_expected(genes, n_genes)
        assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:5])
        k = min(len(genes), 300)                                         # the expectation itself against the twin, on units of the first 400 genes
        if k and max(genes[:k]) < 400:
            assert np.array_equal(gci.twin(1, 400, exons, rd[:k], rp[:k], cg[:k], 0, MIN_MAPQ), gci.ladder_expected(genes[:k], 400)), tag
    for n in (granule - 1, granule, granule + 1, 1, 0):
        run([(7 * k) % 50 - 1 for k in range(n)], "n=%d" % n)
    run([3] * 100000, "one gene")
    run(list(range(100000)), "every unit its own gene")
    # runs of equal genes that start and end on wave seams, one lane in front of them and one behind
    seq = [5] * wave + [6] + [7] * (wave - 1) + [8] * (2 * wave) + [9] * (wave // 2) + [10] * (wave // 2) + [-1] + [11] * (wave - 1) + [12] * (wave + 1) + [13] * (wave - 1) + [14] * (granule - wave) \
        + [15] * granule + [16] * (granule + 1) + [-1] * (wave - 1) + [17, 18] * wave + [19]
    run(seq, "seams")
    # pairs: the same sequence as mates (2i, 2i + 1): runs of two equal genes count once, different genes are ambiguous
    rd, rp, cg = gci.ladder_units(seq[:2 * granule + 2])
    rp["flag"] = np.where(np.arange(len(rp)) & 1, 0x91, 0x41)
    gpu.gene_reset()
    gpu.gene_count_records(rd, rp, cg, len(rd), MIN_MAPQ)
    assert np.array_equal(gpu.gene_counts()[:404], gci.twin(1, 400, exons, rd, rp, cg, len(rd), MIN_MAPQ))


def test_error_cases_leave_the_table_as_it_was(small):
    c, ix, gpu, cl1, cl2 = small
    lib = gpu.lib
    err = lambda g: lib.dg_last_error(g.ctx)
    n_units = C.c_size_t(7)
    # no annotation: a root of its own (the annotation lives with the index)
    fresh = host.DartGPU(ix, _params(c))
    try:
        fresh.map_batch(*host.pack_reads(c["reads"][:100]))
        assert lib.dg_batch_accumulate_genes(fresh.ctx, 0, MIN_MAPQ, C.byref(n_units)) == ERR_ARG and b"annotation" in err(fresh) and n_units.value == 0
        out = np.zeros((8, 3), np.uint64)
        assert lib.dg_gene_download(fresh.ctx, out.ctypes.data, 8) == ERR_ARG and lib.dg_gene_reset(fresh.ctx) == ERR_ARG
        # no batch
        fresh2 = fresh.clone()
        n_genes, exons = gci.case_annotation(c, gci.CASE_SEEDS["se100"])
        fresh.gene_set_annotation(n_genes, exons)
        assert lib.dg_batch_accumulate_genes(fresh2.ctx, 0, MIN_MAPQ, None) == ERR_ARG and b"no finished batch" in err(fresh2)
        assert fresh2.gene_counts(4 + n_genes).sum() == 0
    finally:
        fresh.close()
    n_genes, exons = gci.case_annotation(c, gci.CASE_SEEDS["se100"])
    gpu.gene_set_annotation(n_genes, exons)
    for g in (gpu, cl1, cl2):
        g.set_params(_params(c)); g.gene_reset()
    reads = c["reads"][:500]
    res = gpu.map_batch(*host.pack_reads(reads))
    assert gpu.accumulate_genes(0, MIN_MAPQ) == 500
    before = gpu.gene_counts()
    assert before.sum() == 1500
    same = lambda: np.array_equal(gpu.gene_counts(4 + n_genes), before)
    # a second call on the same batch, also behind a download
    assert lib.dg_batch_accumulate_genes(gpu.ctx, 0, MIN_MAPQ, None) == ERR_ARG and b"once" in err(gpu) and same()
    gpu.download()
    assert lib.dg_batch_accumulate_genes(gpu.ctx, 0, MIN_MAPQ, None) == ERR_ARG and b"once" in err(gpu) and same()
    # odd n_pair_mode, and one above the batch (on a batch that is not counted yet)
    gpu.map_batch(*host.pack_reads(reads))
    assert lib.dg_batch_accumulate_genes(gpu.ctx, 3, MIN_MAPQ, None) == ERR_ARG and b"n_pair_mode" in err(gpu) and same()
    assert lib.dg_batch_accumulate_genes(gpu.ctx, 502, MIN_MAPQ, None) == ERR_ARG and b"n_pair_mode" in err(gpu) and same()
    # after dg_map_batch_compact: no full records
    words, nlist = host.pack_reads_2bit(reads)
    gpu.map_batch_compact(words, nlist, reads.shape[1])
    assert lib.dg_batch_accumulate_genes(gpu.ctx, 0, MIN_MAPQ, None) == ERR_ARG and b"no full records" in err(gpu) and same()
    # merge into itself; a short download buffer (nothing written)
    assert lib.dg_gene_merge(gpu.ctx, gpu.ctx) == ERR_ARG and same()
    short = np.full((3 + n_genes, 3), 0x55, np.uint64)
    assert lib.dg_gene_download(gpu.ctx, short.ctypes.data, 3 + n_genes) == ERR_CAPACITY and b"needed" in err(gpu) and (short == 0x55).all() and same()
    # dg_gene_add: a wrong row count; the downloaded table doubles it
    assert lib.dg_gene_add(gpu.ctx, before.ctypes.data, 3 + n_genes) == ERR_ARG and same()
    gpu.gene_add(before)
    assert np.array_equal(gpu.gene_counts(), 2 * before)
    gpu.gene_reset(); gpu.gene_add(before)
    assert same()
    # bad host records: the first bad read is named, nothing is counted
    r = res.reads.copy(); r["n_rep"][len(r) - 1] += 1; r["best"][7] = -1
    assert lib.dg_gene_count_records(gpu.ctx, len(r), 0, MIN_MAPQ, r.ctypes.data, res.reports.ctypes.data, len(res.reports), res.cigar.ctypes.data, len(res.cigar), C.byref(n_units)) == ERR_ARG
    want_bad = 7 if res.reads["score"][7] > 0 else len(r) - 1
    assert (b"read %d " % want_bad) in err(gpu) and n_units.value == 0 and same()
    assert lib.dg_gene_count_records(gpu.ctx, len(r), 0, MIN_MAPQ, res.reads.ctypes.data, res.reports.ctypes.data, len(res.reports), res.cigar.ctypes.data, len(res.cigar) - 1, None) == ERR_ARG and same()
    assert lib.dg_gene_count_records(gpu.ctx, 501, 502, MIN_MAPQ, res.reads.ctypes.data, res.reports.ctypes.data, len(res.reports), res.cigar.ctypes.data, len(res.cigar), None) == ERR_ARG and same()
    # a bad annotation leaves the old one in place
    assert lib.dg_gene_set_annotation(gpu.ctx, C.byref(host.GeneAnnot(0, 0, 0, None)), None) == ERR_ARG
    bad = np.zeros(2, host.GENE_EXON); bad[0] = (0, 5, 9, 0, 0); bad[1] = (0, 9, 9, 0, 0)
    assert lib.dg_gene_set_annotation(gpu.ctx, C.byref(host.GeneAnnot(1, 0, 2, bad.ctypes.data)), None) == ERR_ARG and b"exon 1 " in err(gpu)
    cl1.gene_count_records(res.reads, res.reports, res.cigar, 0, MIN_MAPQ)
    assert np.array_equal(cl1.gene_counts(), before)
    # a new annotation over a table that holds counts: reset first; tables of different generations do not merge
    cl2.gene_count_records(res.reads[:10], res.reports, res.cigar, 0, MIN_MAPQ)
    gpu.gene_set_annotation(3, [(0, 10, 20, 0, 2)])
    gpu.map_batch(*host.pack_reads(reads))
    assert lib.dg_batch_accumulate_genes(gpu.ctx, 0, MIN_MAPQ, None) == ERR_ARG and b"reset first" in err(gpu) and same()
    assert lib.dg_gene_count_records(gpu.ctx, len(res.reads), 0, MIN_MAPQ, res.reads.ctypes.data, res.reports.ctypes.data, len(res.reports), res.cigar.ctypes.data, len(res.cigar), None) == ERR_ARG and same()
    cl2.gene_reset()
    cl2.gene_count_records(res.reads[:10], res.reports, res.cigar, 0, MIN_MAPQ)
    assert lib.dg_gene_merge(cl2.ctx, cl1.ctx) == ERR_ARG and b"generation" in err(cl2) and np.array_equal(cl1.gene_counts(4 + n_genes), before)
    gpu.gene_reset()
    assert gpu.accumulate_genes(0, MIN_MAPQ) == 500
    got = gpu.gene_counts()
    assert got.shape == (7, 3) and np.array_equal(got, gci.twin(1, 3, [(0, 10, 20, 0, 2)], res.reads, res.reports, res.cigar, 0, MIN_MAPQ))
