"""GPU suite (-m gpu): nothing a context owns outlives it.  A root context and a clone drive every library stage once, are closed, and the cycle runs again: the
device's free memory after the third cycle is what it was after the second, and the third cycle's outputs are the first's byte for byte (a fresh context starts
from nothing).  The first cycle is not measured: the runtime loads code objects and sizes its own pools on first use.

Measured on an MI355X (free bytes after cycle 2 minus free bytes after cycle 3):
    parent commit (dg_destroy frees every field by hand): 0    (free after cycles 1..3: 308302315520, 308260372480, 308260372480)
    this commit (the members free themselves):            0    (free after cycles 1..3: 308300218368, 308258275328, 308258275328)
Both lose the same 41943040 bytes between cycles 1 and 2 (the runtime's own pools) and nothing after.  MARGIN is the parent's figure.
Beyond the calls the cycle must make, the clone's three stores are merged into the root's (dg_*_merge reach into a second context's state)."""
import numpy as np
import pytest
import common
from dart_amd import host

pytestmark = pytest.mark.gpu
MARGIN = 0            # bytes
N_BATCH = 600         # reads per context and cycle (300 pairs)


def fastq_text(reads, first):
    return b"".join(b"@q%d\n%s\n+\n%s\n" % (first + i, r.tobytes(), b"I" * len(r)) for i, r in enumerate(reads))


def one_cycle(case, ix):
    """-> everything the cycle's calls returned, by name"""
    out = {}
    p, _ = common.parse_flags(case["runs"][0]["flags"])
    root = host.DartGPU(ix, host.default_params(paired=1, **p))
    clone = root.clone()
    L = int(ix.chr_len.min())
    root.gene_set_annotation(2, [(0, 100, L // 2, 0, 0), (1, 100, L // 2, 1, 1)])          # (chr, start, end, strand, gene): one exon each
    for k, g in enumerate((root, clone)):
        lo, hi = k * N_BATCH, (k + 1) * N_BATCH
        so, rl, flat = host.pack_reads(case["reads"][lo:hi])
        out["map_batch %d" % k] = g.map_batch(so, rl, flat)
        out["format_sam %d" % k] = g.format_sam(case["headers"][lo:hi], case["quals"][lo:hi], N_BATCH)
        out["format_bam %d" % k] = g.format_bam(case["headers"][lo:hi], case["quals"][lo:hi], N_BATCH, raw=True)
        out["accumulate_sj %d" % k] = g.accumulate_sj()
        out["sj_finish %d" % k] = g.sj_finish()
        out["accumulate_bam %d" % k] = g.accumulate_bam(k)
        out["accumulate_genes %d" % k] = g.accumulate_genes(N_BATCH)
        out["gene_counts %d" % k] = g.gene_counts(4 + 2)
    root.bam_sort_merge(clone); root.sj_merge(clone); root.gene_merge(clone)              # the clone's stores, folded into the root's
    out["merged sj, genes"] = (root.sj_finish(), root.gene_counts())
    n, nb = root.bam_sort_finish()
    out["sorted"] = (n, nb, root.bam_sort_compress(0, nb, raw=True))
    out["markdup"] = root.bam_markdup_finish()
    out["bgzf"] = root.bam_sort_compress(0, nb)
    out["bai"] = root.bam_index_finish(0)
    out["coverage"] = root.bam_coverage_finish()
    for k, g in enumerate((root, clone)):
        pairs = case["reads"][k * N_BATCH:(k + 1) * N_BATCH]
        out["upload_fastq %d" % k] = g.upload_fastq(fastq_text(pairs[0::2], 0), fastq_text(pairs[1::2], 0), rc_odd_reads=True)
    clone.close()
    root.close()
    return out


def same(a, b):
    if isinstance(a, host.BatchResult):
        common.assert_same(a, (b.reads, b.reports, b.cigar, b.sj))
    elif isinstance(a, dict):
        assert list(a) == list(b)
        for k in a:
            same(a[k], b[k])
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            same(x, y)
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b)
    else:
        assert a == b


def test_contexts_free_what_they_own(workdir):
    import torch
    case = common.build_case("pe101_spliced", workdir)
    ix = host.Index(case["prefix"])
    assert len(case["reads"]) >= 2 * N_BATCH
    free, outs = [], []
    for _ in range(3):
        outs.append(one_cycle(case, ix))
        torch.cuda.synchronize(0)
        free.append(torch.cuda.mem_get_info(0)[0])
    print("free device bytes after cycles 1..3: %s; cycle 2 -> 3 lost %d (margin %d)" % (free, free[1] - free[2], MARGIN))
    n_records, n_raw, _ = outs[0]["sorted"]
    assert n_records > N_BATCH and n_raw > 0 and len(outs[0]["coverage"][0]) > 0          # the stages had work: a sorted array, a coverage track
    same(outs[2], outs[0])
    assert free[1] - free[2] <= MARGIN
