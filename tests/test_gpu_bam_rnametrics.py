"""GPU suite (-m gpu): the RNA-seq metrics of the coordinate-sorted BAM, built on the device (dg_rna_set_annotation, dg_bam_rna_*; dart_amd/csrc/dg_rnametrics.h).
The expectation is always the sequential Python twin of tests/rnametrics_inputs.py over the sorted raw array.  No Picard or RSeQC is run: the definition in the
header is what is pinned."""
import ctypes as C
import os, random, re
import numpy as np
import pytest
import common
import bamsort_inputs as bsi
import rnametrics_inputs as rmi
from rnametrics_inputs import SN, M
from dart_amd import host

pytestmark = pytest.mark.gpu
ARG, CAPACITY, RANGE = -3, -4, -6
ANNOT = rmi.crafted_annotation()
CASES = rmi.crafted_cases()
EVERYTHING = [r for name in sorted(CASES) for r in CASES[name]]


class Env:
    pass


def use(g, annot):
    """uploads the annotation for g's index -> (segments, eligible)"""
    return g.rna_set_annotation(*rmi.pack(annot))


def sorted_raw(g):
    n, nb = g.bam_sort_finish()
    return g.bam_sort_compress(0, nb, raw=True)


def load(g, recs, shuffle_seed=None):
    recs = list(recs)
    if shuffle_seed is not None:
        random.Random(shuffle_seed).shuffle(recs)
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(recs), 0)
    return sorted_raw(g)


def check(g, raw, annot, flt=rmi.FILTERS[0], min_cov=rmi.DEFAULT_MIN_COV):
    """the device's words of the finished store against the twin over `raw` -> the views"""
    got = g.bam_rna_finish(*flt, min_cov)
    want = rmi.twin(raw, 2, annot, *flt, min_cov)
    assert got["words"].dtype == np.uint64 and len(got["words"]) == len(want)
    assert np.array_equal(got["words"], want), [(int(k), int(got["words"][k]), int(want[k])) for k in np.flatnonzero(got["words"] != want)[:10]]
    assert g.bam_rna_text(got) == rmi.text_of(want)
    for name, v in rmi.views(want).items():
        assert got[name].shape == v.shape and np.array_equal(got[name], v)
    return got


def with_groups(e, groups):
    """a context of its own that read DG_RNA_MAX_GROUPS = groups at its start (None: the default grid)"""
    old = os.environ.pop("DG_RNA_MAX_GROUPS", None)
    if groups is not None:
        os.environ["DG_RNA_MAX_GROUPS"] = str(groups)
    try:
        return host.DartGPU(e.ix)
    finally:
        os.environ.pop("DG_RNA_MAX_GROUPS", None)
        if old is not None:
            os.environ["DG_RNA_MAX_GROUPS"] = old


def err_of(call):
    with pytest.raises(RuntimeError) as x:
        call()
    m = re.search(r"failed \((-?\d+)\): (.*)", str(x.value), re.S)
    return int(m.group(1)), m.group(2)


@pytest.fixture(scope="module")
def env(workdir):
    e = Env()
    e.case = common.build_case("pe101_spliced", workdir)
    e.ix = host.Index(e.case["prefix"])
    e.gpu = host.DartGPU(e.ix)
    assert len(e.ix.names) == 2
    e.reads, e.headers, e.quals = bsi.sort_reads(e.case)
    e.p, _ = common.parse_flags(["-mis", "5"])
    so, rl, flat = host.pack_reads(e.reads)
    e.gpu.set_params(host.default_params(paired=1, **e.p))
    e.gpu.map_batch(so, rl, flat)
    e.gpu.bam_sort_reset()
    e.unsorted, ct = e.gpu.format_bam(e.headers, e.quals, len(e.reads), raw=True)
    assert e.gpu.accumulate_bam(0) == ct["records"]
    e.case_annot = rmi.case_annotation(e.case, rmi.CASE_SEEDS["pe101_spliced"])
    yield e
    e.gpu.close()


@pytest.mark.parametrize("name", sorted(CASES) + ["everything"])
def test_crafted_records_on_the_device(name, env):
    e, g = env, env.gpu
    recs = EVERYTHING if name == "everything" else CASES[name]
    assert use(g, ANNOT) == (sum(len(s[0]) for s in rmi.flatten(ANNOT, 2)[0]), 6)
    raw = load(g, recs, shuffle_seed=len(name))
    assert sorted(bsi.split(raw)) == sorted(recs)
    for flt in rmi.FILTERS:
        v = check(g, raw, ANNOT, flt, min_cov=1)
    assert g.bam_rna_device_ms > 0 and len(g.bam_rna_device_ms_split) == 3 and g.bam_rna_granules() == (256, 4)
    if name == "everything":
        words, sums = rmi.twin(raw, 2, ANNOT, want_sums=True)
        S = sorted(set(s for s in sums if s > 1))[0]
        n_at = lambda mc: int(check(g, raw, ANNOT, min_cov=mc)["SN"][SN["contributing_transcripts"]])
        assert n_at(S - 1) == n_at(S) == n_at(S + 1) + 1 and n_at(0) == n_at(1) == sum(1 for s in sums if s > 0) and 0 in sums and n_at(1 << 40) == 0
        assert np.array_equal(rmi.paint(raw, 2, ANNOT), words)


def test_counts_grids_and_transcript_counts_give_identical_words(env):
    e = env
    many = lambda n: [EVERYTHING[k % len(EVERYTHING)] for k in range(n)]
    per = {}
    for groups in (1, 2, None):
        g = with_groups(e, groups)
        try:
            use(g, ANNOT)
            for n in (255, 256, 257, 513):                            # record runs and event runs (two per block) straddle workgroups
                raw = load(g, many(n))
                per[groups, n] = check(g, raw, ANNOT, min_cov=1)["words"]
            raw = load(g, many(257))
            for keep in ([3, 5, 6], [3, 5, 6, 7], [0, 3, 5, 6, 7], list(range(11)) * 2):      # 3, 4, 5 and 12 eligible transcripts: a workgroup of k_rm_body takes 4 a trip
                annot = [ANNOT[k] for k in keep]
                assert use(g, annot)[1] == len(rmi.flatten(annot, 2)[1])
                per[groups, "tx", len(keep)] = check(g, raw, annot, min_cov=1)["words"]
        finally:
            g.close()
    for key in [k for k in per if k[0] is None]:
        assert np.array_equal(per[key], per[(1,) + key[1:]]) and np.array_equal(per[key], per[(2,) + key[1:]])


def test_order_batches_ordinals_and_contexts_do_not_change_a_word(env):
    e, g = env, env.gpu
    recs = bsi.split(e.unsorted) + EVERYTHING
    use(g, e.case_annot)
    flt = rmi.FILTERS[1]
    one = check(g, load(g, recs), e.case_annot, flt, min_cov=5)["words"]
    shuffled = list(recs); random.Random(9).shuffle(shuffled)
    cuts = [0, len(recs) // 5, len(recs) // 2, len(recs)]
    g.bam_sort_reset()
    for k, ordinal in enumerate((2, 0, 1)):
        g.bam_sort_add(b"".join(shuffled[cuts[k]:cuts[k + 1]]), ordinal)
    sorted_raw(g)
    assert np.array_equal(g.bam_rna_finish(*flt, 5)["words"], one)
    assert np.array_equal(g.bam_rna_finish(*flt, 5)["words"], one)                               # a repeated call
    assert not np.array_equal(g.bam_rna_finish(*rmi.FILTERS[3], 5)["words"], one)                # and one with another filter
    clone = g.clone()
    try:
        g.bam_sort_reset(); clone.bam_sort_reset()
        clone.bam_sort_add(b"".join(shuffled[:cuts[2]]), 1); g.bam_sort_add(b"".join(shuffled[cuts[2]:]), 0)
        clone.bam_sort_finish()
        assert clone.bam_rna_finish(*flt, 5)["SN"][SN["records"]] == cuts[2]                     # the clone shares the index's annotation
        g.bam_sort_merge(clone)
        sorted_raw(g)
        assert np.array_equal(g.bam_rna_finish(*flt, 5)["words"], one)
    finally:
        clone.close()


def test_mappers_records_behind_marking_and_tagging_and_beside_the_other_stages(env):
    e, g = env, env.gpu
    annot = e.case_annot
    use(g, annot)
    g.bam_sort_reset()
    g.bam_sort_add(e.unsorted, 0); g.bam_sort_add(e.unsorted, 1)                                 # every record twice: the marking finds duplicates
    n, nb = g.bam_sort_finish()
    raw = g.bam_sort_compress(0, nb, raw=True)
    words, sums = rmi.twin(raw, 2, annot, min_cov=rmi.CASE_MIN_COV, want_sums=True)
    assert rmi.rich_enough(words, sums, annot, 2)                                                # every class, every strand row, ten contributing transcripts a strand
    before = check(g, raw, annot, (0x400 | 4, 0), rmi.CASE_MIN_COV)
    # the other stages, built before the call, are what they were behind it
    z = g.bam_sort_compress(0, nb); bai = g.bam_index_finish(1234)
    cov = g.bam_coverage_finish(); qc = g.bam_qc_finish()["words"].copy()
    check(g, raw, annot, min_cov=rmi.CASE_MIN_COV)
    assert g.bam_sort_compress(0, nb, raw=True) == raw and g.bam_sort_compress(0, nb) == z and g.bam_index_finish(1234) == bai
    ent, text = g.bam_coverage_finish()
    assert text == cov[1] and np.array_equal(ent, cov[0]) and np.array_equal(g.bam_qc_finish()["words"], qc)
    st = g.bam_coverage_stats
    d = g.bam_rna_finish(0x704, 0, rmi.CASE_MIN_COV)                                             # the coverage track's filter: its records, blocks and aligned bases
    assert (int(d["SN"][SN["counted"]]), int(d["SN"][SN["blocks"]]), int(d["SN"][SN["aligned_bases"]])) == (st[0], st[1], st[5])
    # behind the duplicate marking it sees the marks
    md = g.bam_markdup_finish()
    assert md[6] > 0
    buf = np.zeros(400, np.uint64)
    assert g.lib.dg_bam_rna_download(g.ctx, buf.ctypes.data, len(buf)) == ARG                    # the marking changes flags: it forgets the words
    marked = g.bam_sort_compress(0, nb, raw=True)
    after = check(g, marked, annot, (0x400 | 4, 0), rmi.CASE_MIN_COV)
    assert int(before["SN"][SN["counted"]]) - int(after["SN"][SN["counted"]]) == md[6]
    # the tagged array gives the untagged array's words
    g.bam_tags_finish()
    assert np.array_equal(g.bam_rna_finish(0x400 | 4, 0, rmi.CASE_MIN_COV)["words"], after["words"])


def test_refusals(env):
    e = env
    fresh = host.DartGPU(e.ix)                                                                   # an index of its own: no annotation yet
    try:
        fresh.bam_sort_add(b"".join(CASES["edges"]), 0)
        fresh.bam_sort_finish()
        rc, msg = err_of(lambda: fresh.bam_rna_finish())
        assert rc == ARG and "dg_rna_set_annotation" in msg
        for rule, annot in rmi.bad_annotations():
            rc, msg = err_of(lambda: use(fresh, annot))
            assert rc == ARG and "transcript 1 " in msg and rule in msg, (rule, msg)
        rc, msg = err_of(lambda: use(fresh, []))
        assert rc == ARG
        t, ex = rmi.pack([rmi.tx(0, 0, [(10, 20)]), rmi.tx(0, 0, [(30, 40), (50, 60)])])
        rc, msg = err_of(lambda: fresh.rna_set_annotation(t, ex[:2]))
        assert rc == ARG and "outside the exon array" in msg
        rc, msg = err_of(lambda: fresh.bam_rna_finish())                                         # a refused annotation is none
        assert rc == ARG and "dg_rna_set_annotation" in msg
        use(fresh, ANNOT)
        first = fresh.bam_rna_finish()["words"]
        use(fresh, ANNOT[3:])                                                                    # a second call replaces the tables
        assert not np.array_equal(fresh.bam_rna_finish()["words"], first)
        assert np.array_equal(fresh.bam_rna_finish()["words"], rmi.twin(b"".join(sorted(CASES["edges"], key=lambda r: bsi.key(r, 2))), 2, ANNOT[3:]))
    finally:
        fresh.close()
    use(e.gpu, ANNOT)
    g = e.gpu.clone()
    try:
        rc, msg = err_of(lambda: g.bam_rna_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg
        buf = np.zeros(400, np.uint64)
        assert g.lib.dg_bam_rna_download(g.ctx, buf.ctypes.data, len(buf)) == ARG
        g.bam_sort_reset()
        assert g.bam_sort_finish() == (0, 0)
        v = g.bam_rna_finish()                                                                   # an empty store: zero BA, RC, ST and BC
        assert not v["words"][:314].any() and v["SN"].tolist() == [0, 0, 0, 0, 11, 6, 0, sum(len(s[0]) for s in rmi.flatten(ANNOT, 2)[0])] + [0] * 8
        raw = load(g, CASES["strands"])
        assert g.lib.dg_bam_rna_finish(g.ctx, 1, 0x904, 0, 100, None, None) == ARG and b"flags" in g.lib.dg_last_error(g.ctx)      # a flag bit nobody defined
        assert g.lib.dg_bam_rna_download(g.ctx, buf.ctypes.data, len(buf)) == ARG                # the refused call left no words
        want = check(g, raw, ANNOT)["words"]
        assert g.lib.dg_bam_rna_download(g.ctx, buf.ctypes.data, len(want) - 1) == CAPACITY and not buf.any()               # one word short: nothing written
        assert g.lib.dg_bam_rna_download(g.ctx, buf.ctypes.data, len(want)) == 0 and np.array_equal(buf[:len(want)], want) and not buf[len(want):].any()
        p = C.c_void_p()
        assert g.lib.dg_bam_rna_device(g.ctx, C.byref(p)) == 0 and p.value
        g.bam_sort_add(CASES["edges"][0], 1)                                                     # a store call behind the finish
        rc, msg = err_of(lambda: g.bam_rna_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg
        # a block that ends behind 2^32 - 1: DG_ERR_RANGE names the record, no words are left, and the context works on
        ok, bad = rmi.range_cases()
        raw = load(g, ok)
        assert check(g, raw, ANNOT)["BA"][0] == 13
        load(g, bad)
        rc, msg = err_of(lambda: g.bam_rna_finish())
        assert rc == RANGE and "record 1 " in msg
        assert g.lib.dg_bam_rna_download(g.ctx, buf.ctypes.data, len(buf)) == ARG
        rc, msg = err_of(lambda: g.bam_rna_finish(0x404))                                        # with the duplicate left out it is the next one
        assert rc == RANGE and "record 2 " in msg
        check(g, load(g, CASES["depth"]), ANNOT, min_cov=1)
    finally:
        g.close()
