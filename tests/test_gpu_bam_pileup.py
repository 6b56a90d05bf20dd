"""GPU suite (-m gpu): the allele counts of the coordinate-sorted BAM, built on the device (dg_bam_pileup_*; dart_amd/csrc/dg_pileup.h).  The expectation is
always the sequential Python twin of tests/pileup_inputs.py over the sorted raw array and the index's own 2-bit text.  No pileup tool is run: the definition in
the header is what is pinned."""
import ctypes as C
import random, re
import numpy as np
import pytest
import common, bam_decode
import bamsort_inputs as bsi
import bamidx_inputs as bii
import pileup_inputs as pui
from dart_amd import host

pytestmark = pytest.mark.gpu
ARG, CAPACITY, RANGE = -3, -4, -6
FIRST = 1234
M = bii.M


class Env:
    pass


def batch(e, g, lo, hi, ordinal, paired=1):
    so, rl, flat = host.pack_reads(e.reads[lo:hi])
    g.set_params(host.default_params(paired=paired, **e.p))
    g.map_batch(so, rl, flat)
    raw, ct = g.format_bam(e.headers[lo:hi], e.quals[lo:hi], hi - lo if paired else 0, raw=True)
    assert g.accumulate_bam(ordinal) == ct["records"]
    return raw


def sorted_raw(g):
    n, nb = g.bam_sort_finish()
    return g.bam_sort_compress(0, nb, raw=True)


def check(e, g, raw, flt=pui.FILTERS[0]):
    """the device's table of the finished store against the twin over `raw` -> (entries as tuples, text, stats)"""
    ent, text = g.bam_pileup_finish(*flt)
    t_ent, t_stats = pui.twin(raw, e.ref, *flt)
    assert ent.dtype == host.SITE_ENTRY == pui.SITE_ENTRY and pui.as_tuples(ent) == t_ent
    assert text == pui.text_of(t_ent, e.names)
    assert g.bam_pileup_stats == t_stats
    return t_ent, text, t_stats


@pytest.fixture(scope="module")
def env(workdir):
    e = Env()
    e.case = common.build_case("pe101_spliced", workdir)
    e.ix = host.Index(e.case["prefix"])
    e.gpu = host.DartGPU(e.ix)
    e.names = [n if isinstance(n, bytes) else n.encode() for n in e.ix.names]
    e.ref = pui.ref_of_index(e.ix)
    assert e.ref.n_chr == len(e.names) == 2
    e.crafted = pui.crafted_cases(e.ref, e.names)
    e.reads, e.headers, e.quals = bsi.sort_reads(e.case)
    e.p, _ = common.parse_flags(["-mis", "5"])
    e.unsorted = {}
    for paired in (1, 0):
        e.gpu.bam_sort_reset()
        e.unsorted[paired] = batch(e, e.gpu, 0, len(e.reads), 0, paired)
    # hand-made records for what the mapper's lack: a secondary, a failed and a duplicate line, each with a mismatch over covered ground, and reads of low quality
    rec = lambda tid, pos, flag, name, mapq=30: pui.rec_on(e.ref, tid, pos, flag, name, [(40, M), (300, bii.N), (40, bii.EQ)], {7: "!", 50: "N"}, mapq)
    e.extra = b"".join([rec(0, 5000, 0x100, b"secondary"), rec(0, 5000, 0x200 | 16, b"qcfail"), rec(0, 5000, 0x400, b"duplicate"), rec(0, 5000, 0, b"mapq0", 0),
                        rec(0, 5000, 0x91, b"mapq3", 3), rec(0, 5000, 0x91, b"mapq30")])
    yield e
    e.gpu.close()


def err_of(call):
    with pytest.raises(RuntimeError) as x:
        call()
    m = re.search(r"failed \((-?\d+)\): (.*)", str(x.value), re.S)
    return int(m.group(1)), m.group(2)


def test_table_equals_the_twin_paired_and_single_for_several_filters_and_agrees_with_the_coverage_track(env):
    e, g = env, env.gpu
    for paired in (1, 0):
        g.bam_sort_reset()
        g.bam_sort_add(e.unsorted[paired], 0); g.bam_sort_add(e.extra, 1)
        raw = sorted_raw(g)
        got = {}
        for flt in ((pui.DEFAULT_EXCLUDE, 0, 2), (pui.DEFAULT_EXCLUDE, 0, 1), (4, 0, 1), (pui.DEFAULT_EXCLUDE, 4, 1), (pui.DEFAULT_EXCLUDE, 0, 3)):
            got[flt] = check(e, g, raw, flt)
            assert g.bam_pileup_device_ms > 0 and len(g.bam_pileup_device_ms_split) == 5 and g.bam_pileup_passes >= 1
            # every kept site's depth is the depth of the coverage entry that contains it, under the same filter
            cov, _ = g.bam_coverage_finish(flt[0], flt[1], entries_only=True)
            starts = {c: np.array([int(x["start"]) for x in cov if x["chr"] == c]) for c in (0, 1)}
            rows = {c: [x for x in cov if x["chr"] == c] for c in (0, 1)}
            for x in got[flt][0]:
                k = int(np.searchsorted(starts[x[0]], x[1], side="right")) - 1
                inside = k >= 0 and int(rows[x[0]][k]["end"]) > x[1]
                assert x[2] == (int(rows[x[0]][k]["depth"]) if inside else 0)
        two, one, dups, mapq, three = (got[k][2] for k in got)
        assert one[0] > 1000 and one[1] > one[0] and one[3] > 500 and one[4] > 0 and one[5] > 0 and one[6] > 500 and one[8] == 0       # real N ops, mismatches, deletions, insertions
        assert one[6] == two[6] == three[6] and one[7] == one[6] > two[7] >= three[7] > 0
        assert dups[0] >= one[0] + 3 and mapq[0] < one[0]
        ent, text = g.bam_pileup_finish(entries_only=True)
        assert pui.as_tuples(ent) == got[pui.DEFAULT_EXCLUDE, 0, 2][0] and text == b""


@pytest.mark.parametrize("name", ["ops", "bases", "seams", "ends", "nothing", "filters", "min_alt", "ties"])
def test_crafted_records_on_the_device(name, env):
    e, g = env, env.gpu
    recs, _ = e.crafted[name]
    rng = random.Random(len(name))
    shuffled = list(recs); rng.shuffle(shuffled)
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(shuffled), 0)
    raw = sorted_raw(g)
    assert sorted(bsi.split(raw)) == sorted(recs)
    for flt in pui.FILTERS:
        ent, _, st = check(e, g, raw, flt)
    if name == "ends":
        assert st[8] == 5            # one base past the chromosome, a D past it, l_seq one short and one long, and the block that ends at 2^32 - 1: tallies, no error


def test_seams_runs_of_equal_keys_across_workgroups_and_sorter_tiles(env):
    e, g = env, env.gpu
    assert g.bam_pileup_granules() == (256, 4096, 16)
    pile = [pui.rec_on(e.ref, 0, 700, 16 if k & 1 else 0, b"p%d" % k, [(30, M), (100, bii.N), (20, M)], {3: "!", 29: "N", 49: "!"}, 9) for k in range(5000)]
    stagger = [pui.rec_on(e.ref, 1, 100 + k, 0, b"s%d" % k, [(101, M)], {1600 - (100 + k): "!"} if 0 <= 1600 - (100 + k) <= 100 else {}, 9) for k in range(1500)]
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(stagger), 1); g.bam_sort_add(b"".join(pile), 0)
    raw = sorted_raw(g)
    ent, text, st = check(e, g, raw)
    # 10000 depth events and 5000 allele events on each of three keys of the pile: runs of equal keys straddle many workgroups and the sorter's tiles
    assert st[1] == 11500 and st[3] == 15000 + 100 and 2 * st[1] + st[3] > 9 * 4096
    assert [x[:4] for x in ent[:3]] == [(0, 703, 5000, 2500), (0, 729, 5000, 2500), (0, 849, 5000, 2500)] and ent[1][5] == pui.N_ and ent[1][6 + pui.N_] == 5000
    assert ent[3][:3] == (1, 1600, 100) and ent[3][6 + ent[3][5]] == 100 and st[9] == 5000 and len(ent) == 4
    # around a workgroup's and a tile's edge: n copies of a read with one mismatch leave 2 n depth events and n allele events, one site
    for n in (85, 86, 255, 256, 257, 1365, 1366, 4096):
        g.bam_sort_reset()
        g.bam_sort_add(b"".join(pui.rec_on(e.ref, 1, 9, 0, b"c%d" % k, [(7, bii.X)], {6: "!"}) for k in range(n)), 0)
        got = check(e, g, sorted_raw(g))[0]
        assert len(got) == 1 and got[0][:4] == (1, 15, n, 0) and got[0][6 + got[0][5]] == n


def test_batches_ordinals_and_contexts_do_not_change_a_byte(env):
    e, g = env, env.gpu
    recs = bsi.split(e.unsorted[1]) + bsi.split(e.extra)
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(recs), 0)
    one = check(e, g, sorted_raw(g), pui.FILTERS[1])
    rng = random.Random(9)
    shuffled = list(recs); rng.shuffle(shuffled)
    cuts = [0, len(recs) // 5, len(recs) // 2, len(recs)]
    g.bam_sort_reset()
    for k, ordinal in enumerate((2, 0, 1)):
        g.bam_sort_add(b"".join(shuffled[cuts[k]:cuts[k + 1]]), ordinal)
    sorted_raw(g)
    ent, text = g.bam_pileup_finish(*pui.FILTERS[1])
    assert (pui.as_tuples(ent), text, g.bam_pileup_stats) == one
    assert g.bam_pileup_finish(*pui.FILTERS[1])[1] == text                     # a repeated call
    assert len(g.bam_pileup_finish(*pui.FILTERS[0])[1]) < len(text)            # and one with another filter
    clone = g.clone()
    try:
        g.bam_sort_reset(); clone.bam_sort_reset()
        clone.bam_sort_add(b"".join(shuffled[:cuts[2]]), 1); g.bam_sort_add(b"".join(shuffled[cuts[2]:]), 0)
        g.bam_sort_merge(clone)
        sorted_raw(g)
        ent, text = g.bam_pileup_finish(*pui.FILTERS[1])
        assert (pui.as_tuples(ent), text, g.bam_pileup_stats) == one
        clone.bam_sort_add(e.unsorted[0], 0)
        check(e, clone, sorted_raw(clone))
    finally:
        clone.close()


def test_before_between_and_after_the_other_stages_and_behind_the_duplicate_marking(env):
    e, g = env, env.gpu
    g.bam_sort_reset()
    g.bam_sort_add(e.unsorted[1], 0); g.bam_sort_add(e.extra, 1)
    n, nb = g.bam_sort_finish()
    before = g.bam_pileup_finish()
    z = g.bam_sort_compress(0, nb)
    between = g.bam_pileup_finish()
    bai = g.bam_index_finish(FIRST)
    cov = g.bam_coverage_finish()
    after = g.bam_pileup_finish(min_alt=1)
    after = g.bam_pileup_finish()
    assert before[1] == between[1] == after[1] and len(before[1]) > 100
    raw = g.bam_sort_compress(0, nb, raw=True)
    assert before[1] == pui.text_of(pui.twin(raw, e.ref)[0], e.names)
    # the finished index and the finished track are still there, and the same bytes
    buf = np.zeros(len(bai), np.uint8)
    assert g.lib.dg_bam_index_download(g.ctx, buf.ctypes.data, len(bai)) == 0 and buf.tobytes() == bai
    tbuf = np.zeros(len(cov[1]), np.uint8)
    assert g.lib.dg_bam_coverage_download(g.ctx, None, 0, tbuf.ctypes.data, len(tbuf)) == 0 and tbuf.tobytes() == cov[1]
    assert g.bam_sort_compress(0, nb) == z and g.bam_index_finish(FIRST) == bai        # the recorded sizes and the places were not disturbed
    # duplicates drop out: the copies of pair 0 are marked, and the table sees the marks
    g.bam_sort_reset()
    g.bam_sort_add(e.unsorted[1], 0)
    n, nb = g.bam_sort_finish()
    raw = g.bam_sort_compress(0, nb, raw=True)
    counted = check(e, g, raw)[2][0]
    md = g.bam_markdup_finish()
    assert md[6] >= 6
    buf = np.zeros(64, np.uint8)
    assert g.lib.dg_bam_pileup_download(g.ctx, buf.ctypes.data, 0, None, 0) == ARG           # the marking forgets the table, as it forgets the index and the track
    marked = g.bam_sort_compress(0, nb, raw=True)
    assert marked != raw
    ent, text, st = check(e, g, marked)
    assert st[0] == counted - md[6]
    assert check(e, g, marked, (4, 0, 2))[2][0] == counted


def _still_works(e, g):
    """after a refused call: the context maps a batch, keeps it, sorts it and counts its alleles"""
    g.bam_sort_reset()
    batch(e, g, 0, 400, 0)
    assert check(e, g, sorted_raw(g), pui.FILTERS[1])[2][0] > 100


def test_empty_store_and_refusals(env):
    e = env
    g = e.gpu.clone()
    try:
        rc, msg = err_of(lambda: g.bam_pileup_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg
        _still_works(e, g)
        g.bam_sort_reset()
        assert g.bam_sort_finish() == (0, 0)
        ent, text = g.bam_pileup_finish()
        assert len(ent) == 0 and text == b"" and g.bam_pileup_stats == (0,) * 10
        # records that all count for nothing, and records without any allele event
        g.bam_sort_add(pui.record(-1, -1, 4, b"u", [], "ACGTA") + pui.rec_on(e.ref, 0, 3, 0x400, b"dup", [(5, M)], {2: "!"}) + pui.rec_on(e.ref, 0, 30, 0, b"clean", [(5, M)]), 0)
        raw = sorted_raw(g)
        assert check(e, g, raw, pui.FILTERS[1])[2] == (1, 1, 5, 0, 0, 0, 0, 0, 0, 0)
        assert [x[:3] for x in check(e, g, raw, (4, 0, 1))[0]] == [(0, 5, 1)]
        # a store call behind the finish
        g.bam_sort_add(pui.rec_on(e.ref, 0, 3, 0, b"late", [(5, M)]), 1)
        rc, msg = err_of(lambda: g.bam_pileup_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg
        buf = np.zeros(256, np.uint8)
        assert g.lib.dg_bam_pileup_download(g.ctx, buf.ctypes.data, 4, None, 0) == ARG
        _still_works(e, g)
        # a flag bit nobody defined; min_alt 0
        assert g.lib.dg_bam_pileup_finish(g.ctx, 2, 0, 0, 1, None, None, None, None) == ARG
        assert g.lib.dg_bam_pileup_finish(g.ctx, 0, 0, 0, 0, None, None, None, None) == ARG and b"min_alt" in g.lib.dg_last_error(g.ctx)
        # a short download: nothing written
        ent, text = g.bam_pileup_finish(min_alt=1)
        assert len(ent) > 3 and len(text) > 256
        assert g.lib.dg_bam_pileup_download(g.ctx, buf.ctypes.data, len(ent) - 1, None, 0) == CAPACITY and not buf.any()
        assert g.lib.dg_bam_pileup_download(g.ctx, None, 0, buf.ctypes.data, len(text) - 1) == CAPACITY and not buf.any()
        assert g.lib.dg_bam_pileup_download(g.ctx, None, 0, None, 0) == 0
        pe = C.c_void_p(); pt = C.c_void_p()
        assert g.lib.dg_bam_pileup_device(g.ctx, C.byref(pe), C.byref(pt)) == 0 and pe.value and pt.value
        # a block that ends behind 2^32 - 1: refused with the record's index, nothing left behind; the sorted array still compresses
        recs, _ = e.crafted["ends_bad"]
        names = [r[36:36 + r[12] - 1] for r in recs]
        g.bam_sort_reset()
        g.bam_sort_add(b"".join(recs), 0)
        n, nb = g.bam_sort_finish()
        rc, msg = err_of(lambda: g.bam_pileup_finish())
        assert rc == RANGE and "record %d " % names.index(b"ends_at_2_32") in msg
        rc, msg = err_of(lambda: g.bam_pileup_finish(exclude=4))
        assert rc == RANGE and "record %d " % names.index(b"a_duplicate_out_of_range") in msg
        assert g.lib.dg_bam_pileup_download(g.ctx, buf.ctypes.data, 4, None, 0) == ARG
        assert g.bam_sort_compress(0, nb, raw=True) == b"".join(recs)
        assert len(g.bam_sort_compress(0, nb)) > 28
        _still_works(e, g)
    finally:
        g.close()
    # text without names: DG_ERR_ARG; with the entries-only flag it works (a context made through the C calls alone: DartGPU sets the names itself)
    lib = e.gpu.lib
    st = C.c_int(0)
    f = e.ix.files(0)
    raw_ctx = lib.dg_init_files(C.byref(f), C.byref(host.default_params(paired=0)), 0, 0, C.byref(st))
    assert raw_ctx
    try:
        data = np.frombuffer(pui.rec_on(e.ref, 1, 40, 0, b"r", [(6, M)], {2: "!"}) + b"\0", np.uint8)
        n = C.c_size_t(0); nb = C.c_size_t(0); ne = C.c_size_t(0)
        assert lib.dg_bam_sort_add(raw_ctx, data.ctypes.data, len(data) - 1, 0, C.byref(n)) == 0 and n.value == 1
        assert lib.dg_bam_sort_finish(raw_ctx, C.byref(n), C.byref(nb), None) == 0
        assert lib.dg_bam_pileup_finish(raw_ctx, 0, 0x704, 0, 1, C.byref(ne), C.byref(nb), None, None) == ARG and b"names" in lib.dg_last_error(raw_ctx)
        assert lib.dg_bam_pileup_finish(raw_ctx, host.PU_ENTRIES_ONLY, 0x704, 0, 1, C.byref(ne), C.byref(nb), None, None) == 0 and (ne.value, nb.value) == (1, 0)
        ent = np.zeros(1, host.SITE_ENTRY)
        assert lib.dg_bam_pileup_download(raw_ctx, ent.ctypes.data, 1, None, 0) == 0 and pui.as_tuples(ent)[0][:4] == (1, 42, 1, 0)
    finally:
        lib.dg_destroy(raw_ctx)


def test_planted_variants_are_kept_sites_with_the_planted_allele_on_top(env):
    """reads from a copy of the genome with 20 SNVs, one 3-base deletion and one 2-base insertion at about 20x, mapped at -mis 5: device == twin, and every
    planted variant whose twin depth is at least 4 is a kept site with the planted allele as top.  The share that reaches depth 4 is a condition: three quarters.
    (On the CPU oracle's alignments run through the twin: 22 planted, 21 reach depth 4 and all 21 are recovered; the reads that span the deletion are left
    unaligned or soft-clipped by the mapper, so its positions have no depth.)"""
    e, g = env, env.gpu
    variants, reads = pui.planted_case(e.ref)
    n = len(reads)
    so, rl, flat = host.pack_reads(reads)
    g.bam_sort_reset()
    g.set_params(host.default_params(paired=0, **e.p))
    g.map_batch(so, rl, flat)
    _, ct = g.format_bam(["p%d" % i for i in range(n)], ["I" * reads.shape[1]] * n, 0, raw=True)
    assert g.accumulate_bam(0) == ct["records"]
    raw = sorted_raw(g)
    ent, text, st = check(e, g, raw)
    deep, found = pui.planted_found(raw, e.ref, ent, variants)
    print("planted %d, depth >= 4: %d, recovered: %d; stats %s" % (len(variants), len(deep), len(found), st))
    assert len(variants) == 22 and sorted(v[0] for v in variants) == ["del", "ins"] + ["snv"] * 20
    assert 4 * len(deep) >= 3 * len(variants)
    assert found == deep
