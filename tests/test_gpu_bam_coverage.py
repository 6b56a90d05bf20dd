"""GPU suite (-m gpu): the coverage track of the coordinate-sorted BAM, built on the device (dg_bam_coverage_*; dart_amd/csrc/dg_coverage.h).  The expectation is
always the sequential Python twin of tests/coverage_inputs.py over the sorted raw array.  No bedtools or samtools is run: the definition in the header is what
is pinned."""
import ctypes as C
import random, re
import numpy as np
import pytest
import common, bam_decode
import bamsort_inputs as bsi
import bamidx_inputs as bii
import coverage_inputs as cvi
from dart_amd import host

pytestmark = pytest.mark.gpu
BLOCK = bii.BLOCK
ARG, CAPACITY, RANGE = -3, -4, -6
FIRST = 1234


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


def check(e, g, raw, flt=cvi.FILTERS[0]):
    """the device's track of the finished store against the twin over `raw` -> (entries as tuples, text, stats)"""
    ent, text = g.bam_coverage_finish(*flt)
    t_ent, t_stats = cvi.twin(raw, e.n_chr, *flt)
    assert ent.dtype == host.COV_ENTRY and ent.tolist() == t_ent
    assert text == cvi.text_of(t_ent, e.names)
    assert g.bam_coverage_stats == t_stats
    assert g.bam_coverage_stats[5] == sum(int(x["depth"]) * (int(x["end"]) - int(x["start"])) for x in ent)
    return t_ent, text, t_stats


@pytest.fixture(scope="module")
def env(workdir):
    e = Env()
    e.case = common.build_case("pe101_spliced", workdir)
    e.ix = host.Index(e.case["prefix"])
    e.gpu = host.DartGPU(e.ix)
    e.names = [n if isinstance(n, bytes) else n.encode() for n in e.ix.names]
    e.n_chr = len(e.names)
    assert e.n_chr == 2
    e.reads, e.headers, e.quals = bsi.sort_reads(e.case)
    e.p, _ = common.parse_flags(e.case["runs"][0]["flags"])
    e.unsorted = {}
    for paired in (1, 0):
        e.gpu.bam_sort_reset()
        e.unsorted[paired] = batch(e, e.gpu, 0, len(e.reads), 0, paired)
    # hand-made records for what the mapper's lack: a secondary, a failed and a duplicate line over covered ground, and two reads of low mapping quality
    rec = lambda tid, pos, flag, name, mapq=30: bii.record(tid, pos, flag, name, [(40, bii.M), (300, bii.N), (40, bii.EQ)], l_seq=80, mapq=mapq)
    e.extra = b"".join([rec(0, 5000, 0x100, b"secondary"), rec(0, 5010, 0x200 | 16, b"qcfail"), rec(1, 5020, 0x400, b"duplicate"), rec(1, 5030, 0, b"mapq0", 0),
                        rec(0, 5040, 0x91, b"mapq3", 3)])
    yield e
    e.gpu.close()


def err_of(call):
    with pytest.raises(RuntimeError) as x:
        call()
    m = re.search(r"failed \((-?\d+)\): (.*)", str(x.value), re.S)
    return int(m.group(1)), m.group(2)


def test_track_equals_the_twin_paired_and_single_for_every_filter(env):
    e, g = env, env.gpu
    for paired in (1, 0):
        g.bam_sort_reset()
        g.bam_sort_add(e.unsorted[paired], 0); g.bam_sort_add(e.extra, 1)
        raw = sorted_raw(g)
        got = {}
        for flt in ((cvi.DEFAULT_EXCLUDE, 0, None), (4, 0, None), (cvi.DEFAULT_EXCLUDE, 4, None), (cvi.DEFAULT_EXCLUDE, 0, "+"), (cvi.DEFAULT_EXCLUDE, 0, "-")):
            got[flt[0], flt[1], flt[2]] = check(e, g, raw, flt)
            assert g.bam_coverage_device_ms > 0 and len(g.bam_coverage_device_ms_split) == 5 and g.bam_coverage_passes >= 1
        dflt, dups, mapq, plus, minus = (got[k][2] for k in got)
        assert dflt[1] > dflt[0] > 1000 and dflt[6] >= 2 and dflt[3] > 500          # real N ops: more blocks than records; reads that overlap
        assert dups[0] >= dflt[0] + 3 and 0 < mapq[0] < dflt[0]                    # the three excluded lines count with exclude = 4; low qualities drop out
        assert plus[5] + minus[5] == dflt[5] and plus[0] + minus[0] == dflt[0] and plus[0] > 0 and minus[0] > 0
        assert len({got[k][1] for k in got}) == 5
        # entries only: the same entries, no text
        ent, text = g.bam_coverage_finish(entries_only=True)
        assert ent.tolist() == got[cvi.DEFAULT_EXCLUDE, 0, None][0] and text == b""


@pytest.mark.parametrize("name", ["cigar", "depth", "edge", "nothing", "filters"])
def test_crafted_records_on_the_device(name, env):
    e, g = env, env.gpu
    n_chr, recs, _ = cvi.crafted_cases()[name]
    assert n_chr == e.n_chr
    rng = random.Random(len(name))
    shuffled = list(recs); rng.shuffle(shuffled)
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(shuffled), 0)
    raw = sorted_raw(g)
    assert sorted(bsi.split(raw)) == sorted(recs)
    for flt in cvi.FILTERS:
        check(e, g, raw, flt)


def test_seams_runs_of_equal_keys_across_workgroups_and_sorter_tiles(env):
    e, g = env, env.gpu
    g0, g1 = g.bam_coverage_granules()
    assert (g0, g1) == (256, 4096)
    pile = [bii.record(0, 700, 16 if k & 1 else 0, b"p%d" % k, [(30, bii.M), (100, bii.N), (20, bii.M)], l_seq=50, mapq=9) for k in range(5000)]
    stagger = [bii.record(1, 100 + k, 0, b"s%d" % k, [(101, bii.M)], l_seq=101, mapq=9) for k in range(1500)]
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(stagger), 1); g.bam_sort_add(b"".join(pile), 0)
    raw = sorted_raw(g)
    ent, text, st = check(e, g, raw)
    assert st[1] == 11500 and 2 * st[1] > 5 * g1                   # events in six tiles of the sorter, ninety workgroups
    assert ent[:2] == [(0, 700, 730, 5000), (0, 830, 850, 5000)] and st[6] == 5000 and st[2] == 4 + 101 + 101      # (a staggered read begins where another ends: no breakpoint there)
    assert max(d for c, _, _, d in ent if c == 1) == 101
    assert text.startswith(e.names[0] + b"\t700\t730\t5000\n")
    # around a workgroup's and a tile's edge: n copies of a one-block record leave 2 n events, two breakpoints, one entry
    for n in (g0 // 2 - 1, g0 // 2, g0 // 2 + 1, g1 // 2, g1 // 2 + 1):
        g.bam_sort_reset()
        g.bam_sort_add(b"".join(bii.record(1, 9, 0, b"c%d" % k, [(7, bii.X)], l_seq=7) for k in range(n)), 0)
        assert check(e, g, sorted_raw(g))[0] == [(1, 9, 16, n)]


def test_batches_ordinals_and_contexts_do_not_change_a_byte(env):
    e, g = env, env.gpu
    recs = bsi.split(e.unsorted[1]) + bsi.split(e.extra)
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(recs), 0)
    one = check(e, g, sorted_raw(g))
    rng = random.Random(9)
    shuffled = list(recs); rng.shuffle(shuffled)
    cuts = [0, len(recs) // 5, len(recs) // 2, len(recs)]
    g.bam_sort_reset()
    for k, ordinal in enumerate((2, 0, 1)):
        g.bam_sort_add(b"".join(shuffled[cuts[k]:cuts[k + 1]]), ordinal)
    raw3 = sorted_raw(g)
    ent, text = g.bam_coverage_finish()
    assert (ent.tolist(), text, g.bam_coverage_stats) == one
    assert g.bam_coverage_finish()[1] == text                     # a repeated call
    clone = g.clone()
    try:
        g.bam_sort_reset(); clone.bam_sort_reset()
        clone.bam_sort_add(b"".join(shuffled[:cuts[2]]), 1); g.bam_sort_add(b"".join(shuffled[cuts[2]:]), 0)
        g.bam_sort_merge(clone)
        sorted_raw(g)
        ent, text = g.bam_coverage_finish()
        assert (ent.tolist(), text, g.bam_coverage_stats) == one
        # the clone covers too, and a context's track does not depend on what it covered before
        clone.bam_sort_add(e.unsorted[0], 0)
        check(e, clone, sorted_raw(clone))
    finally:
        clone.close()


def test_before_between_and_after_compress_and_index(env):
    e, g = env, env.gpu
    g.bam_sort_reset()
    g.bam_sort_add(e.unsorted[1], 0); g.bam_sort_add(e.extra, 1)
    n, nb = g.bam_sort_finish()
    before = g.bam_coverage_finish()
    z = g.bam_sort_compress(0, nb)
    between = g.bam_coverage_finish()
    bai = g.bam_index_finish(FIRST)
    after = g.bam_coverage_finish(strand="-")
    after = g.bam_coverage_finish()
    assert before[1] == between[1] == after[1] and len(before[1]) > 1000
    assert before[0].tolist() == between[0].tolist() == after[0].tolist()
    raw = g.bam_sort_compress(0, nb, raw=True)
    assert before[1] == cvi.text_of(cvi.twin(raw, e.n_chr)[0], e.names)
    # the finished index is still there, and the same bytes
    buf = np.zeros(len(bai), np.uint8)
    assert g.lib.dg_bam_index_download(g.ctx, buf.ctypes.data, len(bai)) == 0 and buf.tobytes() == bai
    assert bai == bii.build_bai(raw, [s for _, s in bam_decode.bgzf_blocks(z)], FIRST, e.n_chr)
    assert g.bam_sort_compress(0, nb) == z and g.bam_index_finish(FIRST) == bai        # the recorded sizes and the places were not disturbed


def _still_covers(e, g):
    """after a refused call: the context maps a batch, keeps it, sorts it and covers it"""
    g.bam_sort_reset()
    batch(e, g, 0, 400, 0)
    assert check(e, g, sorted_raw(g))[2][0] > 100


def test_empty_store_and_refusals(env):
    e = env
    g = e.gpu.clone()
    try:
        # no finish at all on a fresh context
        rc, msg = err_of(lambda: g.bam_coverage_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg
        _still_covers(e, g)
        # an empty store
        g.bam_sort_reset()
        assert g.bam_sort_finish() == (0, 0)
        ent, text = g.bam_coverage_finish()
        assert len(ent) == 0 and text == b"" and g.bam_coverage_stats == (0,) * 7
        # records that all count for nothing
        g.bam_sort_add(bii.record(-1, -1, 4, b"u", l_seq=5) + bii.record(0, 3, 0x400, b"dup", [(5, bii.M)], l_seq=5), 0)
        raw = sorted_raw(g)
        assert check(e, g, raw)[2] == (0,) * 7
        assert check(e, g, raw, (4, 0, None))[0] == [(0, 3, 8, 1)]
        # a store call behind the finish
        g.bam_sort_add(bii.record(0, 3, 0, b"late", [(5, bii.M)], l_seq=5), 1)
        rc, msg = err_of(lambda: g.bam_coverage_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg
        buf = np.zeros(64, np.uint8)
        assert g.lib.dg_bam_coverage_download(g.ctx, buf.ctypes.data, 4, None, 0) == ARG
        _still_covers(e, g)
        # a flag bit nobody defined
        assert g.lib.dg_bam_coverage_finish(g.ctx, 8, 0, 0, None, None, None, None) == ARG
        # a short download: nothing written
        ent, text = g.bam_coverage_finish()
        assert len(ent) > 4 and len(text) > 64
        assert g.lib.dg_bam_coverage_download(g.ctx, buf.ctypes.data, len(ent) - 1, None, 0) == CAPACITY and not buf.any()
        assert g.lib.dg_bam_coverage_download(g.ctx, None, 0, buf.ctypes.data, len(text) - 1) == CAPACITY and not buf.any()
        assert g.lib.dg_bam_coverage_download(g.ctx, None, 0, None, 0) == 0
        pe = C.c_void_p(); pt = C.c_void_p()
        assert g.lib.dg_bam_coverage_device(g.ctx, C.byref(pe), C.byref(pt)) == 0 and pe.value and pt.value
        # a block that ends behind 2^32 - 1: refused with the record's index, nothing left behind; the sorted array still compresses
        n_chr, recs, _ = cvi.crafted_cases()["edge_bad"]
        g.bam_sort_reset()
        g.bam_sort_add(b"".join(recs), 0)
        n, nb = g.bam_sort_finish()
        rc, msg = err_of(lambda: g.bam_coverage_finish())
        assert rc == RANGE and "record 2 " in msg
        rc, msg = err_of(lambda: g.bam_coverage_finish(exclude=4))
        assert rc == RANGE and "record 1 " in msg
        assert g.lib.dg_bam_coverage_download(g.ctx, buf.ctypes.data, 4, None, 0) == ARG
        assert g.bam_sort_compress(0, nb, raw=True) == b"".join(recs)
        assert len(g.bam_sort_compress(0, nb)) > 28
        _still_covers(e, g)
    finally:
        g.close()
    # text without names: DG_ERR_ARG; with the entries-only flag it works (a context made through the C calls alone: DartGPU sets the names itself)
    lib = e.gpu.lib
    st = C.c_int(0)
    f = e.ix.files(0)
    raw_ctx = lib.dg_init_files(C.byref(f), C.byref(host.default_params(paired=0)), 0, 0, C.byref(st))
    assert raw_ctx
    try:
        data = np.frombuffer(bii.record(1, 40, 0, b"r", [(6, bii.M)], l_seq=6) + b"\0", np.uint8)
        n = C.c_size_t(0); nb = C.c_size_t(0); ne = C.c_size_t(0)
        assert lib.dg_bam_sort_add(raw_ctx, data.ctypes.data, len(data) - 1, 0, C.byref(n)) == 0 and n.value == 1
        assert lib.dg_bam_sort_finish(raw_ctx, C.byref(n), C.byref(nb), None) == 0
        assert lib.dg_bam_coverage_finish(raw_ctx, 0, 0x704, 0, C.byref(ne), C.byref(nb), None, None) == ARG and b"names" in lib.dg_last_error(raw_ctx)
        assert lib.dg_bam_coverage_finish(raw_ctx, host.COV_ENTRIES_ONLY, 0x704, 0, C.byref(ne), C.byref(nb), None, None) == 0 and (ne.value, nb.value) == (1, 0)
        ent = np.zeros(1, host.COV_ENTRY)
        assert lib.dg_bam_coverage_download(raw_ctx, ent.ctypes.data, 1, None, 0) == 0 and ent.tolist() == [(1, 40, 46, 1)]
    finally:
        lib.dg_destroy(raw_ctx)
