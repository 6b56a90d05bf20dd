"""GPU suite (-m gpu): the QC tables of the coordinate-sorted BAM, built on the device (dg_bam_qc_*; dart_amd/csrc/dg_qc.h).  The expectation is always the
sequential Python twin of tests/qc_inputs.py over the sorted raw array and the index's own 2-bit text.  No samtools is run: the definition in the header is
what is pinned."""
import ctypes as C
import os, random, re, struct
import numpy as np
import pytest
import common
import bamsort_inputs as bsi
import bamidx_inputs as bii
import pileup_inputs as pui
import qc_inputs as qci
from qc_inputs import SN
from dart_amd import host

pytestmark = pytest.mark.gpu
ARG, CAPACITY = -3, -4
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


def check(e, g, raw, flt=qci.FILTERS[0]):
    """the device's tables of the finished store against the twin over `raw` -> the views"""
    got = g.bam_qc_finish(*flt)
    want = qci.twin(raw, e.ref, *flt)
    assert got["words"].dtype == np.uint64 and len(got["words"]) == len(want)
    assert np.array_equal(got["words"], want), [(int(k), int(got["words"][k]), int(want[k])) for k in np.flatnonzero(got["words"] != want)[:10]]
    assert g.bam_qc_text(got) == qci.text_of(want, e.names, e.ix.chr_len)
    for name, v in qci.views(want, e.ref.n_chr).items():
        assert got[name].shape == v.shape and np.array_equal(got[name], v)
    return got


def with_groups(e, groups):
    """a context of its own that read DG_QC_MAX_GROUPS = groups at its start (None: the default grid)"""
    old = os.environ.pop("DG_QC_MAX_GROUPS", None)
    if groups is not None:
        os.environ["DG_QC_MAX_GROUPS"] = str(groups)
    try:
        return host.DartGPU(e.ix)
    finally:
        os.environ.pop("DG_QC_MAX_GROUPS", None)
        if old is not None:
            os.environ["DG_QC_MAX_GROUPS"] = old


@pytest.fixture(scope="module")
def env(workdir):
    e = Env()
    e.case = common.build_case("pe101_spliced", workdir)
    e.ix = host.Index(e.case["prefix"])
    e.gpu = host.DartGPU(e.ix)
    e.names = [n if isinstance(n, bytes) else n.encode() for n in e.ix.names]
    e.ref = pui.ref_of_index(e.ix)
    assert e.ref.n_chr == len(e.names) == 2
    e.crafted = qci.crafted_cases(e.ref, e.names)
    e.reads, e.headers, e.quals = bsi.sort_reads(e.case)
    e.p, _ = common.parse_flags(["-mis", "5"])
    e.unsorted = {}
    for paired in (1, 0):
        e.gpu.bam_sort_reset()
        e.unsorted[paired] = batch(e, e.gpu, 0, len(e.reads), 0, paired)
    # the hand-made extras of the allele counts' test: a secondary, a failed and a duplicate line, each with a mismatch over covered ground, and reads of low quality
    rec = lambda tid, pos, flag, name, mapq=30: pui.rec_on(e.ref, tid, pos, flag, name, [(40, M), (300, bii.N), (40, bii.EQ)], {7: "!", 50: "N"}, mapq)
    e.extra = b"".join([rec(0, 5000, 0x100, b"secondary"), rec(0, 5000, 0x200 | 16, b"qcfail"), rec(0, 5000, 0x400, b"duplicate"), rec(0, 5000, 0, b"mapq0", 0),
                        rec(0, 5000, 0x91, b"mapq3", 3), rec(0, 5000, 0x91, b"mapq30")])
    # host-made records for the grids: copies of a few shapes, so that every table is busy and the twin stays cheap (it is linear in the distinct records)
    shapes = [qci.rec_on(e.ref, k & 1, 100 + 37 * k, (0x43, 0x93, 0x53, 0x83, 0, 16, 0x400, 0x4)[k % 8], b"g%d" % k, [(2, bii.S), (20 + k, M), (k % 3, bii.I), (1 + k % 2, bii.D), (9, M)],
                         {5: "!", 8: "N"}, mapq=(0, 4, 5, 255, 30)[k % 5], qual=qci.quals_of(31 + k + k % 3, k), next_tid=k & 1, next_pos=150 + 30 * k, tlen=(250 + k) * (1 if k & 2 else -1)) for k in range(16)]
    e.shapes = shapes
    yield e
    e.gpu.close()


def many(e, n):
    """n host-made records: the sixteen shapes over and over"""
    return [e.shapes[k % 16] for k in range(n)]


def twin_of_many(e, n, flt=qci.FILTERS[0]):
    """the twin over n records of `many`: the words are sums over records, so sixteen twins of one record each, weighted"""
    total = np.zeros(qci.layout(e.ref.n_chr)["words"], np.uint64)
    for k in range(16):
        total += qci.twin(e.shapes[k], e.ref, *flt) * np.uint64(len(range(k, n, 16)))
    return total


def err_of(call):
    with pytest.raises(RuntimeError) as x:
        call()
    m = re.search(r"failed \((-?\d+)\): (.*)", str(x.value), re.S)
    return int(m.group(1)), m.group(2)


@pytest.mark.parametrize("name", ["lengths", "big", "ops", "ends", "pairs", "flags", "quals"])
def test_crafted_records_on_the_device(name, env):
    e, g = env, env.gpu
    recs = e.crafted[name]
    rng = random.Random(len(name))
    shuffled = list(recs); rng.shuffle(shuffled)
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(shuffled), 0)
    raw = sorted_raw(g)
    assert sorted(bsi.split(raw)) == sorted(recs)
    for flt in qci.FILTERS:
        v = check(e, g, raw, flt)
    assert g.bam_qc_device_ms > 0 and len(g.bam_qc_device_ms_split) == 2
    if name == "lengths":
        assert v["SN"][SN["profiled"]] == 2 * len(qci.LENGTHS) and v["RL"][:, 0].sum() == 2          # l_seq 0 with a CIGAR: in the flag tables, not profiled
    if name == "big":
        assert g.bam_qc_granules() == (256, 4, 64, 32, 16384) and v["SN"][SN["profiled"]] == 3 and v["SN"][SN["profiled_bases"]] == sum(qci.BIG_LENGTHS)
    if name == "ends":
        assert v["SN"][SN["left_out"]] == 4


def test_malformed_records_never_reach_the_store(env):
    """dg_bam_sort_add refuses every record that is not whole (block_size smaller than the fields need, or a record that ends behind the input), so the sorted
    array never holds one and SN.malformed stays 0 on the device; the row is carried by tests/test_qc_lane_code_host.py, which runs the lane code over such arrays."""
    e, g = env, env.gpu
    good = qci.rec_on(e.ref, 0, 200, 0, b"good", [(10, M)], {1: "!"})
    for bad in (qci.liar(e.ref), good[:len(good) - 3], struct.pack("<I", 40) + good[4:44]):
        g.bam_sort_reset()
        rc, msg = err_of(lambda: g.bam_sort_add(good + bad, 0))
        assert rc == ARG
    g.bam_sort_reset()
    g.bam_sort_add(good, 0)
    assert check(e, g, sorted_raw(g))["SN"][SN["malformed"]] == 0


def test_counts_and_grids_give_identical_words(env):
    e = env
    per_group = {}
    for groups in (1, 3, None):
        g = with_groups(e, groups)
        try:
            for n in ((1, 255, 256, 257, 3000) if groups else (65537,)):
                g.bam_sort_reset()
                g.bam_sort_add(b"".join(many(e, n)), 0)
                nrec, nb = g.bam_sort_finish()
                assert nrec == n
                got = g.bam_qc_finish()
                # 3000 records, 16 a trip: 188 trips of the one workgroup and 5 flushes on the way; 63 trips each of three and a flush on the way
                assert np.array_equal(got["words"], twin_of_many(e, n)), (groups, n)
                per_group[groups, n] = got["words"]
            if groups is None:
                # the default grid against the capped ones on the same records
                for cap in (1, 3):
                    h = with_groups(e, cap)
                    try:
                        h.bam_sort_add(b"".join(many(e, 65537)), 0)
                        h.bam_sort_finish()
                        assert np.array_equal(h.bam_qc_finish()["words"], per_group[None, 65537])
                    finally:
                        h.close()
        finally:
            g.close()
    for n in (1, 255, 256, 257, 3000):
        assert np.array_equal(per_group[1, n], per_group[3, n])


def test_mappers_records_for_several_filters_and_against_the_other_stages(env):
    e, g = env, env.gpu
    for paired in (1, 0):
        g.bam_sort_reset()
        g.bam_sort_add(e.unsorted[paired], 0); g.bam_sort_add(e.extra, 1)
        n, nb = g.bam_sort_finish()
        md = g.bam_markdup_finish()
        raw = g.bam_sort_compress(0, nb, raw=True)
        got = {flt: check(e, g, raw, flt) for flt in qci.FILTERS}
        v = got[0x704, 0]
        # the totals of the allele counts under the same filter: aligned bases, mismatches, deleted bases, insertions
        g.bam_pileup_finish(0x704, 0, 1, entries_only=True)
        st = g.bam_pileup_stats
        assert (int(v["SN"][SN["aligned"]]), int(v["SN"][SN["mismatches"]]), int(v["SN"][SN["deleted_bases"]]), int(v["PC"][:, 10].sum())) == (st[2], st[3], st[4], st[5])
        assert int(v["SN"][SN["profiled"]]) == st[0] and int(v["SN"][SN["left_out"]]) == st[8]
        assert int(v["FS"][:, 4].sum()) == md[6]                                  # the records that left the marking with 0x400
        assert int(v["CH"].sum()) == n == int(v["SN"][SN["records"]]) and v["SN"][SN["malformed"]] == 0
        # a condition, not a measurement: no column is pinned at zero only
        assert v["SN"][SN["mismatches"]] > 0 and v["PC"][:, 10].sum() > 0 and v["SN"][SN["deleted_bases"]] > 0 and v["SN"][SN["n_ops"]] > 0
        if paired:
            assert v["FS"][:, 11].sum() > 0 and v["IS"].sum() > 0 and v["SN"][SN["pairs"]] == v["IS"].sum() and v["RL"][1].sum() > 0
        d = got[qci.FILTERS[0]]
        assert got[4, 0]["SN"][SN["profiled"]] > d["SN"][SN["profiled"]] > got[qci.DEFAULT_EXCLUDE, 4]["SN"][SN["profiled"]]
        for flt in qci.FILTERS[1:]:                                               # the filter touches the profile only
            for sec in ("FS", "CH", "MQ", "IS", "RL"):
                assert np.array_equal(got[flt][sec], d[sec])


def test_order_batches_ordinals_and_contexts_do_not_change_a_word(env):
    e, g = env, env.gpu
    recs = bsi.split(e.unsorted[1]) + bsi.split(e.extra) + e.crafted["ops"] + e.crafted["pairs"]
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(recs), 0)
    one = check(e, g, sorted_raw(g), qci.FILTERS[1])["words"]
    rng = random.Random(9)
    shuffled = list(recs); rng.shuffle(shuffled)
    cuts = [0, len(recs) // 5, len(recs) // 2, len(recs)]
    g.bam_sort_reset()
    for k, ordinal in enumerate((2, 0, 1)):
        g.bam_sort_add(b"".join(shuffled[cuts[k]:cuts[k + 1]]), ordinal)
    sorted_raw(g)
    assert np.array_equal(g.bam_qc_finish(*qci.FILTERS[1])["words"], one)
    assert np.array_equal(g.bam_qc_finish(*qci.FILTERS[1])["words"], one)                        # a repeated call
    assert not np.array_equal(g.bam_qc_finish(*qci.FILTERS[0])["words"], one)                    # and one with another filter
    clone = g.clone()
    try:
        g.bam_sort_reset(); clone.bam_sort_reset()
        clone.bam_sort_add(b"".join(shuffled[:cuts[2]]), 1); g.bam_sort_add(b"".join(shuffled[cuts[2]:]), 0)
        g.bam_sort_merge(clone)
        sorted_raw(g)
        assert np.array_equal(g.bam_qc_finish(*qci.FILTERS[1])["words"], one)
    finally:
        clone.close()
    # read-only on the array, and the other stages' results stay
    g.bam_sort_reset()
    g.bam_sort_add(e.unsorted[1], 0)
    n, nb = g.bam_sort_finish()
    z = g.bam_sort_compress(0, nb); bai = g.bam_index_finish(1234)
    before = g.bam_sort_compress(0, nb, raw=True)
    g.bam_qc_finish()
    assert g.bam_sort_compress(0, nb, raw=True) == before and g.bam_sort_compress(0, nb) == z and g.bam_index_finish(1234) == bai


def test_refusals(env):
    e = env
    g = e.gpu.clone()
    try:
        rc, msg = err_of(lambda: g.bam_qc_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg
        buf = np.zeros(40000, np.uint64)
        assert g.lib.dg_bam_qc_download(g.ctx, buf.ctypes.data, len(buf)) == ARG
        g.bam_sort_reset()
        assert g.bam_sort_finish() == (0, 0)
        assert not g.bam_qc_finish()["words"].any()                                              # an empty store: all-zero words
        g.bam_sort_add(b"".join(e.crafted["flags"]), 0)
        raw = sorted_raw(g)
        assert g.lib.dg_bam_qc_finish(g.ctx, 1, 0x904, 0, None, None) == ARG and b"flags" in g.lib.dg_last_error(g.ctx)      # a flag bit nobody defined
        assert g.lib.dg_bam_qc_download(g.ctx, buf.ctypes.data, len(buf)) == ARG                 # the refused call left no tables
        want = check(e, g, raw)["words"]
        assert g.lib.dg_bam_qc_download(g.ctx, buf.ctypes.data, len(want) - 1) == CAPACITY and not buf.any()               # one word short: nothing written
        assert g.lib.dg_bam_qc_download(g.ctx, buf.ctypes.data, len(want)) == 0 and np.array_equal(buf[:len(want)], want) and not buf[len(want):].any()
        p = C.c_void_p()
        assert g.lib.dg_bam_qc_device(g.ctx, C.byref(p)) == 0 and p.value
        g.bam_sort_add(e.crafted["quals"][0], 1)                                                 # a store call behind the finish
        rc, msg = err_of(lambda: g.bam_qc_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg
        assert g.lib.dg_bam_qc_download(g.ctx, buf.ctypes.data, len(buf)) == ARG
        check(e, g, sorted_raw(g))
        # the duplicate marking changes flags: it forgets the tables, as it forgets the index and the track
        g.bam_markdup_finish()
        assert g.lib.dg_bam_qc_download(g.ctx, buf.ctypes.data, len(buf)) == ARG
    finally:
        g.close()
