"""GPU suite (-m gpu): UMI-aware duplicate marking of the coordinate-sorted BAM on the device (dg_bam_markdup_umi_*; dart_amd/csrc/dg_umidup.h).  The expectation
is always the sequential Python twin of tests/umidup_inputs.py over the sorted raw array; records go in through dg_bam_sort_add, so nothing but one test maps.
No umi_tools is run: the definition in include/dartgpu.h is what is pinned."""
import random, re
import numpy as np
import pytest
import common
import bamsort_inputs as bsi
import markdup_inputs as mdi
import umidup_inputs as udi
from dart_amd import host

pytestmark = pytest.mark.gpu
ARG, RANGE = -3, -6
CASES = udi.crafted_cases()


@pytest.fixture(scope="module")
def env(workdir):
    class Env:
        pass
    e = Env()
    e.case = common.build_case("pe101_spliced", workdir)
    e.ix = host.Index(e.case["prefix"])
    e.gpu = host.DartGPU(e.ix)
    e.n_chr = len(e.ix.names)
    assert e.n_chr == 2
    yield e
    e.gpu.close()


def store(g, recs, seed=0):
    """the records, shuffled, as the store's only segment -> the sorted raw array"""
    shuffled = list(recs); random.Random(seed).shuffle(shuffled)
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(shuffled), 0)
    n, nb = g.bam_sort_finish()
    return g.bam_sort_compress(0, nb, raw=True), nb


def mark_and_check(e, g, raw, nb, max_edit, sep=b"_"):
    """count-only first, then written, then again: the array and the stats against the twin -> (marked bytes, stats)"""
    want, stats, _ = udi.twin(raw, e.n_chr, max_edit, sep)
    before = g.bam_sort_compress(0, nb, raw=True)                                 # (raw, or what an earlier call made of it: the input's 0x400 plays no part)
    assert g.bam_markdup_umi_finish(max_edit, sep, count_only=True) == stats
    assert g.bam_sort_compress(0, nb, raw=True) == before                         # counting writes nothing
    assert g.bam_markdup_umi_finish(max_edit, sep) == stats and g.bam_markdup_umi_stats == stats
    assert g.bam_sort_compress(0, nb, raw=True) == want
    assert g.bam_markdup_umi_finish(max_edit, sep) == stats and g.bam_sort_compress(0, nb, raw=True) == want       # idempotent
    return want, stats


def err_of(call):
    with pytest.raises(RuntimeError) as x:
        call()
    m = re.search(r"failed \((-?\d+)\): (.*)", str(x.value), re.S)
    return int(m.group(1)), m.group(2)


def test_same_position_different_umis_are_not_duplicates(env):
    e, g = env, env.gpu
    raw, nb = store(g, CASES["different_umis"][1])
    assert mdi.twin(raw, e.n_chr)[1][3] == 2 and g.bam_markdup_finish(count_only=True)[3] == 2       # by position alone two of the three pairs are copies
    for max_edit in (0, 1):
        marked, st = mark_and_check(e, g, raw, nb, max_edit)
        assert st[3] == st[6] == 0 and st[8] == 6 and st[9] == 1
        assert not any(flag & mdi.DUP for _, flag in mdi.flags_by_name(marked))


@pytest.mark.parametrize("name", sorted(n for n in CASES if n not in ("empty", "different_umis")))
def test_crafted_records_on_the_device(name, env):
    e, g = env, env.gpu
    n_chr, recs = CASES[name]
    raw, nb = store(g, recs, len(name))
    assert sorted(bsi.split(raw)) == sorted(recs)
    for max_edit in (0, 1):
        _, st = mark_and_check(e, g, raw, nb, max_edit)
        if name == "family_of_64":
            assert (st[10], st[11]) == ((3, 0) if max_edit else (0, 0))
        if name == "family_of_65":
            assert (st[10], st[11]) == (0, 3)
        if name == "one_hop_chain" and max_edit:
            assert st[3] == 13 and st[7] == 14


def test_random_records_and_the_device_times(env):
    e, g = env, env.gpu
    assert g.bam_markdup_umi_granules() == (256, 4096, 64, 64)
    rng = random.Random(31)
    raw, nb = store(g, udi.random_records(rng, 3000, e.n_chr), 31)
    _, s0 = mark_and_check(e, g, raw, nb, 0)
    _, s1 = mark_and_check(e, g, raw, nb, 1)
    print("3000 random records: exact %s, edit1 %s; device ms %s, %d passes" % (s0, s1, g.bam_markdup_umi_device_ms_split, g.bam_markdup_umi_passes))
    assert s0[8] > 2000 and s0[9] > 50 and s1[10] > 20 and s0[3] < s1[3] < g.bam_markdup_finish(count_only=True)[3]
    assert g.bam_markdup_umi_device_ms > 0 and len(g.bam_markdup_umi_device_ms_split) == 8
    # only the bits of the largest U are sorted, 4 per pass, once for the pairs and once for the ends, beside the plain marking's passes
    bits = max(udi.umi_of(nm) for nm in udi.names_of(bsi.split(raw))).bit_length()
    plain_passes = g.bam_markdup_passes
    g.bam_markdup_umi_finish(1, count_only=True)
    assert 16 <= bits <= 18 and g.bam_markdup_umi_passes == plain_passes + 2 * ((bits + 3) // 4)
    # another separator: no name holds a UMI, and the plain marking's bytes come out
    marked, sc = mark_and_check(e, g, raw, nb, 1, b":")
    assert sc[8] == 0 and g.bam_markdup_finish() == sc[:8] and g.bam_sort_compress(0, nb, raw=True) == marked


def test_families_and_groups_across_workgroups(env):
    e, g = env, env.gpu
    rng = random.Random(5)
    recs = []
    umis = [udi.doubled(k) for k in range(60)] + [b"AAAAAC", b"AACCAT", b"GGGGGT"]               # 63 groups; the last three, one pair each, lie one letter from a doubled one
    for k in range(700):                                                                           # one family over three workgroups of pairs, six of ends
        recs += mdi.pair(b"a%d_" % k + umis[k % 60 if k < 697 else k - 637], 0, 1000, 0, 0, 1300, 1, q1=60 + k % 37)
    for k in range(700):                                                                           # 700 groups: crowded, nobody marked
        recs += mdi.pair(b"b%d_" % k + bytes(b"ACGT"[k >> s & 3] for s in (10, 8, 6, 4, 2, 0)), 1, 1000, 0, 1, 1300, 1)
    for k in range(600):                                                                           # fragments on the first family's lo end and elsewhere
        recs.append(mdi.mrec(0, 1000 if k % 3 else 5000, 0, b"f%d_" % k + rng.choice(umis), [(50, mdi.M)], mdi.quals_of(100 + k)))
    raw, nb = store(g, recs, 7)
    _, s0 = mark_and_check(e, g, raw, nb, 0)
    _, s1 = mark_and_check(e, g, raw, nb, 1)
    assert s0[1] == 1400 and s0[3] == 700 - 63 and s0[11] == 3 and s0[9] == 2 and s1[10] >= 9 and s1[3] == 700 - 60 and (s0[7], s1[7]) == (12, 13)


def test_mapped_records_without_umis_are_marked_as_by_the_plain_call(env):
    e, g = env, env.gpu
    reads, headers, quals = bsi.sort_reads(e.case)
    n = 600
    reads = np.ascontiguousarray(np.concatenate([reads[:n], reads[:200]]))
    headers = list(headers[:n]) + ["dup%d" % (k // 2) for k in range(200)]
    quals = list(quals[:n]) + ["H" * reads.shape[1]] * 200
    assert not any("_" in h for h in headers)
    p, _ = common.parse_flags(e.case["runs"][0]["flags"])
    so, rl, flat = host.pack_reads(reads)
    g.bam_sort_reset()
    g.set_params(host.default_params(paired=1, **p))
    g.map_batch(so, rl, flat)
    _, ct = g.format_bam(headers, quals, len(reads), raw=True)
    assert g.accumulate_bam(0) == ct["records"]
    n_rec, nb = g.bam_sort_finish()
    raw = g.bam_sort_compress(0, nb, raw=True)
    plain = g.bam_markdup_finish()
    want = g.bam_sort_compress(0, nb, raw=True)
    assert want == mdi.twin(raw, e.n_chr)[0] and plain[3] >= 10          # (of the 100 copied pairs; how many map with both mates is the mapper's business)
    for max_edit in (0, 1):
        g.bam_sort_finish()
        assert g.bam_sort_compress(0, nb, raw=True) == raw
        st = g.bam_markdup_umi_finish(max_edit)
        assert st[:8] == plain and st[8:] == (0, 0, 0, 0) and g.bam_sort_compress(0, nb, raw=True) == want


def test_two_splits_over_ordinals_and_contexts_give_the_same_bytes(env):
    e, g = env, env.gpu
    rng = random.Random(41)
    recs = udi.random_records(rng, 1500, e.n_chr)
    raw, nb = store(g, recs, 41)
    one, st = mark_and_check(e, g, raw, nb, 1)
    a = g.clone()
    try:
        cuts = [0, len(recs) // 3, len(recs) // 2, len(recs)]
        shuffled = list(recs); random.Random(41).shuffle(shuffled)
        # the same records in the same order under three ordinals, on two contexts
        g.bam_sort_reset(); a.bam_sort_reset()
        g.bam_sort_add(b"".join(shuffled[cuts[0]:cuts[1]]), 0); a.bam_sort_add(b"".join(shuffled[cuts[1]:cuts[2]]), 1); g.bam_sort_add(b"".join(shuffled[cuts[2]:cuts[3]]), 2)
        g.bam_sort_merge(a)
        n, nb2 = g.bam_sort_finish()
        assert nb2 == nb and g.bam_sort_compress(0, nb, raw=True) == raw
        assert g.bam_markdup_umi_finish(1) == st and g.bam_sort_compress(0, nb, raw=True) == one
        # and all of them on the clone
        a.bam_sort_reset()
        for k in range(3):
            a.bam_sort_add(b"".join(shuffled[cuts[k]:cuts[k + 1]]), k)
        a.bam_sort_finish()
        assert a.bam_markdup_umi_finish(1) == st and a.bam_sort_compress(0, nb, raw=True) == one
    finally:
        a.close()


def test_argument_errors_leave_the_array_as_it_was(env):
    e = env
    g = e.gpu.clone()
    try:
        rc, msg = err_of(lambda: g.bam_markdup_umi_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg and msg.startswith("dg_bam_markdup_umi_finish")
        raw, nb = store(g, CASES["join_3_1"][1])
        R = host.DgUmiRules
        call = lambda rules, flags=0: g.lib.dg_bam_markdup_umi_finish(g.ctx, host.C.byref(rules) if rules is not None else None, flags, None, None)
        assert call(None) == ARG and call(R(0, 2, b"_", b"")) == ARG and call(R(0, 0, b"\0", b"")) == ARG and call(R(1, 0, b"_", b"")) == ARG and call(R(0x80000000, 1, b"_", b"")) == ARG
        assert call(R(0, 1, b"_", b""), 2) == ARG and call(R(0, 1, b"_", b""), 0x80000001) == ARG
        assert g.bam_sort_compress(0, nb, raw=True) == raw
        assert mark_and_check(e, g, raw, nb, 1)[1][3] == 3
        # an empty store gives zeros
        g.bam_sort_reset()
        assert g.bam_sort_finish() == (0, 0) and g.bam_markdup_umi_finish(1) == (0,) * 12
        # a store call behind the finish
        g.bam_sort_add(CASES["join_3_1"][1][0], 1)
        rc, msg = err_of(lambda: g.bam_markdup_umi_finish(1))
        assert rc == ARG and "dg_bam_sort_finish" in msg
        # an unclipped end outside the end key: the plain call's text, nothing written
        n_chr, recs, _, _ = mdi.crafted_cases()["range"]
        raw, nb = store(g, recs)
        rc, msg = err_of(lambda: g.bam_markdup_umi_finish(1))
        assert rc == RANGE and "record 0 " in msg and g.bam_sort_compress(0, nb, raw=True) == raw
        raw, nb = store(g, CASES["one_hop_chain"][1])
        assert mark_and_check(e, g, raw, nb, 1)[1][3] == 13
    finally:
        g.close()
