"""GPU suite (-m gpu): the splice-junction table on the device (dg_sj_*, dart_amd/csrc/dg_sjtab.h) against the reference's golden junctions.tab, the Python
twin (dart_amd/sam.py::junction_twin) and a dict over the tuples downloaded the old way."""
import ctypes as C
import numpy as np
import pytest
import common
import sj_device_inputs as sji
from dart_amd import host

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_CAPACITY = -3, -4


@pytest.fixture(scope="module")
def small(workdir):
    """the smallest golden index: a root context and two clones"""
    c = common.build_case("se100", workdir)
    ix = host.Index(c["prefix"])
    gpu = host.DartGPU(ix)
    yield c, ix, gpu, gpu.clone(), gpu.clone()
    gpu.close()


def _same(got, want_rows, ix):
    ent, text = got
    t_ent, t_text, _ = sji.twin(want_rows, ix)
    assert text == t_text, common.first_diff(text.decode("latin1"), t_text.decode("latin1"))
    assert len(ent) == len(t_ent)
    for f in host.SJ_ENTRY.names:
        assert np.array_equal(ent[f], t_ent[f]), f


def _fresh(*gpus):
    for g in gpus:
        g.sj_reset()


def test_empty_table_and_error_cases(small, workdir):
    c, ix, gpu, _, _ = small
    lib = gpu.lib
    fresh = host.DartGPU(ix)
    try:
        ent, text = fresh.sj_finish()
        assert len(ent) == 0 and text == b"" and fresh.sj_lines == 0
        assert lib.dg_batch_accumulate_sj(fresh.ctx, None) == ERR_ARG and b"no finished batch" in lib.dg_last_error(fresh.ctx)      # before any batch
        # an se100 batch that has no tuples (its reads without a junction; single reads map independently): nothing is added; a second call on the same
        # batch is refused
        fresh.set_params(host.default_params(paired=0))
        first = fresh.map_batch(*host.pack_reads(c["reads"][:2000]))
        plain = c["reads"][:2000][first.reads["n_sj"] == 0]
        res = fresh.map_batch(*host.pack_reads(plain))
        assert 0 < len(plain) < 2000 and len(res.sj) == 0 and fresh.accumulate_sj() == 0
        assert lib.dg_batch_accumulate_sj(fresh.ctx, None) == ERR_ARG and b"once" in lib.dg_last_error(fresh.ctx)
        assert len(fresh.sj_finish()[0]) == 0
    finally:
        fresh.close()
    # finish without names: DG_ERR_ARG; with the entries-only flag it works (a context made through the C calls alone: DartGPU sets the names itself)
    st = C.c_int(0)
    f = ix.files(0)
    raw = lib.dg_init_files(C.byref(f), C.byref(host.default_params(paired=0)), 0, 0, C.byref(st))
    assert raw
    try:
        e = sji.entries_of([(5, 9, 2)])
        assert lib.dg_sj_add(raw, e.ctypes.data, 1) == 0
        ne = C.c_size_t(0); nl = C.c_size_t(0); nb = C.c_size_t(7)
        assert lib.dg_sj_finish(raw, 0, C.byref(ne), C.byref(nl), C.byref(nb), None) == ERR_ARG and b"names" in lib.dg_last_error(raw)
        assert lib.dg_sj_finish(raw, host.SJ_ENTRIES_ONLY, C.byref(ne), C.byref(nl), C.byref(nb), None) == 0
        assert (ne.value, nl.value, nb.value) == (1, 1, 0)
    finally:
        lib.dg_destroy(raw)
    # a short buffer: DG_ERR_CAPACITY, nothing written
    _fresh(gpu)
    gpu.sj_add([(5, 9, 2), (7, 11, 1)])
    ent, text = gpu.sj_finish()
    assert len(ent) == 2 and len(text) > 4
    small_ent = np.zeros(1, host.SJ_ENTRY); small_ent["count"] = 77
    t_buf = np.full(len(text), 0x55, np.uint8)
    assert lib.dg_sj_download(gpu.ctx, small_ent.ctypes.data, 1, t_buf.ctypes.data, len(text)) == ERR_CAPACITY
    assert lib.dg_sj_download(gpu.ctx, None, 0, t_buf.ctypes.data, len(text) - 1) == ERR_CAPACITY and b"needed" in lib.dg_last_error(gpu.ctx)
    assert int(small_ent["count"][0]) == 77 and (t_buf == 0x55).all()
    assert lib.dg_sj_download(gpu.ctx, None, 0, t_buf.ctypes.data, len(text)) == 0 and t_buf.tobytes() == text      # either pointer may be NULL; the context is still usable
    # a coordinate the table does not hold, reserving a table that is not empty, merging a context into itself
    bad = sji.entries_of([(-(1 << 63), 1, 1)])
    assert lib.dg_sj_add(gpu.ctx, bad.ctypes.data, 1) == ERR_ARG
    assert lib.dg_sj_reserve(gpu.ctx, 1024) == ERR_ARG and lib.dg_sj_merge(gpu.ctx, gpu.ctx) == ERR_ARG
    _same(gpu.sj_finish(), [(5, 9, 2), (7, 11, 1)], ix)


def test_synthetic_keys_equal_the_twin(small):
    c, ix, gpu, _, _ = small
    granule, min_slots = gpu.sj_granules()
    assert granule >= 64 and min_slots >= 64 and min_slots & (min_slots - 1) == 0
    _fresh(gpu)
    rows = sji.synthetic_keys(ix)
    rows += [(1000, 5, 1), (1000, 6, 2), (1000, 7, 3), (5, 1000, 1), (6, 1000, 2)]          # pairs that share g1 and differ in g2, and the reverse
    rows += [(40, (1 << 32) + 3, 1), (40, (2 << 32) + 3, 2), ((1 << 32) + 40, 3, 4), ((5 << 32) + 40, 3, 8), (40, 3, 16)]      # keys that differ only above bit 32
    rows += [(12, 34, 0)]                                                              # a count of 0 adds nothing
    gpu.sj_add(rows)
    _same(gpu.sj_finish(), rows, ix)
    ent, _ = gpu.sj_finish(entries_only=True)                                          # the table stays intact: finishing again gives the same entries
    assert len(ent) == len(sji.twin(rows, ix)[0])
    # one key 100 000 times in one call: contention on one slot, the in-wave combining
    _fresh(gpu)
    hot = np.zeros(100000, host.SJ_ENTRY); hot["g1"], hot["g2"], hot["count"] = 77, 99, 1
    gpu.sj_add(hot)
    _same(gpu.sj_finish(), [(77, 99, 100000)], ix)
    # call sizes on the insert kernel's seams
    for n in (granule - 1, granule, granule + 1, 1):
        _fresh(gpu)
        rows = [(3 * k % 50, k % 7, 1 + k % 3) for k in range(n)]
        gpu.sj_add(rows)
        _same(gpu.sj_finish(), rows, ix)


def _growth_rows(ix, n=5000, seed=11):
    rng = np.random.default_rng(seed)
    keys = np.unique(np.stack([rng.integers(0, 2 * int(ix.l_pac), n), rng.integers(-1000, 1 << 34, n)], 1), axis=0)
    return keys


def test_growth_counts_every_tuple_once(small):
    c, ix, gpu, _, _ = small
    _fresh(gpu)
    gpu.sj_reserve(1)                                            # the minimum
    keys = _growth_rows(ix)
    both = np.concatenate([keys, keys]); np.random.default_rng(3).shuffle(both)
    at = 0
    for size in (1, 255, 256, 257, 1000, 3, 4096, len(both)):  # calls of uneven size
        part = both[at:at + size]; at += len(part)
        e = np.zeros(len(part), host.SJ_ENTRY); e["g1"], e["g2"], e["count"] = part[:, 0], part[:, 1], 1
        gpu.sj_add(e)
    assert at == len(both)
    ent, _ = gpu.sj_finish(entries_only=True)
    assert (ent["count"] == 2).all()
    assert np.array_equal(np.stack([ent["g1"], ent["g2"]], 1), keys)      # numpy.unique's set, in its (signed, g1 first) order


def test_same_multiset_gives_the_same_bytes(small):
    c, ix, gpu, cl1, cl2 = small
    keys = _growth_rows(ix, 3000, seed=12)
    rng = np.random.default_rng(8)
    rows = np.concatenate([keys, keys[:1500], keys[:700], np.asarray(sji.synthetic_keys(ix))[:, :2].astype(np.int64)])
    def ent_of(a):
        e = np.zeros(len(a), host.SJ_ENTRY); e["g1"], e["g2"], e["count"] = a[:, 0], a[:, 1], 1
        return e
    # 1: one call, in one order
    _fresh(gpu, cl1, cl2)
    gpu.sj_add(ent_of(rows))
    ent1, text1 = gpu.sj_finish()
    # 2: another order, split over the root and two clones, merged
    _fresh(gpu)
    shuffled = rows.copy(); rng.shuffle(shuffled)
    thirds = np.array_split(shuffled, 3)
    for g, part in zip((gpu, cl1, cl2), thirds):
        g.sj_add(ent_of(part))
    gpu.sj_merge(cl1); gpu.sj_merge(cl2)
    ent2, text2 = gpu.sj_finish()
    assert len(cl1.sj_finish(entries_only=True)[0]) == 0 and len(cl2.sj_finish(entries_only=True)[0]) == 0      # after the merge the source is empty
    # 3: growth at other moments: the smallest table, many small calls
    _fresh(gpu)
    gpu.sj_reserve(1)
    for part in np.array_split(shuffled[::-1], 9):
        gpu.sj_add(ent_of(part))
    ent3, text3 = gpu.sj_finish()
    assert text1 == text2 == text3 and len(text1) > 0
    assert ent1.tobytes() == ent2.tobytes() == ent3.tobytes()
    _same((ent1, text1), [tuple(r) for r in rows.tolist()], ix)
    gpu.sj_reset()
    assert len(gpu.sj_finish()[0]) == 0 and gpu.sj_finish()[1] == b""


@pytest.mark.parametrize("name", ["pe101_spliced", "pe151_spliced"])
def test_mapping_path_reproduces_the_golden_junction_table(name, workdir):
    c = common.build_case(name, workdir)
    ix = host.Index(c["prefix"])
    gpu = host.DartGPU(ix)
    try:
        ctxs = [gpu, gpu.clone(), gpu.clone()]
        reads = c["reads"]
        step = 3000                                             # batches of a few thousand reads (even: pairs stay together), dealt over a root and two clones
        for run in c["runs"]:
            p, _ = common.parse_flags(run["flags"])
            _fresh(*ctxs)
            want = {}; types = []; total = 0
            for b, lo in enumerate(range(0, len(reads), step)):
                g = ctxs[b % 3]
                g.set_params(host.default_params(paired=1, **p))
                res = g.map_batch(*host.pack_reads(reads[lo:lo + step]))
                total += g.accumulate_sj()
                for g1, g2 in zip(res.sj["g1"].tolist(), res.sj["g2"].tolist()):      # the tuples downloaded the old way
                    want[(g1, g2)] = want.get((g1, g2), 0) + 1
                types.append(res.sj["type"].copy())
            gpu.sj_merge(ctxs[1]); gpu.sj_merge(ctxs[2])
            ent, text = gpu.sj_finish()
            assert text.decode("latin1") == common.golden_junctions(run["base"]), run["base"]
            assert total == sum(want.values()) and len(ent) == len(want)
            assert [(int(e["g1"]), int(e["g2"]), int(e["count"])) for e in ent] == [(k[0], k[1], want[k]) for k in sorted(want)]
            types = np.concatenate(types)
            assert np.isin(types, (0, 2)).any() and np.isin(types, (1, 3)).any() and (ent["count"] > 1).any()      # both strands, repeated keys: the case proves something
        # once after dg_map_batch_compact: the tuples of a compact run are counted the same way
        p, _ = common.parse_flags(c["runs"][0]["flags"])
        _fresh(gpu)
        gpu.set_params(host.default_params(paired=1, **p))
        words, nlist = host.pack_reads_2bit(reads[:step])
        res = gpu.map_batch_compact(words, nlist, reads.shape[1])
        assert gpu.accumulate_sj() == len(res.sj) > 0
        ent, text = gpu.sj_finish(entries_only=True)
        assert text == b"" and ent.tobytes() == sji.twin(list(zip(res.sj["g1"].tolist(), res.sj["g2"].tolist())), ix)[0].tobytes()
    finally:
        gpu.close()
