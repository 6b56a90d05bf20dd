"""GPU suite (-m gpu): duplicate marking of the coordinate-sorted BAM on the device (dg_bam_markdup_*; dart_amd/csrc/dg_markdup.h).  The expectation is always
the sequential Python twin of tests/markdup_inputs.py over the sorted raw array.  No samtools or Picard is run: the definition in the header is what is pinned."""
import os, random, re, struct
import numpy as np
import pytest
import common, bam_decode
import bamsort_inputs as bsi
import bamidx_inputs as bii
import coverage_inputs as cvi
import markdup_inputs as mdi
from dart_amd import host

pytestmark = pytest.mark.gpu
ARG, RANGE = -3, -6
FIRST = 1234
N_COPIES = 200


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


def mark_and_check(e, g, hash_bits=mdi.HASH_BITS):
    """finish, mark, and compare the array and the stats with the twin -> (unmarked bytes, marked bytes, stats)"""
    n, nb = g.bam_sort_finish()
    raw = g.bam_sort_compress(0, nb, raw=True)
    want, stats, _ = mdi.twin(raw, e.n_chr, hash_bits)
    assert g.bam_markdup_finish(count_only=True) == stats
    assert g.bam_sort_compress(0, nb, raw=True) == raw                            # counting writes nothing
    assert g.bam_markdup_finish() == stats and g.bam_markdup_stats == stats
    got = g.bam_sort_compress(0, nb, raw=True)
    assert got == want
    assert stats[6] == 2 * stats[3] + stats[4] and stats[0] == 2 * stats[1] + stats[2]
    assert g.bam_markdup_finish() == stats and g.bam_sort_compress(0, nb, raw=True) == want       # idempotent
    return raw, got, stats


@pytest.fixture(scope="module")
def env(workdir):
    e = Env()
    e.case = common.build_case("pe101_spliced", workdir)
    e.ix = host.Index(e.case["prefix"])
    e.gpu = host.DartGPU(e.ix)
    e.names = [n if isinstance(n, bytes) else n.encode() for n in e.ix.names]
    e.n_chr = len(e.names)
    assert e.n_chr == 2
    reads, headers, quals = bsi.sort_reads(e.case)
    L = reads.shape[1]
    # the first pairs again under new names, every quality lowered by one
    e.reads = np.ascontiguousarray(np.concatenate([reads, reads[:2 * N_COPIES]]))
    e.headers = list(headers) + ["dup%d" % (k // 2) for k in range(2 * N_COPIES)]
    e.quals = list(quals) + ["H" * L] * (2 * N_COPIES)
    e.p, _ = common.parse_flags(e.case["runs"][0]["flags"])
    e.unsorted = {}
    for paired in (1, 0):
        e.gpu.bam_sort_reset()
        e.unsorted[paired] = batch(e, e.gpu, 0, len(e.reads), 0, paired)
    e.others = {}

    def with_bits(bits):
        """a context created under DG_MARKDUP_HASH_BITS = bits"""
        if bits == mdi.HASH_BITS:
            return e.gpu
        if bits not in e.others:
            os.environ["DG_MARKDUP_HASH_BITS"] = str(bits)
            try:
                e.others[bits] = host.DartGPU(e.ix)
            finally:
                del os.environ["DG_MARKDUP_HASH_BITS"]
        return e.others[bits]
    e.with_bits = with_bits
    yield e
    for g in e.others.values():
        g.close()
    e.gpu.close()


def err_of(call):
    with pytest.raises(RuntimeError) as x:
        call()
    m = re.search(r"failed \((-?\d+)\): (.*)", str(x.value), re.S)
    return int(m.group(1)), m.group(2)


def name_of(rec):
    return rec[36:36 + rec[12] - 1]


def test_mapped_records_paired_and_single(env):
    e, g = env, env.gpu
    for paired in (1, 0):
        g.bam_sort_reset()
        g.bam_sort_add(e.unsorted[paired], 0)
        raw, marked, st = mark_and_check(e, g)
        print("paired=%d: %d reads, %d records, stats %s, device ms %s, %d passes" % (paired, len(e.reads), len(bii.offsets(raw)), st, g.bam_markdup_device_ms_split, g.bam_markdup_passes))
        assert g.bam_markdup_device_ms > 0 and len(g.bam_markdup_device_ms_split) == 6 and g.bam_markdup_passes >= 12
        offs = bii.offsets(raw)
        by_name = {}
        for i, at in enumerate(offs):
            flag = struct.unpack_from("<H", marked, at + 18)[0]
            by_name.setdefault(name_of(raw[at:]), []).append((mdi.examine(raw, at, e.n_chr, i) is not None, bool(flag & mdi.DUP)))
        if paired:
            checked = 0
            for k in range(N_COPIES):
                orig, copy = by_name[e.headers[2 * k].encode()], by_name[b"dup%d" % k]
                if sum(x for x, _ in orig) == 2 and len(orig) == 2:
                    assert [d for _, d in copy] == [True, True] and [d for _, d in orig] == [False, False], e.headers[2 * k]
                    checked += 1
            assert checked >= 1 and st[3] >= checked and st[1] >= 2 * checked          # (how many pairs map with both mates is the mapper's business)
        else:
            assert st[1] == 0 and st[3] == 0 and st[4] >= 1 and st[2] == st[0]


@pytest.mark.parametrize("name", sorted(n for n, c in mdi.crafted_cases().items() if c[3] and n not in ("range", "empty")))
def test_crafted_records_on_the_device(name, env):
    e = env
    n_chr, recs, hash_bits, _ = mdi.crafted_cases()[name]
    assert n_chr == e.n_chr
    g = e.with_bits(hash_bits)
    rng = random.Random(len(name))
    shuffled = list(recs); rng.shuffle(shuffled)
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(shuffled), 0)
    raw, marked, st = mark_and_check(e, g, hash_bits)
    assert sorted(bsi.split(raw)) == sorted(recs)
    if name == "crowd":
        assert st[5] == 65


def test_seams_families_and_piles_across_workgroups_and_sorter_tiles(env):
    e, g = env, env.gpu
    g0, g1, g2 = g.bam_markdup_granules()
    assert (g0, g1, g2) == (256, 4096, 64)
    n = 5000
    recs = []
    for k in range(n):                                             # one signature, distinct scores: the last one survives; mates 5000 records apart
        recs += mdi.pair(b"d%d" % k, 0, 1000, 0, 0, 2000, 1, q1=100 + k, q2=60)
    for k in range(n):                                             # one signature, equal scores: the first one survives
        recs += mdi.pair(b"e%d" % k, 1, 1000, 0, 1, 2000, 1)
    recs += mdi.pair(b"under_the_pile", 1, 5000, 0, 1, 5100, 1)
    recs += [mdi.mrec(1, 5000, 0, b"pile%d" % k, [(50, mdi.M)], mdi.quals_of(100 + k)) for k in range(n)]      # every one of them on the pair's end
    recs += [mdi.mrec(1, 7000, 0, b"heap%d" % k, [(50, mdi.M)], mdi.quals_of(100 + (k * 7919) % n)) for k in range(n)]  # fragments alone: one survives
    assert 2 * n > 2 * g1 and n > 3000
    g.bam_sort_reset()
    cut = 2 * n + 2 * (n // 2)                                     # in the middle of the second family: its later half comes first in the array
    g.bam_sort_add(b"".join(recs[:cut]), 1); g.bam_sort_add(b"".join(recs[cut:]), 0)
    raw, marked, st = mark_and_check(e, g)
    assert st == (6 * n + 2, 2 * n + 1, 2 * n, 2 * n - 2, 2 * n - 1, 0, 6 * n - 5, n)
    clear = {nm for nm, flag in mdi.flags_by_name(marked) if not flag & mdi.DUP}
    assert clear == {b"d%d" % (n - 1), b"e%d" % (n // 2), b"under_the_pile", b"heap%d" % next(k for k in range(n) if (k * 7919) % n == n - 1)}
    # around a workgroup's and a tile's edge: a family of m pairs leaves m - 1 duplicates
    for m in (g0 - 1, g0, g0 + 1, g1 // 2, g1 // 2 + 1):
        g.bam_sort_reset()
        g.bam_sort_add(b"".join(b"".join(mdi.pair(b"s%d" % k, 0, 10, 0, 0, 10, 1)) for k in range(m)), 0)
        assert mark_and_check(e, g)[2] == (2 * m, m, 0, m - 1, 0, 0, 2 * m - 2, m)


def test_hash_bits_from_the_environment(env):
    e = env
    g = e.with_bits(6)
    rng = random.Random(6)
    # 2000 records: random ones (some thirty candidates per run of the 64), and seventy pairs whose names share one hash: a crowd
    recs = mdi.random_records(rng, 1860, e.n_chr)[:1860]
    for k, nm in enumerate(mdi.collide(6, 17, b"crowd", 70)):
        recs += mdi.pair(nm, 1, 4000 + k % 5, 0, 1, 4300, 1, q1=60 + k)
    assert len(recs) == 2000
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(recs), 0)
    raw, marked, st = mark_and_check(e, g, 6)
    assert st[5] > 0 and st[1] > 0
    assert mdi.twin(raw, e.n_chr)[0] != marked                      # (with all 48 bits nothing is crowded: another verdict)
    # the same records on the ordinary context
    e.gpu.bam_sort_reset()
    e.gpu.bam_sort_add(b"".join(recs), 0)
    assert mark_and_check(e, e.gpu)[2][5] == 0


def test_batches_clones_and_fed_back_records_do_not_change_a_byte(env):
    e, g = env, env.gpu
    n = len(e.reads)
    g.bam_sort_reset()
    batch(e, g, 0, n, 0)
    raw, one, st = mark_and_check(e, g)
    assert raw == b"".join(bsi.expected_sorted([(0, e.unsorted[1])], e.n_chr))
    cuts = [0, n // 6 * 2, n // 2 // 2 * 2 + 200, n]
    a, b = g.clone(), g.clone()
    try:
        for c in (g, a, b):
            c.bam_sort_reset()
        pieces = [batch(e, c, cuts[k], cuts[k + 1], k) for k, c in ((2, b), (0, g), (1, a))]
        g.bam_sort_merge(b); g.bam_sort_merge(a)
        assert mark_and_check(e, g)[1:] == (one, st)
        # the records fed back from the host under the same ordinals, on a clone
        a.bam_sort_reset()
        for k, piece in zip((2, 0, 1), pieces):
            a.bam_sort_add(piece, k)
        assert mark_and_check(e, a)[1:] == (one, st)
        # the store is untouched: another finish gives the unmarked array again
        assert sorted_raw(a) == raw
    finally:
        a.close(); b.close()


def test_compress_index_and_coverage_see_the_marks(env):
    e, g = env, env.gpu
    g.bam_sort_reset()
    g.bam_sort_add(e.unsorted[1], 0)
    n, nb = g.bam_sort_finish()
    raw = g.bam_sort_compress(0, nb, raw=True)
    unmarked_cov = g.bam_coverage_finish()
    unmarked_counted = g.bam_coverage_stats[0]
    z0 = g.bam_sort_compress(0, nb)                               # every block compressed -- before the marking
    assert len(g.bam_index_finish(FIRST)) > 100
    st = g.bam_markdup_finish()
    rc, msg = err_of(lambda: g.bam_index_finish(FIRST))
    assert rc == ARG and "has not been compressed" in msg
    z = g.bam_sort_compress(0, nb)
    marked = g.bam_sort_compress(0, nb, raw=True)
    assert marked == mdi.twin(raw, e.n_chr)[0] and z != z0
    z = g.bam_sort_compress(0, nb)
    bai = g.bam_index_finish(FIRST)
    assert bai == bii.build_bai(marked, [s for _, s in bam_decode.bgzf_blocks(z)], FIRST, e.n_chr)
    ent, text = g.bam_coverage_finish()
    t_ent, t_stats = cvi.twin(marked, e.n_chr)
    assert ent.tolist() == t_ent and text == cvi.text_of(t_ent, e.names) and g.bam_coverage_stats == t_stats
    assert t_stats[0] == unmarked_counted - st[6] and st[6] > 0 and text != unmarked_cov[1]
    # with duplicates counted, the unmarked track again
    assert g.bam_coverage_finish(exclude=0x304)[1] == unmarked_cov[1]


def _still_marks(e, g):
    """after a refused call: the context maps a batch, keeps it, sorts it and marks it"""
    g.bam_sort_reset()
    batch(e, g, 0, 400, 0)
    assert mark_and_check(e, g)[2][0] > 100


def test_empty_store_and_refusals(env):
    e = env
    g = e.gpu.clone()
    try:
        # no finish at all on a fresh context
        rc, msg = err_of(lambda: g.bam_markdup_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg
        _still_marks(e, g)
        # an empty store
        g.bam_sort_reset()
        assert g.bam_sort_finish() == (0, 0)
        assert g.bam_markdup_finish() == (0,) * 8
        # records that all play no part
        g.bam_sort_add(bii.record(-1, -1, 4, b"u", l_seq=5) + bii.record(0, 3, 0x100 | 0x400, b"sec", [(5, bii.M)], l_seq=5), 0)
        raw, marked, st = mark_and_check(e, g)
        assert st == (0,) * 8 and marked == raw
        # a store call behind the finish
        g.bam_sort_add(bii.record(0, 3, 0, b"late", [(5, bii.M)], l_seq=5), 1)
        rc, msg = err_of(lambda: g.bam_markdup_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg
        _still_marks(e, g)
        # a flag bit nobody defined: refused, the array as it was
        n, nb = g.bam_sort_finish()
        raw = g.bam_sort_compress(0, nb, raw=True)
        assert g.lib.dg_bam_markdup_finish(g.ctx, 2, None, None) == ARG and g.lib.dg_bam_markdup_finish(g.ctx, 0x80000001, None, None) == ARG
        assert g.bam_sort_compress(0, nb, raw=True) == raw
        assert g.lib.dg_bam_markdup_finish(g.ctx, 0, None, None) == 0
        # an unclipped end outside the end key: refused with the record's index, nothing written; the sorted array still compresses
        n_chr, recs, _, _ = mdi.crafted_cases()["range"]
        dups = [mdi.mrec(0, 10, 0, b"fine_too", [(5, mdi.M)], mdi.quals_of(50)), mdi.mrec(0, 10, 0x400, b"fine_marked", [(5, mdi.M)], mdi.quals_of(300))]
        g.bam_sort_reset()
        g.bam_sort_add(b"".join(recs[1:] + dups), 0)
        n, nb = g.bam_sort_finish()
        raw = g.bam_sort_compress(0, nb, raw=True)
        assert [name_of(r) for r in bsi.split(raw)] == [b"fine", b"fine_too", b"fine_marked", b"too_far_right"]
        rc, msg = err_of(lambda: g.bam_markdup_finish())
        assert rc == RANGE and "record 3 " in msg
        rc, msg = err_of(lambda: g.bam_markdup_finish(count_only=True))
        assert rc == RANGE and "record 3 " in msg
        assert g.bam_sort_compress(0, nb, raw=True) == raw
        assert len(g.bam_sort_compress(0, nb)) > 28
        g.bam_sort_reset()
        g.bam_sort_add(b"".join(recs), 0)
        g.bam_sort_finish()
        rc, msg = err_of(lambda: g.bam_markdup_finish())
        assert rc == RANGE and "record 0 " in msg
        _still_marks(e, g)
    finally:
        g.close()
