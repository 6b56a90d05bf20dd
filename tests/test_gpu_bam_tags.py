"""GPU suite (-m gpu): MD, NM and ts written onto the records of the coordinate-sorted BAM on the device (dg_bam_tags_*; dart_amd/csrc/dg_tags.h).  The
expectation is always the sequential Python twin of tests/tags_inputs.py over the sorted raw array and the index's own 2-bit text.  No samtools is run: the
definition in the header is what is pinned."""
import os, random, re, struct
import numpy as np
import pytest
import common, bam_decode
import bamsort_inputs as bsi
import bamidx_inputs as bii
import pileup_inputs as pui
import tags_inputs as tgi
from dart_amd import host, synth, index_build

pytestmark = pytest.mark.gpu
ARG, CAPACITY = -3, -4
BLOCK = bii.BLOCK
FIRST = 1234
MAPPER_SEED = 5          # chosen on the CPU oracle's alignments run through the twin: 766 of 800 records rewritten, 474 mismatches, 5 records with a deletion, 49 ts:A:+ and 40 ts:A:-


class Env:
    pass


def index_of(workdir, tag, ref, names):
    """an index over the twin's reference: the text the device compares with is the text the twin reads"""
    g = synth.Genome([n.decode() for n in names], ref.chr_len, np.ascontiguousarray(ref.codes, dtype=np.uint8), np.zeros((0, 3), np.int64))
    prefix = os.path.join(workdir, "tags_" + tag)
    index_build.build_index_from_genome(g, prefix, device="cpu")
    ix = host.Index(prefix)
    got = pui.ref_of_index(ix)
    assert np.array_equal(got.codes, ref.codes) and got.chr_len == ref.chr_len
    return ix


def sorted_raw(g):
    n, nb = g.bam_sort_finish()
    return g.bam_sort_compress(0, nb, raw=True) if nb else b""


def tagged(g, flags=tgi.ALL):
    nb, st = g.bam_tags_finish(flags=flags)
    return (g.bam_sort_compress(0, nb, raw=True) if nb else b""), st


def check(g, ref, recs, flags=tgi.ALL, shuffle=1):
    """the records through the store, the sort and the stage: the tagged array == the twin over the sorted bytes -> (sorted raw, tagged raw, stats)"""
    recs = list(recs)
    random.Random(shuffle).shuffle(recs)
    g.bam_sort_reset()
    g.bam_sort_add(b"".join(recs), 0)
    raw = sorted_raw(g)
    assert sorted(bsi.split(raw)) == sorted(recs)
    out, st = tagged(g, flags)
    want, t_st = tgi.twin(raw, ref, flags)
    assert out == want and st == t_st
    return raw, out, st


@pytest.fixture(scope="module")
def env(workdir):
    e = Env()
    e.ref = tgi.REF
    e.ix = index_of(workdir, "crafted", e.ref, tgi.NAMES)
    e.gpu = host.DartGPU(e.ix)
    e.cases = tgi.crafted_cases()
    e.rref = pui.random_ref(3, [1700, 1601, 1602])
    e.rix = index_of(workdir, "random", e.rref, [b"c0", b"chr_one", b"2"])
    e.rgpu = host.DartGPU(e.rix)
    rng = random.Random(17)
    e.random = tgi.with_old_tags(pui.random_records(rng, 3000, e.rref), rng)
    yield e
    e.gpu.close(); e.rgpu.close()


@pytest.fixture(scope="module")
def mapped(workdir):
    """one small batch mapped by the device: spliced pairs on a genome of 70 kb, the first five pairs twice more under other names (duplicates), the records unsorted"""
    m = Env()
    m.genome = synth.make_genome([40000, 30000], seed=MAPPER_SEED, repeat_scale=20.0, n_introns=14)
    prefix = os.path.join(workdir, "tags_mapped")
    index_build.build_index_from_genome(m.genome, prefix, device="cpu")
    m.ix = host.Index(prefix)
    m.ref = pui.ref_of_index(m.ix)
    m.n_chr = len(m.ix.names)
    m1, m2 = synth.make_reads(m.genome, 400, rlen=101, seed=MAPPER_SEED + 1, spliced_frac=0.5, indel_frac=0.2, n_frac=0.01)
    arr = host.interleave_pairs(m1, m2)
    reads = np.ascontiguousarray(np.concatenate([arr, arr[0:10], arr[0:10]]))
    headers = ["r%d" % (i // 2) for i in range(len(arr))] + ["copy%d" % (i // 2) for i in range(20)]
    m.gpu = host.DartGPU(m.ix)
    p, _ = common.parse_flags(["-mis", "5"])
    so, rl, flat = host.pack_reads(reads)
    m.gpu.set_params(host.default_params(paired=1, **p))
    m.gpu.map_batch(so, rl, flat)
    m.unsorted, ct = m.gpu.format_bam(headers, ["I" * 101] * len(reads), len(reads), raw=True)
    assert ct["records"] >= len(arr)
    yield m
    m.gpu.close()


def err_of(call):
    with pytest.raises(RuntimeError) as x:
        call()
    m = re.search(r"failed \((-?\d+)\): (.*)", str(x.value), re.S)
    return int(m.group(1)), m.group(2)


@pytest.mark.parametrize("name", ["step", "text", "nm", "ts", "aux", "not_eligible"])
def test_crafted_records_on_the_device_for_all_seven_flag_sets(name, env):
    e = env
    for flags in tgi.FLAG_SETS:
        raw, out, st = check(e.gpu, e.ref, e.cases[name], flags, shuffle=flags)
    if name == "aux":
        assert st[2] == 8 and st[3] == 19                    # (flags 7: the unreadable aux areas, the old tags removed)
    if name == "ts":
        assert st[6] == 21 and st[7] == 3 | 1 << 32
    if name == "nm":
        assert sorted(tgi.nm_of(x) for x in bsi.split(out)) == [0, 255, 255, 256, 256]
    if name == "text":
        longest = max(bsi.split(out), key=len)
        assert tgi.name_of(longest) == b"thousand" and len(tgi.md_of(longest)) == 2001


def test_random_records_and_the_seams_of_the_grid(env):
    e, g = env, env.rgpu
    G, lanes, step = g.bam_tags_granules()
    assert (G, lanes, step) == (256, 16, 16)
    raw, out, st = check(g, e.rref, e.random)
    assert len(raw) > 3 * BLOCK and len(out) > len(raw)                                  # the arrays cross several 0xff00 boundaries
    assert st[0] > 1200 and st[1] > 100 and st[3] >= st[0] and st[4] > 300 and st[5] > 1000 and st[7] & 0xFFFFFFFF > 50
    last = bsi.split(out)[-1]
    assert struct.unpack_from("<i", last, 4)[0] == -1 and last == bsi.split(raw)[-1]     # unplaced records at the end, copied verbatim
    check(g, e.rref, e.random, tgi.MD_ | tgi.TS_, shuffle=2)
    check(g, e.rref, e.random, tgi.NM_, shuffle=3)
    for n in (G - 1, G, G + 1, 2 * G + 1, 1, 16, 17):                                    # a workgroup of the length pass, and of the write pass (G / lanes records), one either side
        check(g, e.rref, e.random[100:100 + n])
    # an empty store: 0 bytes, and nothing to compress
    g.bam_sort_reset()
    assert g.bam_sort_finish() == (0, 0)
    assert g.bam_tags_finish() == (0, (0,) * 8) and g.bam_sort_finish() == (0, 0)


def test_mapper_records(mapped):
    m, g = mapped, mapped.gpu
    g.bam_sort_reset()
    g.bam_sort_add(m.unsorted, 0)
    raw = sorted_raw(g)
    out, st = tagged(g)
    want, t_st = tgi.twin(raw, m.ref, tgi.ALL)
    assert out == want and st == t_st
    recs = bsi.split(want)
    cig_ops = lambda x: {struct.unpack_from("<I", x, 36 + x[12] + 4 * k)[0] & 15 for k in range(x[16] | x[17] << 8)}
    tagged_recs = [x for x in recs if tgi.md_of(x) is not None]
    assert len(tagged_recs) == t_st[0] > 700 and t_st[4] > 100 and t_st[6] > 20
    assert any(re.search(r"[0-9][ACGT][0-9]", tgi.md_of(x)) for x in tagged_recs)                                            # an MD mismatch
    assert any("^" in tgi.md_of(x) and bii.D in cig_ops(x) for x in tagged_recs)                                              # a deletion
    assert any(bii.I in cig_ops(x) and tgi.nm_of(x) > len(re.findall(r"[ACGT]", tgi.md_of(x))) for x in tagged_recs)          # an insertion: NM counts what MD cannot show
    assert any(tgi.ts_of(x) == "+" for x in tagged_recs) and any(tgi.ts_of(x) == "-" for x in tagged_recs)
    # the mapper's NM:i (its count of mismatches) is gone; every rewritten record has exactly one NM and one MD, and AS and XS:i are where they were
    assert t_st[3] == t_st[0] and all(len(tgi.tags_of(x)[b"NM"]) == 1 and list(tgi.tags_of(x))[:2] == [b"AS", b"XS"] for x in tagged_recs)


def test_order_and_repetition(mapped):
    m, g = mapped, mapped.gpu
    g.bam_sort_reset()
    g.bam_sort_add(m.unsorted, 0)
    raw = sorted_raw(g)
    once, st = tagged(g)
    twice, st2 = tagged(g)
    assert twice == once and st2[:3] == st[:3] and st2[4:] == st[4:] and st2[3] > st[3]       # the second call removes what the first appended
    assert sorted_raw(g) == raw                                                               # the store is untouched: the untagged array again
    # tags then marks == marks then tags
    tagged(g)
    md = g.bam_markdup_finish()
    assert md[6] >= 2
    a = g.bam_sort_compress(0, len(once), raw=True)
    sorted_raw(g)
    assert g.bam_markdup_finish() == md
    b, _ = tagged(g)
    assert a == b != once and len(a) == len(once)
    # two contexts merged == one; batches and ordinals do not change a byte
    recs = bsi.split(m.unsorted)
    clone = g.clone()
    try:
        g.bam_sort_reset(); clone.bam_sort_reset()
        # (equal keys keep their input order: ascending ordinal, among equal ordinals the destination's own records first -- the split keeps that order)
        g.bam_sort_add(b"".join(recs[:300]), 0); clone.bam_sort_add(b"".join(recs[300:500]), 0); clone.bam_sort_add(b"".join(recs[500:]), 1)
        g.bam_sort_merge(clone)
        assert sorted_raw(g) == raw and tagged(g)[0] == once
        clone.bam_sort_add(m.unsorted, 0)
        assert sorted_raw(clone) == raw and tagged(clone, tgi.NM_)[0] == tgi.twin(raw, m.ref, tgi.NM_)[0]
    finally:
        clone.close()


def test_later_stages_see_the_new_array(mapped):
    m, g = mapped, mapped.gpu
    g.bam_sort_reset()
    g.bam_sort_add(m.unsorted, 0)
    raw = sorted_raw(g)
    cov = g.bam_coverage_finish()
    pu = g.bam_pileup_finish()
    qc = g.bam_qc_finish()["words"].copy()
    out, st = tagged(g)
    nb = len(out)
    assert nb > len(raw) > 2 * BLOCK
    # the finished track, table and words belonged to the old bytes: gone, as behind a new sort
    assert g.lib.dg_bam_coverage_download(g.ctx, None, 0, None, 0) == ARG and g.lib.dg_bam_pileup_download(g.ctx, None, 0, None, 0) == ARG
    # compressed in pieces and inflated: the tagged bytes; the index is the twin's over the tagged bytes and these block sizes
    z = b"".join(g.bam_sort_compress(off, min(2 * BLOCK, nb - off)) for off in range(0, nb, 2 * BLOCK))
    blocks = bam_decode.bgzf_blocks(z)
    assert b"".join(d for d, _ in blocks) == out
    sizes = [s for _, s in blocks]
    bai = g.bam_index_finish(FIRST)
    assert bai == bii.build_bai(out, sizes, FIRST, m.n_chr) and list(g.bam_index_stats) == bii.twin_stats(out, sizes, FIRST, m.n_chr)
    # coverage, allele counts and QC do not look at tags: equal with and without
    cov2 = g.bam_coverage_finish(); pu2 = g.bam_pileup_finish(); qc2 = g.bam_qc_finish()["words"]
    assert cov2[1] == cov[1] and len(cov[1]) > 1000 and pu2[1] == pu[1] and len(pu[1]) > 100 and np.array_equal(qc2, qc) and qc.sum() > 0
    assert pu2[1] == pui.text_of(pui.twin(out, m.ref)[0], [n if isinstance(n, bytes) else n.encode() for n in m.ix.names])


def test_refusals_leave_the_old_array_usable(env):
    e = env
    g = e.gpu.clone()
    try:
        rc, msg = err_of(lambda: g.bam_tags_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg                                      # no sorted array
        recs = e.cases["text"]
        g.bam_sort_add(b"".join(recs), 0)
        raw = sorted_raw(g)
        for flags in (0, 8, 15, 1 << 31):
            rc, msg = err_of(lambda: g.bam_tags_finish(flags=flags))
            assert rc == ARG and "DG_TAG_MD" in msg
            assert g.bam_sort_compress(0, len(raw), raw=True) == raw
        assert g.lib.dg_bam_tags_finish(g.ctx, 7, None, None, None) == 0                     # every output pointer may be NULL
        n_raw = len(tgi.twin(raw, e.ref, tgi.ALL)[0])
        assert g.bam_sort_compress(0, n_raw, raw=True) == tgi.twin(raw, e.ref, tgi.ALL)[0]
        # a store call in between
        g.bam_sort_add(recs[0], 1)
        rc, msg = err_of(lambda: g.bam_tags_finish())
        assert rc == ARG and "dg_bam_sort_finish" in msg
        raw2 = sorted_raw(g)
        assert len(bsi.split(raw2)) == len(recs) + 1 and tagged(g)[0] == tgi.twin(raw2, e.ref, tgi.ALL)[0]
        ms = (host.C.c_float * 2)()
        assert g.lib.dg_bam_tags_device_ms(g.ctx, ms) == 0 and ms[0] > 0 and ms[1] > 0
        assert g.lib.dg_bam_tags_granules(None) == ARG and g.lib.dg_bam_tags_device_ms(g.ctx, None) == ARG
    finally:
        g.close()
