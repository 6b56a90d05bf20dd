"""GPU suite (-m gpu): coordinate-sorted BAM on the device (dg_batch_accumulate_bam, dg_bam_sort_*; dart_amd/csrc/dg_bamsort.h).  The expectation is always
computed here from the unsorted raw records of the same batches (format_bam(raw=True)): split at block_size, concatenated in ordinal order, stable-sorted
by the key the header defines (tests/bamsort_inputs.py).  No samtools is run: the definition is what is pinned."""
import collections, json, os, re, struct, subprocess, sys
import numpy as np
import pytest
import common, bam_decode
import bamsort_inputs as bsi
import bamidx_inputs as bii
import coverage_inputs as cvi
import markdup_inputs as mdi
from dart_amd import host

pytestmark = pytest.mark.gpu
BLOCK = bsi.BLOCK
ARG = -3


class Env:
    pass


@pytest.fixture(scope="module")
def env(workdir):
    e = Env()
    e.case = common.build_case("pe101_spliced", workdir)
    e.ix = host.Index(e.case["prefix"])
    e.gpu = host.DartGPU(e.ix)
    e.n_chr = len(e.ix.names)
    e.reads, e.headers, e.quals = bsi.sort_reads(e.case)
    e.p, _ = common.parse_flags(e.case["runs"][0]["flags"])
    # the reference both invariance tests compare with, computed once: all reads in one batch, as pairs and as single reads
    e.one = {}
    for paired in (1, 0):
        e.gpu.bam_sort_reset()
        raw = batch(e, e.gpu, 0, len(e.reads), 0, paired)
        e.one[paired] = (raw, sorted_array(e.gpu))
    yield e
    e.gpu.close()


def batch(e, g, lo, hi, ordinal, paired=1, compressed_first=False):
    """maps reads [lo, hi) on g, keeps their records under `ordinal` -> the unsorted raw records"""
    so, rl, flat = host.pack_reads(e.reads[lo:hi])
    g.set_params(host.default_params(paired=paired, **e.p))
    g.map_batch(so, rl, flat)
    npm = hi - lo if paired else 0
    raw, ct = g.format_bam(e.headers[lo:hi], e.quals[lo:hi], npm, raw=True)
    if compressed_first:                                      # the records lie in HBM after a compressing call too
        g.format_bam(e.headers[lo:hi], e.quals[lo:hi], npm)
    assert g.accumulate_bam(ordinal) == ct["records"] == len(bsi.split(raw)) and g.bam_sort_added_bytes == len(raw)
    return raw


def sorted_array(g):
    n, nb = g.bam_sort_finish()
    raw = g.bam_sort_compress(0, nb, raw=True)
    assert len(raw) == nb and len(bsi.split(raw)) == n
    return raw


def inflate(z):
    return b"".join(b for b, _ in bam_decode.bgzf_blocks(z))


def expect(e, segments):
    return b"".join(bsi.expected_sorted(segments, e.n_chr))


def err_of(call):
    """-> (status, text) of a binding call that must fail"""
    with pytest.raises(RuntimeError) as x:
        call()
    m = re.search(r"failed \((-?\d+)\): (.*)", str(x.value), re.S)
    return int(m.group(1)), m.group(2)


def test_sorted_array_equals_the_stable_sort_of_the_unsorted_records(env):
    e = env
    raw, got = e.one[1]
    assert got == expect(e, [(0, raw)])
    # not vacuous
    recs = bsi.split(raw)
    keys = [bsi.key(r, e.n_chr) for r in recs]
    assert keys != sorted(keys), "the unsorted records are in order already"
    placed = collections.Counter(k for k in keys if k >> 33 < e.n_chr)
    assert placed.most_common(1)[0][1] >= 3, "no tie group of three"
    refid = [struct.unpack_from("<i", r, 4)[0] for r in recs]; flag = [struct.unpack_from("<H", r, 18)[0] for r in recs]
    assert -1 in refid and set(range(e.n_chr)) <= set(refid)
    assert any(f & 16 for f in flag) and any(not f & 16 and not f & 4 for f in flag)
    # the BGZF form, with fixed and with dynamic codes (the records go back into the store through the host: the same array)
    e.gpu.bam_sort_reset()
    e.gpu.bam_sort_add(raw, 0)
    n, nb = e.gpu.bam_sort_finish()
    assert (n, nb) == (len(recs), len(raw)) and e.gpu.bam_sort_device_ms > 0 and e.gpu.bam_sort_passes == (33 + e.n_chr.bit_length() + 3) // 4
    fixed = e.gpu.bam_sort_compress(0, nb)
    dyn = e.gpu.bam_sort_compress(0, nb, dynamic=True)
    assert inflate(fixed) == got and inflate(dyn) == got and len(dyn) < len(fixed) < len(got)
    assert len(bam_decode.bgzf_blocks(fixed)) == (nb + BLOCK - 1) // BLOCK
    # the single-read form of the same reads
    raw0, got0 = e.one[0]
    assert got0 == expect(e, [(0, raw0)]) and got0 != got


def test_pieces_give_the_same_compressed_bytes(env):
    e = env
    e.gpu.bam_sort_reset()
    e.gpu.bam_sort_add(e.one[1][0], 0)
    n, nb = e.gpu.bam_sort_finish()
    assert nb > 6 * BLOCK
    for dynamic in (False, True):
        whole = e.gpu.bam_sort_compress(0, nb, dynamic=dynamic)
        for k in (1, 3):
            parts = [e.gpu.bam_sort_compress(off, min(k * BLOCK, nb - off), dynamic=dynamic) for off in range(0, nb, k * BLOCK)]
            assert b"".join(parts) == whole
    assert b"".join(e.gpu.bam_sort_compress(off, min(2 * BLOCK, nb - off), raw=True) for off in range(0, nb, 2 * BLOCK)) == e.one[1][1]


def test_batch_split_clones_and_call_order_do_not_change_a_byte(env):
    e = env
    n = len(e.reads)
    # three uneven batches of single reads, one of them with an odd number of reads; ordinals in ascending read order, calls shuffled
    cuts = [0, 1001, 1001 + 2 * 256 + 6, n]
    assert (cuts[1] - cuts[0]) % 2 == 1
    e.gpu.bam_sort_reset()
    segs = [(k, batch(e, e.gpu, cuts[k], cuts[k + 1], k, paired=0, compressed_first=(k == 1))) for k in (2, 0, 1)]
    got = sorted_array(e.gpu)
    assert got == expect(e, segs) == e.one[0][1]
    # pairs, spread over a parent and a clone, merged in both directions
    cuts = [0, 1400, 1400 + 514, n]
    clone = e.gpu.clone()
    try:
        for into_parent in (True, False):
            e.gpu.bam_sort_reset(); clone.bam_sort_reset()
            segs = []
            for k, g in ((1, clone), (2, e.gpu), (0, clone)):
                segs.append((k, batch(e, g, cuts[k], cuts[k + 1], k)))
            dst, src = (e.gpu, clone) if into_parent else (clone, e.gpu)
            dst.bam_sort_merge(src)
            assert src.bam_sort_info()["records"] == 0 and src.bam_sort_finish() == (0, 0)
            assert dst.bam_sort_info()["segments"] == 3
            assert sorted_array(dst) == expect(e, segs) == e.one[1][1]
    finally:
        clone.close()


def test_equal_ordinals_keep_call_order_and_dst_comes_first_in_a_merge(env):
    e = env
    tie = lambda tag: bsi.record(1, 99, 0, tag, l_seq=3)
    clone = e.gpu.clone()
    try:
        e.gpu.bam_sort_reset(); clone.bam_sort_reset()
        clone.bam_sort_add(tie(b"c0") + tie(b"c1"), 5)
        e.gpu.bam_sort_add(tie(b"p0"), 5)
        clone.bam_sort_add(tie(b"c2"), 4)
        e.gpu.bam_sort_add(tie(b"p1"), 5)
        e.gpu.bam_sort_merge(clone)
        names = [r[36:38] for r in bsi.split(sorted_array(e.gpu))]
        assert names == [b"c2", b"p0", b"p1", b"c0", b"c1"]
    finally:
        clone.close()


def test_store_growth_in_a_fresh_process_changes_nothing(env, workdir):
    """DG_BAMSORT_FIRST_CAP makes the first store 4096 bytes: the child process keeps the same reads in five batches on a parent and a clone, merges and
    sorts; each of the two stores grew (allocate, copy, free) in at least two separate calls, and the bytes are the same"""
    e = env
    npz = os.path.join(workdir, "bamsort_child.npz"); out = os.path.join(workdir, "bamsort_child.bin")
    np.savez(npz, reads=e.reads, headers=np.array(e.headers), quals=np.array(e.quals), p=json.dumps(e.p))
    child_env = dict(os.environ, DG_BAMSORT_FIRST_CAP="1")
    r = subprocess.run([sys.executable, os.path.join(common.HERE, "bamsort_child.py"), e.case["prefix"], npz, out], env=child_env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["growths"] >= 2 and info["clone_growths"] >= 2, info
    assert open(out, "rb").read() == e.one[1][1]


def _descending(n, n_chr):
    """n small records whose keys descend, with many ties (eight records per key)"""
    recs, n_keys = [], (n + 7) // 8
    for i in range(n):
        k = (n - 1 - i) // 8                                  # the key's rank: chromosome, position and strand all grow with it
        recs.append(bsi.record(k * n_chr // n_keys, k // 2, 16 if k & 1 else 0, b"q%d" % i))
    keys = [bsi.key(r, n_chr) for r in recs]
    assert keys == sorted(keys, reverse=True) and len(set(keys)) == n_keys
    return recs


def test_seams_of_the_sorter_through_records_from_the_host(env):
    e = env
    g0, g, smallest = e.gpu.bam_sort_granules()
    assert (g0, g) == (256, 4096) and smallest >= 1
    for n in (g - 1, g, g + 1, 2 * g + 1):
        recs = _descending(n, e.n_chr)
        cut = n // 3
        e.gpu.bam_sort_reset()
        assert e.gpu.bam_sort_add(b"".join(recs[cut:]), 1) == n - cut
        assert e.gpu.bam_sort_add(b"".join(recs[:cut]), 0) == cut
        want = sorted(recs, key=lambda r: bsi.key(r, e.n_chr))
        assert sorted_array(e.gpu) == b"".join(want), n


def _descending_aligned(n, n_chr):
    """_descending's keys and ties, every record placed with one CIGAR op and qualities: the index, the coverage track and the duplicate marker all take it"""
    n_keys = (n + 7) // 8
    recs = [bii.record(k * n_chr // n_keys, k // 2, 16 if k & 1 else 0, b"q%d" % i, [(20, bii.M)], l_seq=20, mapq=30, fill=30)
            for i, k in ((i, (n - 1 - i) // 8) for i in range(n))]
    assert len({struct.unpack_from("<i", r, 4)[0] for r in recs[::max(n // 64, 1)]}) >= 2
    return recs


@pytest.mark.parametrize("n", [65535, 65536, 65537, 131073])
def test_more_than_256_workgroup_sums_carry_through_the_tile_sum_scans(env, n):
    """One record per lane: 65 536 records are 256 workgroup sums, the last size that k_tiles_top (both widths) and k_cv_top scan without a carry; 65 537 and
    131 073 give 257 and 513.  Store, index, coverage track (entries only) and duplicate counts of the same array, each against its Python twin."""
    e, g = env, env.gpu
    assert e.n_chr >= 2
    recs = _descending_aligned(n, e.n_chr)
    cut = n // 3
    g.bam_sort_reset()
    assert g.bam_sort_add(b"".join(recs[cut:]), 1) == n - cut
    assert g.bam_sort_add(b"".join(recs[:cut]), 0) == cut
    raw = sorted_array(g)
    assert raw == b"".join(sorted(recs, key=lambda r: bsi.key(r, e.n_chr)))
    sizes = bii.stored_sizes(raw)
    assert g.bam_index_finish(1 << 40, sizes) == bii.build_bai(raw, sizes, 1 << 40, e.n_chr)
    ent, text = g.bam_coverage_finish(entries_only=True)
    t_ent, t_stats = cvi.twin(raw, e.n_chr)
    assert ent.tolist() == t_ent and text == b"" and g.bam_coverage_stats == t_stats and t_stats[0] == n and len(t_ent) > 2 * e.n_chr
    stats = mdi.twin(raw, e.n_chr)[1]
    assert g.bam_markdup_finish(count_only=True) == stats and stats[0] == stats[2] == n and stats[4] == n - (n + 7) // 8
    assert g.bam_sort_compress(0, len(raw), raw=True) == raw


def test_seams_of_the_key_kernels_through_batches(env):
    e = env
    g0 = e.gpu.bam_sort_granules()[0]
    e.gpu.bam_sort_reset()
    segs, lo = [], 0
    for k, n in enumerate((g0 - 1, g0, g0 + 1)):
        segs.append((k, batch(e, e.gpu, lo, lo + n, k, paired=0)))
        lo += n
    assert sorted_array(e.gpu) == expect(e, segs)


def test_no_record_one_record_and_arrays_around_one_block(env):
    e = env
    e.gpu.bam_sort_reset()
    assert e.gpu.bam_sort_finish() == (0, 0) and e.gpu.bam_sort_compress(0, 0) == b"" and e.gpu.bam_sort_compress(0, 0, raw=True) == b""
    assert e.gpu.bam_sort_add(b"", 0) == 0 and e.gpu.bam_sort_finish() == (0, 0)
    one = bsi.record(1, 7, 16, b"only", l_seq=5)
    e.gpu.bam_sort_add(one, 3)
    assert sorted_array(e.gpu) == one and inflate(e.gpu.bam_sort_compress(0, len(one))) == one
    for total in (BLOCK - 1, BLOCK, BLOCK + 1):
        recs = [bsi.record(i % 2, 5000 - i, 0, b"w%03d" % i, l_seq=101, fill=0x21) for i in range(200)]
        size = sum(len(r) for r in recs)
        recs.append(bsi.record(0, 0, 0, b"filler", tags=b"ZZZ" + b"t" * (total - size - 36 - 7 - 4) + b"\0"))
        assert sum(len(r) for r in recs) == total
        e.gpu.bam_sort_reset()
        e.gpu.bam_sort_add(b"".join(recs), 0)
        n, nb = e.gpu.bam_sort_finish()
        assert nb == total
        want = b"".join(sorted(recs, key=lambda r: bsi.key(r, e.n_chr)))
        z = e.gpu.bam_sort_compress(0, nb)
        assert inflate(z) == want and [len(b) for b, _ in bam_decode.bgzf_blocks(z)] == ([total] if total <= BLOCK else [BLOCK, 1])
        assert inflate(e.gpu.bam_sort_compress(0, nb, dynamic=True)) == want


def _still_sorts(e, g):
    """after a refused call: the context maps a batch, keeps it and sorts it"""
    g.bam_sort_reset()
    raw = batch(e, g, 0, 400, 0)
    assert sorted_array(g) == expect(e, [(0, raw)])


def test_calls_and_refusals(env):
    e = env
    g = e.gpu.clone()
    try:
        # finish twice; finish, more batches, finish; reset
        g.bam_sort_reset()
        a = batch(e, g, 0, 300, 1)
        first = sorted_array(g)
        assert sorted_array(g) == first == expect(e, [(1, a)])
        b = batch(e, g, 300, 700, 0)
        assert sorted_array(g) == expect(e, [(1, a), (0, b)])
        g.bam_sort_reset()
        assert g.bam_sort_info()["records"] == 0 and g.bam_sort_finish() == (0, 0)
        # a batch is added once
        batch(e, g, 0, 200, 0)
        rc, msg = err_of(lambda: g.accumulate_bam(1))
        assert rc == ARG and "already" in msg and g.bam_sort_info()["segments"] == 1
        _still_sorts(e, g)
        # no formatted batch: after the upload, after the run, after a SAM text, after dg_bgzf_compress alone
        so, rl, flat = host.pack_reads(e.reads[:200])
        g.upload(so, rl, flat)
        rc, msg = err_of(lambda: g.accumulate_bam(0))
        assert rc == ARG and "dg_batch_format_bam" in msg
        g.run()
        assert err_of(lambda: g.accumulate_bam(0))[0] == ARG
        g.bgzf_compress(b"some bytes, no batch of records")
        assert err_of(lambda: g.accumulate_bam(0))[0] == ARG
        g.format_bam(e.headers[:200], e.quals[:200], 200, raw=True)
        g.format_sam(e.headers[:200], e.quals[:200], 200)            # (reuses the per-read offsets)
        assert err_of(lambda: g.accumulate_bam(0))[0] == ARG
        _still_sorts(e, g)
        # ranges of the sorted array
        n, nb = g.bam_sort_finish()
        assert nb > BLOCK
        for off, length in ((1, BLOCK), (BLOCK - 4, 4), (0, BLOCK - 1), (0, nb + 1), (2 * BLOCK * (nb // BLOCK), 0)):
            rc, msg = err_of(lambda: g.bam_sort_compress(off, length))
            assert rc == ARG and "multiple" in msg, (off, length)
        assert inflate(g.bam_sort_compress(BLOCK, nb - BLOCK)) == g.bam_sort_compress(BLOCK, nb - BLOCK, raw=True)
        assert g.lib.dg_bam_sort_compress(g.ctx, 0, nb, 7, None, None) == ARG
        _still_sorts(e, g)
        # the sorted array ends with the next store call
        g.bam_sort_add(bsi.record(0, 1, 0), 9)
        rc, msg = err_of(lambda: g.bam_sort_compress(0, 0))
        assert rc == ARG and "dg_bam_sort_finish" in msg
        # merge with itself
        rc, msg = err_of(lambda: g.bam_sort_merge(g))
        assert rc == ARG and "differ" in msg
        _still_sorts(e, g)
        # records from outside that break a rule: refused whole, the text names the record
        for name, (data, why, bad) in sorted(bsi.malformed_cases(e.n_chr).items()):
            before = g.bam_sort_info()
            rc, msg = err_of(lambda: g.bam_sort_add(data, 2))
            assert rc == ARG and "record %d:" % bad in msg and "nothing was added" in msg, (name, msg)
            assert g.bam_sort_info() == before
            _still_sorts(e, g)
    finally:
        g.close()
