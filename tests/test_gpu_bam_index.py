"""GPU suite (-m gpu): the BAM index of the coordinate-sorted BAM, built on the device (dg_bam_index_*; dart_amd/csrc/dg_bamidx.h).  The expectation is always
the sequential Python twin of tests/bamidx_inputs.py over the sorted raw array and the block sizes read from the compressed bytes; an independent reader
answers region queries through the device's index.  No samtools is run: the definition in the header is what is pinned."""
import random, re, struct
import numpy as np
import pytest
import common, bam_decode
import bamsort_inputs as bsi
import bamidx_inputs as bii
from dart_amd import host

pytestmark = pytest.mark.gpu
BLOCK = bii.BLOCK
ARG, CAPACITY, RANGE = -3, -4, -6
FIRST = 1234                                                   # a first_block_offset: where the records' blocks would begin in a file


class Env:
    pass


def batch(e, g, lo, hi, ordinal, paired=1):
    so, rl, flat = host.pack_reads(e.reads[lo:hi])
    g.set_params(host.default_params(paired=paired, **e.p))
    g.map_batch(so, rl, flat)
    raw, ct = g.format_bam(e.headers[lo:hi], e.quals[lo:hi], hi - lo if paired else 0, raw=True)
    assert g.accumulate_bam(ordinal) == ct["records"]
    return raw


def sizes_of(z):
    return [s for _, s in bam_decode.bgzf_blocks(z)]


def finish_compress_index(g, first=FIRST, dynamic=False, piece=None):
    """-> (sorted raw array, compressed bytes, the device's index)"""
    n, nb = g.bam_sort_finish()
    raw = g.bam_sort_compress(0, nb, raw=True)
    piece = nb if piece is None else piece
    z = b"".join(g.bam_sort_compress(off, min(piece, nb - off), dynamic=dynamic) for off in range(0, nb, max(piece, 1)))
    return raw, z, g.bam_index_finish(first)


@pytest.fixture(scope="module")
def env(workdir):
    e = Env()
    e.case = common.build_case("pe101_spliced", workdir)
    e.ix = host.Index(e.case["prefix"])
    e.gpu = host.DartGPU(e.ix)
    e.n_chr = len(e.ix.names)
    assert e.n_chr == 2
    e.reads, e.headers, e.quals = bsi.sort_reads(e.case)
    e.p, _ = common.parse_flags(e.case["runs"][0]["flags"])
    e.unsorted = {}
    for paired in (1, 0):
        e.gpu.bam_sort_reset()
        e.unsorted[paired] = batch(e, e.gpu, 0, len(e.reads), 0, paired)
    # the store most tests index, computed once: the mapped pairs, and hand-made records for what they lack -- a record far behind the chromosome's end (pos
    # is not checked against its length): the windows in between are filled from their predecessor
    e.extra = bii.record(1, 200000 + 5 * 16384 + 3, 0, b"far_behind", [(50, bii.M)], l_seq=50) + bii.record(0, 70000, 4, b"placed_unmapped_by_hand", l_seq=10)
    e.gpu.bam_sort_reset()
    e.gpu.bam_sort_add(e.unsorted[1], 0); e.gpu.bam_sort_add(e.extra, 1)
    e.raw, e.z, e.bai = finish_compress_index(e.gpu)
    e.stats = e.gpu.bam_index_stats
    yield e
    e.gpu.close()


def err_of(call):
    with pytest.raises(RuntimeError) as x:
        call()
    m = re.search(r"failed \((-?\d+)\): (.*)", str(x.value), re.S)
    return int(m.group(1)), m.group(2)


def test_index_equals_the_twin_for_fixed_and_dynamic_codes_and_single_reads(env):
    e = env
    seen = []
    for paired, dynamic in ((1, False), (1, True), (0, False)):
        e.gpu.bam_sort_reset()
        e.gpu.bam_sort_add(e.unsorted[paired], 0)
        raw, z, bai = finish_compress_index(e.gpu, dynamic=dynamic)
        assert raw == b"".join(bsi.expected_sorted([(0, e.unsorted[paired])], e.n_chr))
        sizes = sizes_of(z)
        assert len(sizes) == (len(raw) + BLOCK - 1) // BLOCK > 6
        assert bai == bii.build_bai(raw, sizes, FIRST, e.n_chr)
        assert list(e.gpu.bam_index_stats) == bii.twin_stats(raw, sizes, FIRST, e.n_chr) and e.gpu.bam_index_device_ms > 0
        seen.append(bai)
    assert len(set(seen)) == 3                                # other block sizes, other offsets: the two codes' indices differ
    # the call may be repeated, with the caller's sizes too; the recorded sizes are those of the last compress of each block
    assert e.gpu.bam_index_finish(FIRST) == seen[2] == e.gpu.bam_index_finish(FIRST, sizes)
    assert e.gpu.bam_index_finish(FIRST + 1) != seen[2]


def test_the_index_of_the_mapped_reads_is_not_vacuous(env):
    e = env
    sizes = sizes_of(e.z)
    assert e.bai == bii.build_bai(e.raw, sizes, FIRST, e.n_chr) and list(e.stats) == bii.twin_stats(e.raw, sizes, FIRST, e.n_chr)
    ix = bii.parse_bai(e.bai)
    assert all(len(r["bins"]) > 1 and r["pseudo"] is not None for r in ix["refs"])                     # both references have bins
    assert any(num < 4681 for r in ix["refs"] for num, _ in r["bins"])                                  # a chunk in a bin above level 5
    assert e.stats[3] > e.stats[4]                                                                      # a neighbour merge happened
    assert any(len(chunks) > 1 for r in ix["refs"] for _, chunks in r["bins"])                          # and a pair of chunks of one bin was not merged
    intv = ix["refs"][1]["intv"]
    assert len(intv) == (200000 + 5 * 16384 + 52) // 16384 + 1 and intv[-2] == intv[-3] != intv[-1]    # windows filled from their predecessor
    assert ix["n_no_coor"] == e.stats[1] > 0
    f = [bii.fields(e.raw, at, e.n_chr) for at in bii.offsets(e.raw)]
    names = [e.raw[at + 36:at + 36 + e.raw[at + 12] - 1] for at in bii.offsets(e.raw)]
    placed_unmapped = [nm for x, nm in zip(f, names) if x["placed"] and not x["mapped"]]
    assert b"placed_unmapped_by_hand" in placed_unmapped                                                # (the mapper leaves the random mate of sort_reads' "half" pair unplaced)
    assert sum(r["pseudo"][3] for r in ix["refs"]) == len(placed_unmapped)
    assert any(x["rlen"] > 101 for x in f)                                                              # introns: records of several CIGAR ops


def test_region_queries_through_the_index_find_what_a_scan_finds(env):
    e = env
    bam = bytes(FIRST) + e.z                                   # the blocks where the index says they are; the bytes in front are never read
    scanned = bii.scan(e.raw, e.n_chr)
    rng = random.Random(3)
    lens = [300000, 200000]
    hits = empty = 0
    for t in range(e.n_chr):
        regions = [(0, 1), (16383, 16385), (lens[t] - 1, lens[t])]
        if t == 1:
            regions += [(200000 + 2 * 16384 + 5, 200000 + 2 * 16384 + 900), (200000 + 5 * 16384, 200000 + 5 * 16384 + 10)]        # inside a filled window; the record behind it
        for _ in range(200):
            b = rng.randrange(0, lens[t]); regions.append((b, b + rng.choice([1, 30, 500, 20000])))
        for b, en in regions:
            want = bii.brute(e.raw, e.n_chr, t, b, en, scanned)
            assert bii.query(e.bai, bam, t, b, en) == want, (t, b, en)
            hits += len(want); empty += not want
    assert hits > 1000 and empty >= 1
    assert bii.query(e.bai, bam, 1, 200000 + 5 * 16384, 200000 + 5 * 16384 + 10)[0][36:46] == b"far_behind"


def test_pieces_batches_and_contexts_do_not_change_a_byte(env):
    e = env
    e.gpu.bam_sort_reset()
    e.gpu.bam_sort_add(e.unsorted[1], 0); e.gpu.bam_sort_add(e.extra, 1)
    for k in (1, 3):
        raw, z, bai = finish_compress_index(e.gpu, piece=k * BLOCK)
        assert (raw, z, bai) == (e.raw, e.z, e.bai), k
    # the same reads in uneven batches on a parent and a clone, merged
    n = len(e.reads)
    cuts = [0, 1400, 1400 + 514, n]
    clone = e.gpu.clone()
    try:
        e.gpu.bam_sort_reset(); clone.bam_sort_reset()
        for k, g in ((1, clone), (2, e.gpu), (0, clone)):
            batch(e, g, cuts[k], cuts[k + 1], k)
        e.gpu.bam_sort_add(e.extra, 3)
        e.gpu.bam_sort_merge(clone)
        raw, z, bai = finish_compress_index(e.gpu, piece=2 * BLOCK)
        assert raw == e.raw and bai == e.bai
        # the clone indexes too, and a context's index does not depend on what it indexed before
        clone.bam_sort_add(e.unsorted[0], 0)
        raw0, z0, bai0 = finish_compress_index(clone)
        assert bai0 == bii.build_bai(raw0, sizes_of(z0), FIRST, e.n_chr) != e.bai
    finally:
        clone.close()


def _one_bin_each(n, n_chr, tag=b"s"):
    """n records, each in a 16 kb bin of its own (pos is not checked against the chromosome's length): n chunks, none merged with a neighbour of its bin"""
    half = (n + 1) // 2
    return [bii.record(k // half % n_chr, (k % half) * 16384 + 5, 16 if k & 1 else 0, tag + b"%d" % k, [(20, bii.M)], l_seq=20) for k in range(n)]


def _index_with_given_sizes(e, recs, first):
    raw = b"".join(sorted(recs, key=lambda r: bsi.key(r, e.n_chr)))
    e.gpu.bam_sort_reset()
    cut = len(recs) // 3
    e.gpu.bam_sort_add(b"".join(recs[cut:]), 1); e.gpu.bam_sort_add(b"".join(recs[:cut]), 0)
    n, nb = e.gpu.bam_sort_finish()
    assert e.gpu.bam_sort_compress(0, nb, raw=True) == raw
    sizes = bii.stored_sizes(raw)
    bai = e.gpu.bam_index_finish(first, sizes)
    assert bai == bii.build_bai(raw, sizes, first, e.n_chr), len(recs)
    assert list(e.gpu.bam_index_stats) == bii.twin_stats(raw, sizes, first, e.n_chr)
    return raw, sizes, bai


def test_seams_of_the_sorter_the_record_kernel_and_the_blocks(env):
    e = env
    g0, g = e.gpu.bam_index_granules()
    assert (g0, g) == (256, 4096)
    for n in (g - 1, g, g + 1, 2 * g + 1):                     # chunks around the sorter's tile; caller-given sizes and offsets of 48 bits
        _index_with_given_sizes(e, _one_bin_each(n, e.n_chr), 1 << 40)
        assert e.gpu.bam_index_stats[3] == e.gpu.bam_index_stats[4] == e.gpu.bam_index_stats[2] == n
    for n in (g0 - 1, g0, g0 + 1):                             # records around k_bi_rec's workgroup, a few of them unplaced
        recs = _one_bin_each(n - 3, e.n_chr) + [bii.record(-1, -1, 4, b"u%d" % k, l_seq=4) for k in range(3)]
        _index_with_given_sizes(e, recs, 0)
        assert e.gpu.bam_index_stats[:2] == (n - 3, 3)
    for total in (BLOCK - 1, BLOCK, BLOCK + 1):                # arrays around one block: voff of the last record's end
        recs = [bii.record(i % 2, 5000 - i, 0, b"w%03d" % i, [(101, bii.M)], l_seq=101, fill=0x21) for i in range(200)]
        size = sum(len(r) for r in recs)
        recs.append(bsi.record(0, 0, 0, b"filler", tags=b"ZZZ" + b"t" * (total - size - 36 - 7 - 4) + b"\0"))
        assert sum(len(r) for r in recs) == total
        raw, sizes, bai = _index_with_given_sizes(e, recs, 1 << 40)
        assert len(sizes) == (1 if total <= BLOCK else 2)
        last_end = bii.parse_bai(bai)["refs"][1]["pseudo"][1]
        assert last_end == ((1 << 40) + sum(sizes)) << 16      # the array's end reads as the start of what follows the last block


def _still_indexes(e, g):
    """after a refused call: the context maps a batch, keeps it, sorts it and indexes it"""
    g.bam_sort_reset()
    batch(e, g, 0, 400, 0)
    raw, z, bai = finish_compress_index(g)
    assert bai == bii.build_bai(raw, sizes_of(z), FIRST, e.n_chr)


def test_empty_one_record_and_refusals(env):
    e = env
    g = e.gpu.clone()
    try:
        # no finish at all on a fresh context
        rc, msg = err_of(lambda: g.bam_index_finish(0))
        assert rc == ARG and "dg_bam_sort_finish" in msg
        _still_indexes(e, g)
        # an empty store
        g.bam_sort_reset()
        assert g.bam_sort_finish() == (0, 0)
        empty = g.bam_index_finish(99)
        assert empty == bii.build_bai(b"", [], 99, e.n_chr) and len(empty) == 8 + 8 * e.n_chr + 8 and g.bam_index_stats == (0,) * 6
        assert g.bam_index_finish(99, []) == empty
        # one record
        one = bii.record(1, 7, 16, b"only", [(5, bii.M)], l_seq=5)
        g.bam_sort_add(one, 3)
        raw, z, bai = finish_compress_index(g)
        assert raw == one and bai == bii.build_bai(one, sizes_of(z), FIRST, e.n_chr) and g.bam_index_stats == (1, 0, 1, 1, 1, 1)
        # a store call behind the finish
        g.bam_sort_add(one, 4)
        rc, msg = err_of(lambda: g.bam_index_finish(0))
        assert rc == ARG and "dg_bam_sort_finish" in msg
        _still_indexes(e, g)
        # a block never compressed: the text names it; only raw pieces; the marks end with the next finish
        g.bam_sort_reset()
        g.bam_sort_add(e.unsorted[1], 0)
        n, nb = g.bam_sort_finish()
        assert nb > 3 * BLOCK
        rc, msg = err_of(lambda: g.bam_index_finish(0))
        assert rc == ARG and "block 0 " in msg
        _still_indexes(e, g)
        g.bam_sort_reset()
        g.bam_sort_add(e.unsorted[1], 0)
        assert g.bam_sort_finish()[1] == nb
        g.bam_sort_compress(0, BLOCK); g.bam_sort_compress(2 * BLOCK, nb - 2 * BLOCK)
        rc, msg = err_of(lambda: g.bam_index_finish(0))
        assert rc == ARG and "block 1 " in msg
        g.bam_sort_compress(BLOCK, BLOCK)
        whole = g.bam_index_finish(0)
        g.bam_sort_finish()
        g.bam_sort_compress(0, nb, raw=True)
        rc, msg = err_of(lambda: g.bam_index_finish(0))
        assert rc == ARG and "block 0 " in msg
        _still_indexes(e, g)
        g.bam_sort_reset()
        g.bam_sort_add(e.unsorted[1], 0)
        assert g.bam_sort_finish()[1] == nb
        z = g.bam_sort_compress(0, nb)
        assert g.bam_index_finish(0) == whole == bii.build_bai(g.bam_sort_compress(0, nb, raw=True), sizes_of(z), 0, e.n_chr)
        # the caller's sizes: a wrong count, a zero
        n_blocks = (nb + BLOCK - 1) // BLOCK
        rc, msg = err_of(lambda: g.bam_index_finish(0, [100] * (n_blocks + 1)))
        assert rc == ARG and "n_blocks" in msg
        assert err_of(lambda: g.bam_index_finish(0, [100] * (n_blocks - 1)))[0] == ARG
        rc, msg = err_of(lambda: g.bam_index_finish(0, [100] * (n_blocks - 1) + [0]))
        assert rc == ARG and "block %d " % (n_blocks - 1) in msg
        _still_indexes(e, g)
        g.bam_sort_reset()
        g.bam_sort_add(e.unsorted[1], 0)
        assert g.bam_sort_finish()[1] == nb
        # offsets that need more than 48 bits
        assert err_of(lambda: g.bam_index_finish(1 << 48, [100] * n_blocks))[0] == RANGE
        assert err_of(lambda: g.bam_index_finish((1 << 48) - 150, [100] * n_blocks))[0] == RANGE
        # the download's capacity
        assert g.bam_index_finish(0, [100] * n_blocks)
        buf = np.zeros(64, np.uint8)
        assert g.lib.dg_bam_index_download(g.ctx, buf.ctypes.data, 63) == CAPACITY and not buf.any()
        _still_indexes(e, g)
        # a placed record that ends behind 2^29: refused with its index, and nothing is left behind; end = 2^29 itself is taken
        recs = [bii.record(0, 5, 0, b"a", [(9, bii.M)], l_seq=9), bii.record(0, bii.MAX_END - 40, 0, b"fits", [(40, bii.M)], l_seq=40),
                bii.record(1, bii.MAX_END - 40, 0, b"too_far", [(41, bii.M)], l_seq=41), bii.record(-1, -1, 4, b"u")]
        g.bam_sort_reset()
        g.bam_sort_add(b"".join(recs), 0)
        n, nb = g.bam_sort_finish()
        rc, msg = err_of(lambda: g.bam_index_finish(0, [77]))
        assert rc == RANGE and "record 2 " in msg and "CSI" in msg
        assert g.lib.dg_bam_index_download(g.ctx, buf.ctypes.data, 64) == ARG
        assert g.bam_sort_compress(0, nb, raw=True) == b"".join(recs)        # the sorted array stays
        g.bam_sort_reset()
        g.bam_sort_add(b"".join(recs[:2] + recs[3:]), 0)
        g.bam_sort_finish()
        assert g.bam_index_finish(0, [77]) == bii.build_bai(b"".join(recs[:2] + recs[3:]), [77], 0, e.n_chr)
        _still_indexes(e, g)
    finally:
        g.close()
