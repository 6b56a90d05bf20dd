"""GPU suite (-m gpu): transcript-level expression on the device (dg_tx_*, dart_amd/csrc/dg_txquant.h) against the sequential Python twin of
tests/txquant_inputs.py over the records downloaded the old way: the class table as a dictionary, its eight words, and the EM's words, which must equal the
twin's exactly.  The definition is the header's comment; no quantification tool is run."""
import ctypes as C
import json, os, subprocess, sys
import numpy as np
import pytest
import common
import genecount_inputs as gci
import txquant_inputs as txi
from txquant_inputs import M, N
from dart_amd import host

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_CAPACITY = -3, -4
MIN_MAPQ = txi.MIN_MAPQ
CASES = ["se100", "pe101_spliced", "pe151_spliced"]


def _params(c):
    return host.default_params(paired=1 if c["spec"]["paired"] else 0, max_mismatch=5)


def _table(g):
    off, ids, cnt, words = g.tx_classes()
    return txi.table_dict(off, ids, cnt), [int(x) for x in words]


@pytest.fixture(scope="module")
def small(workdir):
    """the smallest golden index: a root context and two clones"""
    c = common.build_case("se100", workdir)
    ix = host.Index(c["prefix"])
    gpu = host.DartGPU(ix, _params(c))
    yield c, ix, gpu, gpu.clone(), gpu.clone()
    gpu.close()


@pytest.mark.parametrize("name", CASES)
def test_mapped_batches_equal_the_twin_whatever_the_split(name, workdir):
    c = common.build_case(name, workdir)
    n_chr = len(c["genome"].lengths)
    tr = txi.case_annotation(c, txi.CASE_SEEDS[name])
    tx, ex = txi.annot_arrays(tr)
    L = txi.lengths(tr)
    arr, npm = gci.case_batch(c)
    ix = host.Index(c["prefix"])
    gpu = host.DartGPU(ix, _params(c))
    try:
        n_merged, n_seg = gpu.tx_set_annotation(tx, ex)
        assert n_merged == sum(len(txi.merged(e)) for _, _, e in tr) and n_seg > 0
        # one batch
        res = gpu.map_batch(*host.pack_reads(arr))
        n_units = gpu.accumulate_tx(npm, MIN_MAPQ, 0)
        one = _table(gpu)
        want = txi.twin(tr, n_chr, res.reads, res.reports, res.cigar, npm, MIN_MAPQ)
        classes, words = want
        print(name, "units", n_units, "words", words, "classes", len(classes), "device ms", gpu.tx_device_ms_split)
        assert txi.rich_enough(tr, classes, words, npm > 0), (words, len(classes))          # by the twin alone
        assert n_units == len(gci.units_of(len(arr), npm)) == words[0]
        assert one[1] == words and one[0] == classes
        # the EM: the start values, one look at the flag, and to convergence; the words equal the twin's, bit for bit
        for rounds in (0, 16, 1000):
            got = [int(x) for x in gpu.tx_finish(200, rounds)]
            ref = txi.em(classes, words, L, 200, rounds)
            print(name, "max_rounds", rounds, "rounds", got[len(L) + 8], "converged", got[len(L) + 9], "EM ms", gpu.tx_em_device_ms)
            assert got == ref, [(t, a, b) for t, (a, b) in enumerate(zip(got, ref)) if a != b][:5]
        assert _table(gpu) == (classes, words)                      # the EM leaves the class table as it was
        names = ["T%05d" % t for t in range(len(L))]
        assert gpu.tx_text(np.array(ref, np.uint64), tx, ex, names) == txi.text(ref, L, names)
        # three batches over a root and two clones (which count with the root's annotation), merged
        ctxs = [gpu, gpu.clone(), gpu.clone()]
        gpu.tx_reset()
        cut = [0, len(arr) // 3 // 2 * 2, len(arr) // 3 // 2 * 4 + 2, len(arr)]
        for g, lo, hi in zip(ctxs[::-1], cut[:-1], cut[1:]):
            g.set_params(_params(c))
            g.map_batch(*host.pack_reads(arr[lo:hi]))
            g.accumulate_tx(hi - lo if npm else 0, MIN_MAPQ, 0)
        gpu.tx_merge(ctxs[2]); gpu.tx_merge(ctxs[1])
        assert _table(gpu) == (classes, words)
        assert _table(ctxs[1]) == ({}, [0] * 8) and _table(ctxs[2]) == ({}, [0] * 8)      # after the merge the source is empty
        assert [int(x) for x in gpu.tx_finish(200, 1000)] == ref
        # the downloaded records fed back through dg_tx_count_records, on a clone; a downloaded table added to an empty one and to itself
        assert ctxs[1].tx_count_records(res.reads, res.reports, res.cigar, npm, MIN_MAPQ, 0) == n_units
        assert _table(ctxs[1]) == (classes, words)
        off, ids, cnt, w8 = ctxs[1].tx_classes()
        ctxs[2].tx_add(off, ids, cnt, w8)
        assert _table(ctxs[2]) == (classes, words)
        ctxs[2].tx_add(off, ids, cnt, w8)
        assert _table(ctxs[2]) == txi.add_tables(want, want)
        # the strand modes
        for mode in (1, 2):
            ctxs[1].tx_reset()
            ctxs[1].tx_count_records(res.reads, res.reports, res.cigar, npm, MIN_MAPQ, mode)
            w = txi.twin(tr, n_chr, res.reads, res.reports, res.cigar, npm, MIN_MAPQ, mode)
            assert _table(ctxs[1]) == w and w[0] != classes
            assert [int(x) for x in ctxs[1].tx_finish(200, 16)] == txi.em(w[0], w[1], L, 200, 16, mode)
    finally:
        gpu.close()


def _expect_seams(tabs, granule, wave):
    """the crafted runs against the ladder's arithmetic and the twin"""
    by = {t[0]: t for t in tabs}
    seqs = txi.seam_sequences(granule, wave)
    ladder_tr = [(0, 0, [(100 + 20 * t, 110 + 20 * t)]) for t in range(400)]
    for tag, ts in seqs.items():
        classes, words = txi.ladder_expected(ts)
        assert by[tag][1] == classes and by[tag][2] == words, tag
        if len(ts) <= 3000:                                          # the expectation itself against the twin, on the first 400 transcripts
            assert txi.twin(ladder_tr, 1, *txi.ladder_units(ts), 0, MIN_MAPQ) == (classes, words), tag
            assert by[tag][3][:400] == txi.em(classes, words, [10] * 400, 200, 16)[:400] and by[tag][3][txi.SEAM_TX:] == txi.em(classes, words, [10] * 400, 200, 16)[400:], tag
    assert by["seams in two calls"][1:3] == by["seams"][1:3]
    assert by["one class"][3][3] == 100000 << 20 and sum(by["every unit its own class"][3][:txi.SEAM_TX]) == 100000 << 20
    rd, rp, cg = txi.ladder_units(seqs["seams"][:2 * granule + 2])
    rp["flag"] = np.where(np.arange(len(rp)) & 1, 0x91, 0x61)
    want = txi.twin(ladder_tr, 1, rd, rp, cg, len(rd), MIN_MAPQ)
    assert by["pairs"][1] == want[0] and by["pairs"][2] == want[1] and want[1][6] > 0 and want[1][3] > 0
    fan = txi.fan(300)
    rd, rp, cg, npm = txi.fan_records(granule)
    want = txi.twin(fan, 1, rd, rp, cg, npm, MIN_MAPQ)
    assert by["fan"][1] == want[0] and by["fan"][2] == want[1] and max(len(k) for k in want[0]) == 300
    assert by["fan"][3] == txi.em(want[0], want[1], txi.lengths(fan), 200, 16)


def test_crafted_records_on_the_kernels_seams_with_and_without_colliding_hashes(small, workdir):
    c, ix, gpu, _, _ = small
    granule, wave = gpu.tx_granules()
    assert granule >= wave >= 32 and granule % wave == 0
    tabs = txi.seam_tables(gpu)
    _expect_seams(tabs, granule, wave)
    # all of it again in a fresh process whose hashes keep four bits: every build meets colliding hashes and is finished exactly; the tables are equal
    out = os.path.join(workdir, "tx_child.json")
    env = dict(os.environ, DG_TX_HASH_BITS="4")
    r = subprocess.run([sys.executable, os.path.join(common.HERE, "txquant_inputs.py"), c["prefix"], out], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    child = json.load(open(out))
    assert len(child) == len(tabs)
    for (tag, classes, words, res), (ctag, ccl, cwords, cres) in zip(tabs, child):
        assert tag == ctag and words == cwords and res == cres, tag
        assert classes == {tuple(k): v for k, v in ccl}, tag


def test_error_cases_leave_the_table_as_it_was(small):
    c, ix, gpu, cl1, cl2 = small
    lib = gpu.lib
    err = lambda g: lib.dg_last_error(g.ctx)
    n_units = C.c_size_t(7)
    tr = txi.case_annotation(c, txi.CASE_SEEDS["se100"])
    tx, ex = txi.annot_arrays(tr)
    # no annotation: a root of its own (the annotation lives with the index)
    fresh = host.DartGPU(ix, _params(c))
    try:
        fresh.map_batch(*host.pack_reads(c["reads"][:100]))
        assert lib.dg_batch_accumulate_tx(fresh.ctx, 0, MIN_MAPQ, 0, C.byref(n_units)) == ERR_ARG and b"annotation" in err(fresh) and n_units.value == 0
        assert lib.dg_tx_reset(fresh.ctx) == ERR_ARG and lib.dg_tx_finish(fresh.ctx, 0, 200, 10, None, None) == ERR_ARG
        fresh2 = fresh.clone()
        fresh.tx_set_annotation(tx, ex)
        assert lib.dg_batch_accumulate_tx(fresh2.ctx, 0, MIN_MAPQ, 0, None) == ERR_ARG and b"no finished batch" in err(fresh2)
        assert _table(fresh2) == ({}, [0] * 8)
    finally:
        fresh.close()
    gpu.tx_set_annotation(tx, ex)
    for g in (gpu, cl1, cl2):
        g.set_params(_params(c)); g.tx_reset()
    reads = c["reads"][:500]
    res = gpu.map_batch(*host.pack_reads(reads))
    assert gpu.accumulate_tx(0, MIN_MAPQ, 0) == 500
    before = _table(gpu)
    assert before[1][0] == 500 and before == txi.twin(tr, 1, res.reads, res.reports, res.cigar, 0, MIN_MAPQ)
    same = lambda: _table(gpu) == before
    # a second call on the same batch, also behind a download
    assert lib.dg_batch_accumulate_tx(gpu.ctx, 0, MIN_MAPQ, 0, None) == ERR_ARG and b"once" in err(gpu) and same()
    gpu.download()
    assert lib.dg_batch_accumulate_tx(gpu.ctx, 0, MIN_MAPQ, 0, None) == ERR_ARG and b"once" in err(gpu) and same()
    # odd n_pair_mode, one above the batch, a strand mode that is none (on a batch that is not counted yet)
    gpu.map_batch(*host.pack_reads(reads))
    assert lib.dg_batch_accumulate_tx(gpu.ctx, 3, MIN_MAPQ, 0, None) == ERR_ARG and b"n_pair_mode" in err(gpu) and same()
    assert lib.dg_batch_accumulate_tx(gpu.ctx, 502, MIN_MAPQ, 0, None) == ERR_ARG and b"n_pair_mode" in err(gpu) and same()
    assert lib.dg_batch_accumulate_tx(gpu.ctx, 0, MIN_MAPQ, 3, None) == ERR_ARG and b"strand_mode" in err(gpu) and same()
    # after dg_map_batch_compact: no full records
    words, nlist = host.pack_reads_2bit(reads)
    gpu.map_batch_compact(words, nlist, reads.shape[1])
    assert lib.dg_batch_accumulate_tx(gpu.ctx, 0, MIN_MAPQ, 0, None) == ERR_ARG and b"no full records" in err(gpu) and same()
    # merge into itself; short download buffers (nothing written); a flag that is not defined
    assert lib.dg_tx_merge(gpu.ctx, gpu.ctx) == ERR_ARG and same()
    off, ids, cnt, w8 = gpu.tx_classes()
    s_off = np.full(len(off), 0x55, np.uint64); s_ids = np.full(len(ids), 0x55, np.uint32); s_cnt = np.full(len(cnt), 0x55, np.uint64); s_w = np.full(8, 0x55, np.uint64)
    for capc, capm in ((len(cnt) - 1, len(ids)), (len(cnt), len(ids) - 1)):
        assert lib.dg_tx_classes_download(gpu.ctx, s_off.ctypes.data, s_ids.ctypes.data, s_cnt.ctypes.data, capc, capm, s_w.ctypes.data) == ERR_CAPACITY and b"needed" in err(gpu)
        assert (s_off == 0x55).all() and (s_ids == 0x55).all() and (s_cnt == 0x55).all() and (s_w == 0x55).all() and same()
    assert lib.dg_tx_finish(gpu.ctx, 1, 200, 10, None, None) == ERR_ARG and b"flag" in err(gpu) and same()
    ref = gpu.tx_finish(200, 32)
    short = np.full(len(ref) - 1, 0x55, np.uint64)
    assert lib.dg_tx_download(gpu.ctx, short.ctypes.data, len(short)) == ERR_CAPACITY and (short == 0x55).all()
    # dg_tx_add: a list that is not ascending, an id outside the annotation, an empty list; the downloaded table doubles it
    for mutate in ("swap", "range", "empty"):
        o2, i2 = off.copy(), ids.copy()
        k = int(np.argmax(np.diff(off.astype(np.int64)) >= 2))
        if mutate == "swap":
            a = int(off[k]); i2[a], i2[a + 1] = i2[a + 1], i2[a]
        elif mutate == "range":
            i2[len(i2) - 1] = len(tr)
        else:
            o2[1] = o2[0]
        assert lib.dg_tx_add(gpu.ctx, o2.ctypes.data, i2.ctypes.data, cnt.ctypes.data, len(cnt), w8.ctypes.data) == ERR_ARG and b"class " in err(gpu) and same(), mutate
    gpu.tx_add(off, ids, cnt, w8)
    assert _table(gpu) == txi.add_tables(before, before)
    gpu.tx_reset(); gpu.tx_add(off, ids, cnt, w8)
    assert same()
    # bad host records: the first bad read is named, nothing is counted
    r = res.reads.copy(); r["n_rep"][len(r) - 1] += 1; r["best"][7] = -1
    assert lib.dg_tx_count_records(gpu.ctx, len(r), 0, MIN_MAPQ, 0, r.ctypes.data, res.reports.ctypes.data, len(res.reports), res.cigar.ctypes.data, len(res.cigar), C.byref(n_units)) == ERR_ARG
    want_bad = 7 if res.reads["score"][7] > 0 else len(r) - 1
    assert (b"read %d " % want_bad) in err(gpu) and n_units.value == 0 and same()
    assert lib.dg_tx_count_records(gpu.ctx, len(r), 0, MIN_MAPQ, 0, res.reads.ctypes.data, res.reports.ctypes.data, len(res.reports), res.cigar.ctypes.data, len(res.cigar) - 1, None) == ERR_ARG and same()
    assert lib.dg_tx_count_records(gpu.ctx, 501, 502, MIN_MAPQ, 0, res.reads.ctypes.data, res.reports.ctypes.data, len(res.reports), res.cigar.ctypes.data, len(res.cigar), None) == ERR_ARG and same()
    # a bad annotation leaves the old one in place: the first bad transcript is named
    assert lib.dg_tx_set_annotation(gpu.ctx, C.byref(host.RnaAnnot(0, 0, 0, None, None)), None, None) == ERR_ARG
    btx, bex = txi.annot_arrays([(0, 0, [(5, 9)]), (0, 0, [(9, 9)])])
    assert lib.dg_tx_set_annotation(gpu.ctx, C.byref(host.RnaAnnot(2, 0, 2, btx.ctypes.data, bex.ctypes.data)), None, None) == ERR_ARG and b"transcript 1 " in err(gpu)
    cl1.tx_count_records(res.reads, res.reports, res.cigar, 0, MIN_MAPQ, 0)
    assert _table(cl1) == before
    # a new annotation over a table that holds classes: reset first; tables of different generations do not merge
    cl2.tx_count_records(res.reads[:10], res.reports, res.cigar, 0, MIN_MAPQ, 0)
    one = [(0, 0, [(10, 200000)])]
    gpu.tx_set_annotation(*txi.annot_arrays(one))
    gpu.map_batch(*host.pack_reads(reads))
    assert lib.dg_batch_accumulate_tx(gpu.ctx, 0, MIN_MAPQ, 0, None) == ERR_ARG and b"reset first" in err(gpu) and same()
    assert lib.dg_tx_count_records(gpu.ctx, len(res.reads), 0, MIN_MAPQ, 0, res.reads.ctypes.data, res.reports.ctypes.data, len(res.reports), res.cigar.ctypes.data, len(res.cigar), None) == ERR_ARG and same()
    cl2.tx_reset()
    cl2.tx_count_records(res.reads[:10], res.reports, res.cigar, 0, MIN_MAPQ, 0)
    assert lib.dg_tx_merge(cl2.ctx, cl1.ctx) == ERR_ARG and b"generation" in err(cl2) and _table(cl1) == before
    gpu.tx_reset()
    assert gpu.accumulate_tx(0, MIN_MAPQ, 0) == 500
    assert _table(gpu) == txi.twin(one, 1, res.reads, res.reports, res.cigar, 0, MIN_MAPQ)
    # the other stages are as usable as before
    n_genes, exons = gci.case_annotation(c, gci.CASE_SEEDS["se100"])
    gpu.gene_set_annotation(n_genes, exons); gpu.gene_reset()
    assert gpu.accumulate_genes(0, MIN_MAPQ) == 500
