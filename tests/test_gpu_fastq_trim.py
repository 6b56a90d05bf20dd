"""GPU suite (-m gpu): adapters, poly tails and low-quality ends cut inside the FASTQ upload (dg_set_trim, dart_amd/csrc/dg_trim.h) against the sequential twin
of the definition (tests/trim_inputs.py): nothing changes when nothing is set, the crafted reads on the kernels' seams, mapping parity with a plain upload of
the text the twin wrote after trimming, split invariance, the BGZF upload, the error contract.  Every comparison is exact."""
import numpy as np
import pytest
import common
import fastq_device_inputs as fdi
import gz_device_inputs as gz
import trim_inputs as ti
from dart_amd import host

pytestmark = pytest.mark.gpu
CASES = ["pe101_spliced", "se100"]


@pytest.fixture(scope="module")
def ctxs(workdir):
    out = {}
    for name in CASES:
        c = common.build_case(name, workdir)
        ix = host.Index(c["prefix"])
        out[name] = (c, host.DartGPU(ix))
    yield out
    for v in out.values():
        v[1].close()


@pytest.fixture()
def gpu(ctxs):
    g = ctxs["pe101_spliced"][1]
    g.set_trim(off=True)
    yield g
    g.set_trim(off=True)


def _batch(g):
    so, rl, flat, names, quals = g.download_reads()
    raw = flat.tobytes()
    assert all(int(so[k + 1]) == int(so[k]) + int(rl[k]) for k in range(len(rl) - 1))          # the kept reads lie one behind the other
    return [(names[k], raw[int(so[k]):int(so[k]) + int(rl[k])], quals[k]) for k in range(len(rl))]


def _same_reads(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)


def _set(g, p):
    g.set_trim(adapter=p["adapter"][0], adapter2=p["adapter"][1], qual3=p["qual3"], qual5=p["qual5"], qual_base=p["qual_base"], min_overlap=p["min_overlap"],
               max_err_permille=p["max_err_permille"], poly_mask=p["poly_mask"], poly_min=p["poly_min"], min_len=p["min_len"], flags=p["flags"])


def _against_the_twin(g, t1, t2, rc_odd, p):
    _set(g, p)
    want, stats, wins, idx, plain = ti.trim_batch(ti.records(t1, t2), p, t2 is not None, rc_odd)
    assert g.upload_fastq(t1, t2, rc_odd_reads=rc_odd) == len(want)
    _same_reads(_batch(g), want)
    assert g.trim_stats() == stats
    assert g.trim_device_ms > 0 and g.fastq_device_ms >= g.trim_device_ms
    return stats, idx


@pytest.mark.parametrize("layout", ["two_files_paired", "interleaved_paired", "one_file_single", "two_files_single"])
def test_nothing_set_and_every_step_off_leave_the_plain_upload(layout, gpu):
    t1, t2, inter = fdi.awkward_texts(fdi.random_reads(23, seed=5), fdi.random_reads(23, seed=6))
    a, b = (inter, None) if layout == "interleaved_paired" else (t1, None) if layout == "one_file_single" else (t1, t2)
    paired = layout.endswith("paired")
    want = fdi.reference_reads(a, b, paired)
    assert gpu.upload_fastq(a, b, rc_odd_reads=paired) == len(want)
    plain = _batch(gpu)
    _same_reads(plain, want)
    assert gpu.trim_stats() == [0] * 16
    gpu.set_trim(min_len=1, pairs=paired)
    assert gpu.upload_fastq(a, b, rc_odd_reads=paired) == len(want)
    _same_reads(_batch(gpu), plain)
    st = gpu.trim_stats()
    assert st[0] == st[1] == len(want) and st[2] == st[3] == sum(len(s) for h, s, q in want) and st[4:] == [0] * 12
    gpu.set_trim(off=True)
    assert gpu.upload_fastq(a, b, rc_odd_reads=paired) == len(want)
    _same_reads(_batch(gpu), plain)
    assert gpu.trim_stats() == [0] * 16
    # not inherited by a clone
    gpu.set_trim(adapter=b"ACGT", min_overlap=1, min_len=1000)
    clone = gpu.clone()
    assert clone.upload_fastq(a, b, rc_odd_reads=paired) == len(want)
    _same_reads(_batch(clone), plain)
    clone.close()


def test_crafted_reads_equal_the_twin(gpu):
    assert gpu.trim_granules() == (256, 64)
    reads = ti.crafted_cases()
    text = ti.text_of(reads)
    st, idx = _against_the_twin(gpu, text, None, False, ti.CRAFT)
    assert st[6] > 15 and st[9] >= 5 and st[11] > 0 and st[13] == 1 and 0 < st[1] < st[0]
    for p in (ti.params(qual3=20), ti.params(qual5=20), ti.params(adapter=(ti.ADAPTER[:13], b"")), ti.params(poly_mask=15, poly_min=1),
              ti.params(adapter=(ti.ADAPTER, b""), min_overlap=1, max_err_permille=1000), ti.params(adapter=(ti.ADAPTER, b""), min_overlap=64, max_err_permille=0),
              ti.params(qual3=255, qual5=255, qual_base=0), ti.params(adapter=(b"A", b""), min_overlap=2000)):
        _against_the_twin(gpu, text, None, False, p)


@pytest.mark.parametrize("layout", ["two_texts", "interleaved", "interleaved_odd_last"])
def test_pairs_are_kept_or_dropped_together(layout, gpu):
    t1, t2, inter, inter_odd = ti.pair_texts()
    a, b = (t1, t2) if layout == "two_texts" else (inter, None) if layout == "interleaved" else (inter_odd, None)
    p = dict(ti.CRAFT, flags=ti.PAIRS)
    st, idx = _against_the_twin(gpu, a, b, True, p)
    kept = set(idx)
    assert not {8, 9, 12, 13} & kept and st[12] >= 2 and st[6] > 0 and st[7] > 0        # in pair 4 only mate 2 fails, in pair 6 only mate 1
    if layout != "interleaved":
        assert st[0] % 2 == 1 and st[0] - 1 in kept                                     # the unpaired last read stands alone
    assert any(k & 1 for k in kept)                                                     # mates 2 are stored reverse-complemented (the twin's kept reads say how)
    st2, idx2 = _against_the_twin(gpu, a, b, True, ti.CRAFT)
    assert 8 in set(idx2) and 9 not in set(idx2) and st2[12] == 0


@pytest.mark.parametrize("n", [255, 256, 257])
def test_drops_on_both_sides_of_the_length_kernels_seam_and_a_batch_dropped_whole(n, gpu):
    drop = {0, 100, 254, 255, 256, n - 1} & set(range(n))
    text = ti.text_of(ti.many_reads(n, seed=n, drop_at=drop))
    st, idx = _against_the_twin(gpu, text, None, False, ti.CRAFT)
    assert st[0] == n and st[1] == n - len(drop) and st[6] > n // 4
    st, idx = _against_the_twin(gpu, text, None, False, dict(ti.CRAFT, min_len=500))
    assert st[0] == n and st[1] == 0
    assert gpu.run() == [0, 0, 0]                                  # a batch of which nothing is left is a batch of 0 reads
    assert gpu.format_sam_resident(0)[0] == b""


# ---- mapping parity ---------------------------------------------------------------------------------------------------------------------------------
PARITY = ti.params(qual3=20, min_overlap=3, max_err_permille=100, poly_mask=ti.poly_mask("G"), poly_min=10, min_len=20, adapter=(ti.ADAPTERS["illumina"], ti.ADAPTERS["illumina"]))


@pytest.fixture(scope="module")
def spoiled(ctxs):
    """per case: the FASTQ texts with adapter read-through, low-quality tails and poly-G tails laid over the golden reads, and what the twin makes of them"""
    out = {}
    for name in CASES:
        c, g = ctxs[name]
        paired = bool(c["spec"]["paired"])
        def text(m, seed, tag):
            return b"".join(b"@r%d/%d\n%s\n+\n%s\n" % (i, tag, s, q) for i, (s, q) in enumerate(ti.spoil(m, seed, ti.ADAPTERS["illumina"] + b"ACACGTCTGAACTCCAGTCAC")))
        t1 = text(c["m1"], 31, 1); t2 = text(c["m2"], 32, 2) if paired else None
        p = dict(PARITY, flags=ti.PAIRS if paired else 0)
        kept, stats, wins, idx, plain = ti.trim_batch(ti.records(t1, t2), p, paired, paired)
        out[name] = dict(t1=t1, t2=t2, p=p, kept=kept, stats=stats, plain=ti.fastq_of(plain, paired), paired=paired)
    return out


def _map(g, c, t1, t2, paired, run):
    p, h = common.parse_flags(run["flags"])
    g.set_params(host.default_params(paired=int(paired), **p))
    n = g.upload_fastq(t1, t2, rc_odd_reads=paired)
    reads = _batch(g)
    g.run()
    res = g.download()
    text, ct = g.format_sam_resident(n if paired else 0, unique_only=h["unique"])
    return n, reads, res, text, ct


@pytest.mark.parametrize("name", CASES)
def test_mapping_a_trimmed_upload_equals_mapping_the_text_the_twin_trimmed(name, ctxs, spoiled):
    c, g = ctxs[name]
    s = spoiled[name]
    st = s["stats"]
    # every rule fired, and reads were dropped (pairs: together)
    assert st[5] > 0 and st[6] > 0 and (st[7] > 0) == s["paired"] and st[8] > 0 and st[9] > 0 and st[11] > 0 and (st[12] > 0) == s["paired"] and st[1] < st[0] and st[1] > st[0] // 2
    run = c["runs"][0]
    g.set_trim(off=True)
    n_w, reads_w, res_w, text_w, ct_w = _map(g, c, s["plain"][0], s["plain"][1], s["paired"], run)
    assert n_w == st[1]
    _set(g, s["p"])
    n, reads, res, text, ct = _map(g, c, s["t1"], s["t2"], s["paired"], run)
    assert n == st[1] and g.trim_stats() == st
    g.set_trim(off=True)
    _same_reads(reads, s["kept"]); _same_reads(reads, reads_w)
    common.assert_same(res, (res_w.reads, res_w.reports, res_w.cigar, res_w.sj))
    assert text == text_w, common.first_diff(text.decode("latin1"), text_w.decode("latin1"))
    assert ct == ct_w and len(text) > 0 and ct["unmapped"] < n


def _cut_at(t, rec):
    pos = 0
    for _ in range(4 * rec):
        pos = t.index(b"\n", pos) + 1
    return pos


def test_split_invariance(ctxs, spoiled):
    c, g = ctxs["pe101_spliced"]
    s = spoiled["pe101_spliced"]
    run = c["runs"][0]
    _set(g, s["p"])
    def part(a, b):
        n, reads, res, text, ct = _map(g, c, a, b, True, run)
        return reads, text, ct, g.trim_stats()
    whole_reads, whole, ctw, stw = part(s["t1"], s["t2"])
    rec = c["spec"]["npairs"] // 2
    c1, c2 = _cut_at(s["t1"], rec), _cut_at(s["t2"], rec)
    ra, a, cta, sta = part(s["t1"][:c1], s["t2"][:c2]); rb, b, ctb, stb = part(s["t1"][c1:], s["t2"][c2:])
    g.set_trim(off=True)
    assert ra + rb == whole_reads and a + b == whole and {k: cta[k] + ctb[k] for k in cta} == ctw
    assert [x + y for x, y in zip(sta, stb)] == stw == s["stats"]


def test_bgzf_upload_trims_the_same(ctxs, spoiled):
    c, g = ctxs["pe101_spliced"]
    s = spoiled["pe101_spliced"]
    t1, t2 = s["t1"][:_cut_at(s["t1"], 300)], s["t2"][:_cut_at(s["t2"], 300)]
    _set(g, s["p"])
    n_want = g.upload_fastq(t1, t2, rc_odd_reads=True)
    want, st_want = _batch(g), g.trim_stats()
    assert 0 < n_want < 600
    # whole, with `last`
    n, tail1, tail2, unlike = g.upload_fastq_bgzf(t1[:50], gz.bgzf(t1[50:], block=3000), b"", gz.bgzf(t2, block=4100), rc_odd_reads=True, last=True)
    assert n == n_want and tail1 == b"" and tail2 == b"" and unlike == 0 and g.trim_stats() == st_want
    _same_reads(_batch(g), want)
    # in two pieces that do not end where records end: whole records only, the tails are the untrimmed text's
    k1, k2 = len(t1) // 2 + 13, len(t2) // 2 - 7
    n_a, tail1, tail2, unlike = g.upload_fastq_bgzf(b"", gz.bgzf(t1[:k1], block=2500), b"", gz.bgzf(t2[:k2], block=2500), rc_odd_reads=True)
    taken = min(gz.whole_records(t1[:k1])[0], gz.whole_records(t2[:k2])[0])
    assert tail1 == t1[gz.cut_records(t1, taken):k1] and tail2 == t2[gz.cut_records(t2, taken):k2] and unlike == 0
    reads_a, st_a = _batch(g), g.trim_stats()
    assert st_a[0] == 2 * taken and st_a[1] == n_a
    n_b, tail1, tail2, unlike = g.upload_fastq_bgzf(tail1, gz.bgzf(t1[k1:], block=2500), tail2, gz.bgzf(t2[k2:], block=2500), rc_odd_reads=True, last=True)
    assert tail1 == b"" and tail2 == b"" and n_a + n_b == n_want
    _same_reads(reads_a + _batch(g), want)
    assert [x + y for x, y in zip(st_a, g.trim_stats())] == st_want
    # DG_FQ_CHECK_ONLY: the kept count, no batch
    n, tail1, tail2, unlike = g.upload_fastq_bgzf(b"", gz.bgzf(t1), b"", gz.bgzf(t2), rc_odd_reads=True, last=True, check_only=True)
    assert n == n_want and g.trim_stats() == st_want
    with pytest.raises(RuntimeError):
        g.run()
    g.set_trim(off=True)


def test_error_contract(ctxs, spoiled):
    c, g = ctxs["pe101_spliced"]
    s = spoiled["pe101_spliced"]
    t1, t2 = s["t1"][:_cut_at(s["t1"], 100)], s["t2"][:_cut_at(s["t2"], 100)]
    _set(g, s["p"])
    n_good = g.upload_fastq(t1, t2, rc_odd_reads=True)
    good, st_good = _batch(g), g.trim_stats()
    assert 0 < n_good < 200
    def still_good():
        assert g.upload_fastq(t1, t2, rc_odd_reads=True) == n_good
        _same_reads(_batch(g), good)
        assert g.trim_stats() == st_good
    for kw, word in ((dict(flags=2), "flag"), (dict(flags=0x80000001), "flag"), (dict(adapter=b"A" * 65), "64"), (dict(adapter=b"ACGN"), "ACGT"), (dict(adapter=b"acgt"), "ACGT"),
                     (dict(adapter=b"ACGT", adapter2=b"AC T"), "ACGT"), (dict(min_len=0), "min_len"), (dict(min_overlap=0), "min_overlap"), (dict(max_err_permille=1001), "1000"),
                     (dict(poly_mask=16), "poly_mask"), (dict(qual3=256), "qual"), (dict(qual_base=1000), "qual")):
        with pytest.raises(RuntimeError, match=word):
            g.set_trim(**kw)
        still_good()                                                # the context is usable and its setting is the one it had
    # the plain upload's errors keep their meaning on the untrimmed record
    r = lambda i, seq=b"ACGTACGTACGTACGTACGTACGTACGT": b"@e%d\n" % i + seq + b"\n+\n" + b"I" * len(seq) + b"\n"
    with pytest.raises(RuntimeError, match="read 3 is a record without bases"):
        g.upload_fastq(r(0) + r(1) + r(2) + b"@empty\n\n+\n\n" + r(4) + r(5))
    still_good()
    with pytest.raises(RuntimeError, match="read 1 is longer than DG_MAX_RLEN"):
        g.upload_fastq(r(0) + r(1, b"A" * 1001) + r(2) + r(3))
    still_good()
    with pytest.raises(RuntimeError, match="records"):
        g.upload_fastq(r(0) + r(1) + r(2) + r(3), r(4), rc_odd_reads=True)
    still_good()
    with pytest.raises(RuntimeError, match="max_reads"):                 # max_reads counts the input: 200 reads do not fit 199 although fewer are kept
        g.upload_fastq(t1, t2, rc_odd_reads=True, max_reads=199)
    assert g.fastq_need == 200
    still_good()
    assert g.upload_fastq(t1, t2, rc_odd_reads=True, max_reads=200) == n_good
    assert g.upload_fastq(b"") == 0 and g.trim_stats() == [0] * 16      # no text: no reads
    g.set_trim(off=True)
