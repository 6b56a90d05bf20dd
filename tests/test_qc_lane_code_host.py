"""CPU suite: the host-callable code of the device's QC tables (dart_amd/csrc/dg_qc.h) through tests/native/qc_checks.hip -- k_qc_flag's lane per record and
k_qc_cycle's group of lanes per record, lane by lane -- against the sequential Python twin of tests/qc_inputs.py, the twin against an independent restatement that expands
every record to per-base tuples, and the host formatter (the native program's and the library's dg_bam_qc_format) against the twin's text_of.  The tables are the
definition in the header's comment; no samtools is run."""
import random
import numpy as np
import pytest
import qc_inputs as qci
from qc_inputs import SN, M
from dart_amd import host

CASES = qci.crafted_cases()
BAD = qci.malformed_cases()
REF, NAMES = qci.REF, qci.NAMES


@pytest.fixture(scope="module")
def exe(workdir):
    return qci.build_program(workdir)


def _check(exe, workdir, tag, raw, flt, ref=REF, names=NAMES):
    words, text = qci.run_program(exe, workdir, tag, ref, raw, names, *flt)
    want = qci.twin(raw, ref, *flt)
    assert len(words) == len(want) and np.array_equal(words, want), [(int(k), int(words[k]), int(want[k])) for k in np.flatnonzero(words != want)[:10]]
    assert np.array_equal(qci.naive(raw, ref, *flt), want)
    assert text == qci.text_of(want, names, ref.chr_len)
    return qci.views(want, ref.n_chr)


@pytest.mark.parametrize("name", sorted(CASES))
def test_lane_code_equals_the_twin_and_the_twin_the_restatement_on_the_crafted_records(name, exe, workdir):
    raw = b"".join(CASES[name])
    for k, flt in enumerate(qci.FILTERS):
        _check(exe, workdir, "%s_%d" % (name, k), raw, flt)


@pytest.mark.parametrize("name", sorted(BAD))
def test_records_that_are_not_whole_count_as_malformed_and_for_nothing_else(name, exe, workdir):
    v = _check(exe, workdir, "bad_" + name, BAD[name], qci.FILTERS[2])
    assert v["SN"][SN["malformed"]] >= 1 and v["SN"][SN["records"]] == v["SN"][SN["malformed"]] + v["FS"][:, 0].sum()
    if name in ("liar", "cut_quals", "cut_bases", "cut_head"):
        assert v["SN"][SN["malformed"]] == 1 and v["SN"][SN["profiled"]] == v["FS"][0, 0] == (2 if name == "liar" else 1) and v["IS"].sum() == 0


def test_what_the_crafted_records_are_there_for(exe, workdir):
    run = lambda name, flt=qci.FILTERS[0]: _check(exe, workdir, name + "_again", b"".join(CASES[name]), flt)
    v = run("lengths")
    n = len(qci.LENGTHS)
    assert v["SN"][SN["profiled"]] == 2 * n and v["SN"][SN["left_out"]] == 0 and v["FS"][0, 0] == 2 * n + 2           # l_seq 0 with a CIGAR: whole, counted by the flags, not profiled
    assert v["RL"][:, 0].sum() == 2 and v["RL"][:, 511].sum() == 2 * 4 and v["SN"][SN["profiled_bases"]] == 2 * sum(qci.LENGTHS) == v["PC"][:, 0:5].sum()
    assert v["PC"][:, 0:5, 511].sum() == 2 * ((512 - 511) + (513 - 511) + (700 - 511))                               # the overflow row
    assert v["SN"][SN["clipped"]] == 3 * (n - 3) and v["SN"][SN["bases_without_quality"]] > n and v["PC"][:, 5].sum() == v["SN"][SN["quality_sum"]]
    v = run("ops")
    assert v["ID"][0, 63] == 1 and v["ID"][0, 64] == 3 and v["ID"][1, 63] == 1 and v["ID"][1, 64] == 3 and v["ID"][:, 0].sum() == 0
    assert v["ID"][0, 3] == 4 and v["PC"][0, 10, 0] == 1 and v["PC"][0, 10, 22] == 1 and v["PC"][1, 10, 2] == 1          # an I first: cycle 0 forward, the read's last cycle reversed; an I last, reversed and mate 2: cycle 2
    assert v["PC"][0, 11, 0] == 1 and v["PC"][0, 11, 9] == 1                                                         # a D in front of everything: stored base 0; reversed behind a clip of 2: base 1 of 12
    assert v["SN"][SN["n_ops"]] == 4 and v["SN"][SN["skipped_bases"]] == 2 * 300 + 2 * 70
    iupac = qci.twin(CASES["ops"][11], REF)
    assert qci.views(iupac, 2)["PC"][0, 4].sum() == 11 and qci.views(iupac, 2)["SN"][SN["mismatches"]] >= 11       # eleven IUPAC letters and N: other, and mismatches; '=' in M: the reference base, never one
    v = run("pairs")
    assert v["IS"][:, 1].sum() == 2 and v["IS"][:, 7999].sum() == 2 and v["IS"][:, 8000].sum() == 5 and v["SN"][SN["pairs"]] == 9 + 12
    assert v["IS"][0].sum() - 9 == 2 + 2 and v["IS"][1].sum() == 2 and v["IS"][2].sum() == 6                          # a != b: f < r and f == r inward, f > r outward; a == b other
    v = run("flags")
    assert v["CH"][2].tolist() == [0, 2] and v["CH"][1].tolist() == [1, 1] and v["CH"][0, 1] == 2      # (placed_unmapped_with_cigar, proper_but_unmapped)
    assert v["FS"][1, 0] == 2 and v["FS"][0, 2] == 3 and v["FS"][0, 3] == 1 and v["FS"][0, 4] == 3 and v["FS"][0, 5] == 2 and v["FS"][0, 13] == 1
    assert v["FS"][0, 14] == 5 and v["FS"][0, 15] == 3                                                               # mapq 0 and 4 stay out of row 15, 5 and 255 and 30 are in
    assert [int(v["MQ"][q]) for q in (0, 4, 5, 255)] == [2, 2, 2, 2]
    assert run("flags", qci.FILTERS[2])["SN"][SN["profiled"]] > v["SN"][SN["profiled"]]
    v = run("quals")
    assert v["SN"][SN["bases_without_quality"]] == 12 + 3 and v["SN"][SN["quality_sum"]] == 12 * 93 + (93 + 1 + 2 + 40 + 41 + 93 + 7)
    v = run("ends")
    assert v["SN"][SN["left_out"]] == 4 and v["SN"][SN["profiled"]] == 6
    v = run("empty")
    assert not any(v[k].any() for k in v)


def test_random_records_and_a_shuffled_copy(exe, workdir):
    ref = qci.pui.random_ref(3, [1700, 1601, 1602])
    names = [b"c0", b"chr_one", b"2"]
    rng = random.Random(23)
    recs = qci.random_records(rng, 2000, ref)
    for k, flt in enumerate(qci.FILTERS):
        v = _check(exe, workdir, "random_%d" % k, b"".join(recs), flt, ref, names)
        assert v["SN"][SN["profiled"]] > 500 and v["SN"][SN["left_out"]] > 5 and v["SN"][SN["mismatches"]] > 100 and v["PC"][:, 10].sum() > 50 and v["IS"].sum() > 20
    shuffled = list(recs); rng.shuffle(shuffled)
    assert shuffled != recs and np.array_equal(qci.twin(b"".join(shuffled), ref), qci.twin(b"".join(recs), ref))
    assert np.array_equal(qci.run_program(exe, workdir, "random_shuffled", ref, b"".join(shuffled), names)[0], qci.twin(b"".join(recs), ref))


def test_lane_code_under_the_sanitizers(workdir):
    """the same program with AddressSanitizer and UBSan on its host code: every field read, every CIGAR walk, every fetch of bases, qualities and reference bases
    stays inside the exact-size heap copies, every add inside the words.  Stand-alone; never through python's process, never on the GPU."""
    exe = qci.build_program(workdir, sanitize=True)
    for name in sorted(CASES):
        raw = b"".join(CASES[name])
        for k, flt in enumerate((qci.FILTERS[0], qci.FILTERS[2])):
            words, text = qci.run_program(exe, workdir, "san_%s_%d" % (name, k), REF, raw, NAMES, *flt)
            want = qci.twin(raw, REF, *flt)
            assert np.array_equal(words, want) and text == qci.text_of(want, NAMES, REF.chr_len)
    for name in sorted(BAD):
        assert np.array_equal(qci.run_program(exe, workdir, "san_bad_" + name, REF, BAD[name], NAMES, 4, 0)[0], qci.twin(BAD[name], REF, 4, 0))
    ref = qci.pui.random_ref(5, [1600, 1700, 1650])
    recs = qci.random_records(random.Random(5), 1000, ref)
    assert np.array_equal(qci.run_program(exe, workdir, "san_random", ref, b"".join(recs), [b"a", b"bb", b"ccc"])[0], qci.twin(b"".join(recs), ref))


# ---- the formatter ----
def _words(n_chr=2, **sections):
    lay = qci.layout(n_chr)
    w = np.zeros(lay["words"], np.uint64)
    v = qci.views(w, n_chr)
    for name, cells in sections.items():
        for idx, val in cells.items():
            v[name][idx] = val
    return w


FORMAT_CASES = {
    "all_zero": _words(),
    "no_aligned_base": _words(SN={7: 5, 6: 0, 5: 10, 13: 3, 14: 200}),                                  # error_ppm's denominator
    "no_quality": _words(SN={5: 10, 13: 10, 14: 0, 6: 10, 7: 1}),                                        # mean_quality_milli's
    "all_pairs_in_the_last_bin": _words(IS={(0, 8000): 3, (2, 8000): 4}, SN={15: 7}),                    # insert_mean_milli's; the median falls in bin 8000
    "median_in_bin_8000": _words(IS={(0, 100): 3, (1, 8000): 2, (2, 8000): 2}, SN={15: 7}),
    "median_just_below": _words(IS={(0, 100): 4, (1, 7999): 1, (2, 8000): 3}, SN={15: 8}),
    "one_pair": _words(IS={(1, 1): 1}, SN={15: 1}),
    "products_of_128_bits": _words(SN={6: (1 << 63) + 5, 7: (1 << 62) + 3, 5: (1 << 64) - 1, 13: 1, 14: (1 << 64) - 7, 15: (1 << 62)}, IS={(0, 7999): 1 << 61, (1, 7998): 1 << 61}),
    "pc_rows_with_gaps": _words(PC={(0, 3, 0): 1, (0, 11, 9): 2, (1, 5, 511): 1 << 40}, RL={(1, 511): 9, (0, 0): 1}, MQ={255: 1, 0: 2}, ID={(0, 64): 1, (1, 1): 2}, CH={(2, 1): 8, (0, 0): 1}, FS={(1, 15): 3, (0, 0): 4}),
}


@pytest.mark.parametrize("name", sorted(FORMAT_CASES))
def test_formatter_equals_text_of(name, exe, workdir):
    w = FORMAT_CASES[name]
    names, lengths = [b"chr1", b"a_longer_name"], [12345, (1 << 40) + 1]
    want = qci.text_of(w, names, lengths)
    assert qci.format_program(exe, workdir, name, w, names, lengths) == want
    lib = host._load_lib()
    assert host.qc_text(lib, w, names, lengths) == want
    d = dict(qci.derived(w, 2))
    if name == "all_zero":
        assert set(d.values()) == {0} and want.count(b"\n") == 20 + 16 + 3
    if name == "no_aligned_base": assert d["error_ppm"] == 0 and d["mean_quality_milli"] == 200 * 1000 // 7
    if name == "no_quality": assert d["mean_quality_milli"] == 0 and d["error_ppm"] == 100000
    if name == "all_pairs_in_the_last_bin": assert d["insert_mean_milli"] == 0 and d["insert_median"] == 8000
    if name == "median_in_bin_8000": assert d["insert_median"] == 8000 and d["insert_mean_milli"] == 100000
    if name == "median_just_below": assert d["insert_median"] == 100
    if name == "one_pair": assert d["insert_median"] == 1 and d["insert_mean_milli"] == 1000
    if name == "products_of_128_bits":
        assert d["error_ppm"] == ((1 << 62) + 3) * 10 ** 6 // ((1 << 63) + 5) and ((1 << 62) + 3) * 10 ** 6 >= 1 << 64 and d["insert_mean_milli"] == 7998500 and d["insert_median"] == 7998


def test_formatter_refusals():
    lib = host._load_lib()
    w = FORMAT_CASES["pc_rows_with_gaps"]
    text = host.qc_text(lib, w, [b"x", b"y"], [1, 2])
    import ctypes as C
    names = (C.c_char_p * 2)(b"x", b"y"); lens = np.array([1, 2], np.int64); nb = C.c_size_t(0)
    buf = np.zeros(len(text), np.uint8)
    assert lib.dg_bam_qc_format(w.ctypes.data, len(w), 2, names, lens.ctypes.data, buf.ctypes.data, len(text) - 1, C.byref(nb)) == -4 and nb.value == len(text) and not buf.any()
    assert lib.dg_bam_qc_format(w.ctypes.data, len(w) - 1, 2, names, lens.ctypes.data, buf.ctypes.data, len(text), C.byref(nb)) == -3
    assert lib.dg_bam_qc_format(w.ctypes.data, len(w), 3, names, lens.ctypes.data, buf.ctypes.data, len(text), C.byref(nb)) == -3
    assert lib.dg_bam_qc_format(w.ctypes.data, len(w), 2, names, lens.ctypes.data, buf.ctypes.data, len(text), C.byref(nb)) == 0 and buf.tobytes() == text
    off = (C.c_size_t * 9)()
    assert lib.dg_bam_qc_offsets(2, off) == 0 and [int(x) for x in off] == [qci.layout(2)[k][0] for k in ("FS", "CH", "MQ", "IS", "RL", "PC", "ID", "SN")] + [qci.layout(2)["words"]]
