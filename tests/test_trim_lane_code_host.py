"""CPU suite: the rules of the device's trimming stage (dart_amd/csrc/dg_trim.h: the packed planes and their unaligned extracts, the walks in rounds of 64 with
a carry, the adapter at every start position, the mate's verdict, the stored window) compiled for the host (tests/native/trim_checks.hip) against the sequential
twin of the definition (tests/trim_inputs.py) on the crafted reads; once more as a build with the address and undefined-behaviour sanitizers."""
import os
import pytest
import trim_inputs as ti


def _compare(exe, path, t1, t2, rc_odd, p):
    st, wins, stats, kept = ti.run_checks_program(exe, path, t1, t2, rc_odd, p)
    assert st == 0
    two = t2 is not None
    want_kept, want_stats, want_wins, idx, plain = ti.trim_batch(ti.records(t1, t2), p, two, rc_odd)
    pairs = bool(p["flags"] & ti.PAIRS)
    assert len(wins) == len(want_wins)
    for k, (g, (a, b, w)) in enumerate(zip(wins, want_wins)):
        ad = (k & 1) if (two or pairs) else 0
        assert g == ti.window_row(a, b, w, ad, k in set(idx)), (k, g, (a, b, w))
    assert stats == want_stats
    assert kept == want_kept
    return want_stats, want_wins, idx


def test_lane_code_trims_the_crafted_reads_as_the_twin(workdir):
    exe = ti.build_checks_program(workdir)
    reads = ti.crafted_cases()
    st, wins, idx = _compare(exe, os.path.join(workdir, "trim_crafted.bin"), ti.text_of(reads), None, False, ti.CRAFT)
    assert st[6] > 15 and st[7] == 0 and st[9] >= 5 and st[11] > 0 and st[12] == 0 and st[13] == 1 and 0 < st[1] < st[0]
    # every step alone, and none
    for p in (ti.params(qual3=20), ti.params(qual5=20), ti.params(adapter=(ti.ADAPTER[:13], b"")), ti.params(poly_mask=15, poly_min=1), ti.params(),
              ti.params(adapter=(ti.ADAPTER, b""), min_overlap=1, max_err_permille=1000), ti.params(adapter=(ti.ADAPTER, b""), min_overlap=64, max_err_permille=0),
              ti.params(qual3=255, qual5=255, qual_base=0), ti.params(adapter=(b"A", b""), min_overlap=2000)):
        _compare(exe, os.path.join(workdir, "trim_crafted.bin"), ti.text_of(reads), None, False, p)


@pytest.mark.parametrize("layout", ["two_texts", "interleaved", "interleaved_odd_last"])
def test_lane_code_pairs_are_kept_or_dropped_together(layout, workdir):
    exe = ti.build_checks_program(workdir)
    t1, t2, inter, inter_odd = ti.pair_texts()
    a, b = (t1, t2) if layout == "two_texts" else (inter, None) if layout == "interleaved" else (inter_odd, None)
    p = dict(ti.CRAFT, flags=ti.PAIRS)
    st, wins, idx = _compare(exe, os.path.join(workdir, "trim_pairs_%s.bin" % layout), a, b, True, p)
    kept = set(idx)
    assert 8 not in kept and 9 not in kept and wins[8][1] - wins[8][0] >= p["min_len"] and wins[9][1] - wins[9][0] < p["min_len"]       # only mate 2 fails
    assert 12 not in kept and 13 not in kept and wins[13][1] - wins[13][0] >= p["min_len"]                                              # only mate 1 fails
    assert st[12] >= 2 and st[7] > 0 and st[6] > 0
    if layout != "interleaved":
        assert st[0] % 2 == 1 and st[0] - 1 in kept                      # the unpaired last read stands alone
    # without the flag every read stands alone (and one text's reads all take adapter 0)
    st2, wins2, idx2 = _compare(exe, os.path.join(workdir, "trim_pairs_%s.bin" % layout), a, b, True, ti.CRAFT)
    assert 8 in set(idx2) and 9 not in set(idx2) and st2[12] == 0


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_lane_code_drops_on_both_sides_of_the_length_kernels_seam(n, workdir):
    exe = ti.build_checks_program(workdir)
    drop = {0, 100, 254, 255, 256, n - 1} & set(range(n))
    reads = ti.many_reads(n, seed=n, drop_at=drop)
    st, wins, idx = _compare(exe, os.path.join(workdir, "trim_many.bin"), ti.text_of(reads), None, False, ti.CRAFT)
    assert st[0] == n and st[1] == n - len(drop) and st[6] > n // 4
    # a batch that is dropped whole
    st, wins, idx = _compare(exe, os.path.join(workdir, "trim_many.bin"), ti.text_of(reads), None, False, dict(ti.CRAFT, min_len=500))
    assert st[0] == n and st[1] == 0 and idx == []


def test_lane_code_under_the_sanitizers(workdir):
    """the same program built with the address and undefined-behaviour sanitizers on the host code: the unaligned extracts at a read's last word stay inside
    the packed planes, shifts stay inside their types"""
    exe = ti.build_checks_program(workdir, sanitize=True)
    reads = ti.crafted_cases()
    for p in (ti.CRAFT, ti.params(adapter=(ti.ADAPTER, b""), min_overlap=1, max_err_permille=1000), ti.params(adapter=(ti.ADAPTER[:33], b""), min_overlap=1, max_err_permille=0)):
        _compare(exe, os.path.join(workdir, "trim_asan.bin"), ti.text_of(reads), None, False, p)
    t1, t2, inter, inter_odd = ti.pair_texts()
    _compare(exe, os.path.join(workdir, "trim_asan.bin"), t1, t2, True, dict(ti.CRAFT, flags=ti.PAIRS))
