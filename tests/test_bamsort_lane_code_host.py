"""CPU suite: the host-callable code of the device's coordinate sort (dart_amd/csrc/dg_bamsort.h) through tests/native/bamsort_checks.hip -- the key of a
record, the checked walk over records from outside, the walk over a byte range, the segment order and the final order -- against the Python twin of
tests/bamsort_inputs.py.  The order is the definition in the header's comment (what `samtools sort` does by default); no samtools is run."""
import pytest
import bamsort_inputs as bsi

N_CHR = 3


@pytest.fixture(scope="module")
def exe(workdir):
    return bsi.build_program(workdir)


def test_key_walk_and_final_order_of_the_crafted_records(exe, workdir):
    segments = bsi.crafted_segments(N_CHR)
    segs, recs, order, bits, data = bsi.run_program(exe, workdir, "crafted", N_CHR, segments)
    assert bits == bsi.key_bits(N_CHR) == 35
    for (ordinal, raw), s, r in zip(segments, segs, recs):
        why, bad, offs = bsi.walk_checked(raw, N_CHR)
        assert why == bsi.OK and s == dict(why=bsi.OK, bad=0, n=len(offs), range=len(offs))
    # every key and store offset, segment by segment (the store holds the segments in call order)
    base = 0
    for (ordinal, raw), r in zip(segments, recs):
        _, _, offs = bsi.walk_checked(raw, N_CHR)
        assert r == [(bsi.key(raw, N_CHR, o), base + o) for o in offs]
        base += len(raw)
    # ascending ordinal, equal ordinals in call order
    assert order == [3, 1, 4, 0, 2]
    want = bsi.expected_sorted(segments, N_CHR)
    assert data == b"".join(want)
    # what the set is there for
    names = [w[36:36 + w[12] - 1] for w in want]
    at = {n: i for i, n in enumerate(names)}
    assert names[0] == b"pos_m1"                                                       # pos -1 on chromosome 0 sorts first
    assert at[b"pos0"] < at[b"pos0_again"] < at[b"pos0_rev"]                           # forward before reverse at one position; equal keys keep their order
    assert at[b"far_fwd"] < at[b"far_rev"] and bsi.key(segments[0][1], N_CHR) == (N_CHR - 1) << 33 | (2 ** 31 - 1) << 1 | 1
    assert [n for n in names if n.startswith(b"tie_")] == [b"tie_d0", b"tie_b0", b"tie_b1", b"tie_b2", b"tie_c0"]      # ordinals 1, 3, 3, 3, 9
    unplaced = [n for n in names if bsi.key(want[at[n]], N_CHR) >> 33 == N_CHR]
    assert names[-len(unplaced):] == unplaced and unplaced == [b"unplaced", b"unplaced_c", b"negative_refid_is_unplaced", b"unplaced_with_pos"]
    assert {len(n) for n in names} >= {1, 254}
    assert max(len(w) for w in want) > 1500 and any(w[16:18] == (300).to_bytes(2, "little") for w in want)


@pytest.mark.parametrize("case", sorted(bsi.malformed_cases(N_CHR)))
def test_malformed_records_are_refused_with_their_index(case, exe, workdir):
    data, why, bad = bsi.malformed_cases(N_CHR)[case]
    assert bsi.walk_checked(data, N_CHR)[:2] == (why, bad)
    good = bsi.record(1, 10, 0, b"kept")
    segs, recs, order, bits, out = bsi.run_program(exe, workdir, "bad_" + case, N_CHR, [(0, good), (1, data), (2, good)])
    assert segs[1]["why"] == why and segs[1]["bad"] == bad
    assert segs[0]["why"] == segs[2]["why"] == bsi.OK
    assert order == [0, 2] and out == good + good            # nothing of the refused segment was added


def test_empty_input_and_single_record(exe, workdir):
    segs, recs, order, bits, out = bsi.run_program(exe, workdir, "empty", N_CHR, [])
    assert segs == [] and order == [] and out == b""
    one = bsi.record(2, 5, 16, b"only")
    segs, recs, order, bits, out = bsi.run_program(exe, workdir, "one", N_CHR, [(4, b""), (4, one)])
    assert [s["n"] for s in segs] == [0, 1] and out == one and recs[1] == [(2 << 33 | 6 << 1 | 1, 0)]


def test_key_bits_grow_with_the_chromosome_count(exe, workdir):
    for n_chr, bits in ((1, 34), (2, 35), (3, 35), (4, 36), (25, 38), (194, 41)):
        _, _, _, got, _ = bsi.run_program(exe, workdir, "bits%d" % n_chr, n_chr, [(0, bsi.record(n_chr - 1, 0, 0) + bsi.record(-1, 0, 0))])
        assert got == bits == bsi.key_bits(n_chr)


def test_lane_code_under_the_sanitizers(workdir):
    """the same program with AddressSanitizer and UBSan on its host code: every walk stays inside the segment's exact-size heap copy"""
    exe = bsi.build_program(workdir, sanitize=True)
    segments = bsi.crafted_segments(N_CHR) + [(5, d) for d, _, _ in bsi.malformed_cases(N_CHR).values()]
    segs, recs, order, bits, data = bsi.run_program(exe, workdir, "san", N_CHR, segments)
    assert data == b"".join(bsi.expected_sorted(bsi.crafted_segments(N_CHR), N_CHR))
