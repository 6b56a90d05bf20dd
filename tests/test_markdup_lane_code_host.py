"""CPU suite: the host-callable code of the device's duplicate marking (dart_amd/csrc/dg_markdup.h) through tests/native/markdup_checks.hip -- a record's
filter, end key, score and hash, the mate search over the hash-sorted candidates, the sorted pairs and ends, the byte written -- against the sequential Python
twin of tests/markdup_inputs.py, and the twin against a brute-force verdict.  The marking is the definition in the header's comment (modelled on Picard's rules);
no samtools or Picard is run."""
import random
import pytest
import bamsort_inputs as bsi
import markdup_inputs as mdi

CASES = mdi.crafted_cases()
DUP = mdi.DUP


@pytest.fixture(scope="module")
def exe(workdir):
    return mdi.build_program(workdir)


def _check(exe, workdir, tag, n_chr, recs, hash_bits):
    """program == twin == brute force -> (marked bytes, stats, {name: flag & 0x400 != 0} of the examined records, the program's result)"""
    raw = b"".join(recs)
    got = mdi.run_program(exe, workdir, tag, n_chr, raw, hash_bits)
    marked, stats, verdict = mdi.twin(raw, n_chr, hash_bits)
    assert got["bad"] is None
    offs = mdi.offsets(raw)
    for i, at in enumerate(offs):
        r = mdi.examine(raw, at, n_chr, i)
        if r is None:
            assert got["recs"][i][:2] == (0, 0) and i not in got["dup"]
        else:
            assert got["recs"][i] == (1, int(r["cand"]), r["E"], r["score"], mdi.name_hash(r["name"], hash_bits) if r["cand"] else 0)
    assert got["dup"] == verdict
    assert got["marked"] == marked and got["stats"] == stats
    assert verdict == mdi.brute(raw, n_chr, hash_bits)
    assert stats[6] == 2 * stats[3] + stats[4] == sum(verdict.values()) and stats[0] == 2 * stats[1] + stats[2] == len(verdict)
    # nothing but bit 0x400 of examined records differs from the input; the call is idempotent
    assert len(marked) == len(raw)
    diff = [k for k in range(len(raw)) if raw[k] != marked[k]]
    assert all(k - 19 in offs and offs.index(k - 19) in verdict and raw[k] ^ marked[k] == 4 for k in diff)
    assert mdi.twin(marked, n_chr, hash_bits)[:2] == (marked, stats)
    names = {}
    for i, dup in verdict.items():
        names.setdefault(recs[i][36:36 + recs[i][12] - 1], []).append(dup)
    return marked, stats, names, got


@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "range"))
def test_lane_code_equals_the_twin_equals_brute_force_on_the_crafted_records(name, exe, workdir):
    n_chr, recs, hash_bits, _ = CASES[name]
    _check(exe, workdir, name, n_chr, recs, hash_bits)


def test_what_the_crafted_records_are_there_for(exe, workdir):
    run = lambda name: _check(exe, workdir, name + "_again", *CASES[name][:3])
    # CIGARs and end keys: all nine ops, clips on either side, shared unclipped ends, a negative one
    _, st, dup, got = run("cigar")
    assert st == (12, 0, 12, 0, 6, 0, 6, 0)
    E = {CASES["cigar"][1][i][36:36 + CASES["cigar"][1][i][12] - 1]: got["recs"][i][2] for i in range(12)}
    key = lambda tid, u5, s: tid << 34 | (u5 + (1 << 31)) << 1 | s
    assert E[b"all_ops_fwd"] == E[b"same_u5_no_clip"] == key(0, 995, 0) and E[b"all_ops_rev"] == E[b"same_end_no_clip"] == key(0, 1724, 1)
    assert E[b"h_then_s"] == E[b"plain_1993"] == key(0, 1993, 0) and E[b"rev_trailing_clip"] == E[b"rev_plain_2054"] == key(0, 2054, 1)
    assert E[b"u5_negative"] == E[b"u5_negative_too"] == key(0, -8, 0) and E[b"clip_in_the_middle_of_clips"] == E[b"plain_2998"] == key(0, 2998, 0)
    assert dup[b"same_u5_no_clip"] == [True] and dup[b"all_ops_rev"] == [True] and dup[b"plain_1993"] == [True] and dup[b"rev_trailing_clip"] == [True]
    assert dup[b"u5_negative"] == [True] and dup[b"plain_2998"] == [True]
    _, st, dup, got = run("edge")
    assert st[:5] == (2, 0, 2, 0, 0) and sorted(r[2] for r in got["recs"]) == [key(0, -(1 << 31), 0), key(1, 3 * (1 << 31) - 1, 1)]
    # scores: 14, 94 and 0xff count nothing; saturation, then the index decides
    _, st, dup, got = run("quals")
    by = {CASES["quals"][1][i][36:36 + CASES["quals"][1][i][12] - 1]: got["recs"][i][3] for i in range(8)}
    assert by == {b"q14": 0, b"q15": 60, b"q93": 372, b"q94": 0, b"q255": 0, b"saturated_a": mdi.SCORE_MAX, b"saturated_b": mdi.SCORE_MAX, b"just_below": mdi.SCORE_MAX - 1}
    assert sorted(n for n, d in dup.items() if d == [False]) == [b"q93", b"saturated_a"]
    # ties: the smallest index survives; a better score beats it
    _, st, dup, _ = run("ties")
    assert dup[b"tie_a"] == [False] and dup[b"tie_b"] == dup[b"tie_c"] == [True]
    assert dup[b"ptie_a"] == [False, False] and dup[b"ptie_b"] == dup[b"ptie_c"] == [True, True] and dup[b"pbest"] == [False, False] and dup[b"pworse"] == [True, True]
    assert st[7] == 3
    # signatures
    _, st, dup, _ = run("signatures")
    assert dup[b"lo_is_hi_a"] == [True, True] and dup[b"lo_is_hi_b"] == [False, False]
    assert dup[b"fr"] == [True, True] and dup[b"fr_again"] == [True, True] and dup[b"mate2_first"] == [False, False] and dup[b"rf"] == [False, False]
    assert dup[b"two_chr_a"] == [True, True] and dup[b"two_chr_b"] == [False, False] and dup[b"two_chr_other"] == [False, False]
    # fragments and the records that play no part
    marked, st, dup, _ = run("fragments")
    assert dup[b"the_pair"] == [False, False] and dup[b"on_the_pairs_lo"] == dup[b"on_the_pairs_hi"] == [True] and dup[b"other_strand"] == [False]
    assert dup[b"mate_unmapped"] == [True] and dup[b"mate_unmapped_too"] == [False] and dup[b"unpaired"] == [True] and dup[b"unpaired_better"] == [False]
    assert dup[b"partner_not_in_store"] == [False] and dup[b"partner_not_in_store_too"] == [True]
    assert dup[b"both_first"] == [True, False]                   # two fragments: the one at 700 loses to first_and_last's score, the one at 800 is alone
    assert dup[b"first_and_last"] == [False] and dup[b"qc_fail_is_examined"] == [False]
    for nm in (b"secondary", b"supplementary", b"unplaced", b"unplaced_with_cigar", b"pos_m1", b"no_cigar", b"placed_unmapped"):
        assert nm not in dup
    assert mdi.flags_by_name(marked) >= {(b"the_pair", 0x141 | DUP), (b"supplementary", 0x800 | DUP), (b"unplaced", 0x4D | DUP), (b"secondary", 0x100)}
    # the input's bit
    marked, st, dup, _ = run("input_flag")
    assert mdi.flags_by_name(marked) == {(b"survivor_marked_on_input", 0), (b"loser", DUP), (b"loser_marked_on_input", DUP), (b"pair_marked_on_input", 0x61), (b"pair_marked_on_input", 0x91),
                                         (b"secondary_stays_marked", 0x100 | DUP)}
    # malformed records play no part, wherever they lie
    for nm in ("malformed", "malformed_last", "malformed_last_cigar"):
        _, st, dup, _ = run(nm)
        assert st[0] == 6 and not any(k.startswith(b"liar") for k in dup)
    # collisions: different names interleaved in one run still pair up; a lone candidate inside the run stays a fragment
    for bits in (4, 8):
        _, st, dup, _ = run("collide%d" % bits)
        assert st == (49, 24, 1, 20, 1, 0, 41, 6)                  # four signatures of six pairs each; the lone candidate lies on a pair's end
    # a run of 64 pairs up, a run of 65 is crowded
    _, st, dup, _ = run("crowd")
    assert st[5] == 65 and st[1] == 3
    k64, k65 = [n for n in dup if n.startswith(b"in_the_run_of_64_")][0], [n for n in dup if n.startswith(b"in_the_run_of_65_")][0]
    d64, d65 = [n for n in dup if n.startswith(b"dup_of_the_64_")][0], [n for n in dup if n.startswith(b"dup_of_the_65_")][0]
    assert dup[k64] == [False, False] and dup[d64] == [True, True] and dup[k65] == [True, True] and dup[d65] == [False, False]
    assert run("empty")[1] == (0,) * 8


def test_the_range_error_names_the_first_record(exe, workdir):
    n_chr, recs, hash_bits, _ = CASES["range"]
    raw = b"".join(recs)
    got = mdi.run_program(exe, workdir, "range", n_chr, raw, hash_bits)
    with pytest.raises(mdi.RangeError) as x:
        mdi.twin(raw, n_chr, hash_bits)
    assert got["bad"] == x.value.args[0] == 0 and got["marked"] == raw
    got = mdi.run_program(exe, workdir, "range2", n_chr, b"".join(recs[1:]), hash_bits)
    assert got["bad"] == 1


def test_random_records_and_their_shuffled_copy(exe, workdir):
    rng = random.Random(20)
    recs = sorted(mdi.random_records(rng, 3000, 3), key=lambda r: bsi.key(r, 3))
    _, st, _, _ = _check(exe, workdir, "random", 3, recs, mdi.HASH_BITS)
    assert st[0] > 2500 and st[1] > 800 and st[3] > 500 and st[4] > 300 and 6 <= st[7] <= 12
    assert _check(exe, workdir, "random6", 3, recs, 6)[1][5] == 0                 # 64 runs of some thirty candidates: different names side by side in every run
    assert _check(exe, workdir, "random4", 3, recs, 4)[1][1] == 0                 # 16 runs of more than a hundred: every run crowded, no pair left
    # where scores differ, the verdict does not depend on the order of equal keys
    recs = mdi.random_records(rng, 3000, 3, distinct_scores=True)
    one = _check(exe, workdir, "distinct", 3, sorted(recs, key=lambda r: bsi.key(r, 3)), mdi.HASH_BITS)
    rng.shuffle(recs)
    two = _check(exe, workdir, "distinct_shuffled", 3, sorted(recs, key=lambda r: bsi.key(r, 3)), mdi.HASH_BITS)
    assert mdi.flags_by_name(one[0]) == mdi.flags_by_name(two[0]) and one[1] == two[1] and one[1][3] > 300


def test_sanitized_program_over_every_case(workdir):
    san = mdi.build_program(workdir, sanitize=True)
    rng = random.Random(21)
    cases = [(k,) + CASES[k][:3] for k in sorted(CASES)] + [("random", 3, sorted(mdi.random_records(rng, 1500, 3), key=lambda r: bsi.key(r, 3)), 5)]
    for name, n_chr, recs, hash_bits in cases:
        raw = b"".join(recs)
        got = mdi.run_program(san, workdir, "san_" + name, n_chr, raw, hash_bits)
        if name == "range":
            assert got["bad"] == 0
        else:
            assert got["marked"] == mdi.twin(raw, n_chr, hash_bits)[0]
