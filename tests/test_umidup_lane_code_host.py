"""CPU suite: the host-callable code of the device's UMI-aware duplicate marking (dart_amd/csrc/dg_umidup.h) through tests/native/umidup_checks.hip -- a record's
U from the one pass over its name, the sorts with U among the keys, heads, groups, families, the walk of a family's groups, the byte written -- against the
sequential Python twin of tests/umidup_inputs.py, and the twin against a brute-force verdict.  The marking is the definition in include/dartgpu.h; no umi_tools
is run."""
import random
import pytest
import bamsort_inputs as bsi
import markdup_inputs as mdi
import umidup_inputs as udi

CASES = udi.crafted_cases()
PLAIN = mdi.crafted_cases()


@pytest.fixture(scope="module")
def exe(workdir):
    return udi.build_program(workdir)


def _check(exe, workdir, tag, n_chr, recs, max_edit, sep=b"_", hash_bits=udi.HASH_BITS):
    """program == twin == brute force -> (marked bytes, stats, {name: [verdicts]} of the examined records, the program's result)"""
    raw = b"".join(recs)
    got = udi.run_program(exe, workdir, "%s_e%d" % (tag, max_edit), n_chr, raw, max_edit, sep, hash_bits)
    marked, stats, verdict = udi.twin(raw, n_chr, max_edit, sep, hash_bits)
    assert got["bad"] is None
    offs = mdi.offsets(raw)
    for i, at in enumerate(offs):
        r = mdi.examine(raw, at, n_chr, i)
        if r is None:
            assert got["recs"][i][:2] == (0, 0) and got["recs"][i][5] == 0 and i not in got["dup"]
        else:
            assert got["recs"][i] == (1, int(r["cand"]), r["E"], r["score"], mdi.name_hash(r["name"], hash_bits) if r["cand"] else 0, udi.umi_of(r["name"], sep))
    assert got["dup"] == verdict
    assert got["marked"] == marked and got["stats"] == stats
    assert verdict == udi.brute(raw, n_chr, max_edit, sep, hash_bits)
    assert stats[6] == 2 * stats[3] + stats[4] == sum(verdict.values()) and stats[0] == 2 * stats[1] + stats[2] == len(verdict)
    # nothing but bit 0x400 of examined records differs from the input; the call is idempotent
    diff = [k for k in range(len(raw)) if raw[k] != marked[k]]
    assert len(marked) == len(raw) and all(k - 19 in offs and offs.index(k - 19) in verdict and raw[k] ^ marked[k] == 4 for k in diff)
    assert udi.twin(marked, n_chr, max_edit, sep, hash_bits)[:2] == (marked, stats)
    names = {}
    for i, dup in verdict.items():
        names.setdefault(recs[i][36:36 + recs[i][12] - 1], []).append(dup)
    return marked, stats, names, got


@pytest.mark.parametrize("max_edit", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_lane_code_equals_the_twin_equals_brute_force_on_the_crafted_records(name, max_edit, exe, workdir):
    n_chr, recs = CASES[name]
    _check(exe, workdir, name, n_chr, recs, max_edit)


def test_what_the_crafted_records_are_there_for(exe, workdir):
    run = lambda name, max_edit: _check(exe, workdir, name + "_again", *CASES[name], max_edit)
    plain = lambda name: mdi.twin(b"".join(CASES[name][1]), CASES[name][0])
    dups = lambda names, umi: sum(d[0] for n, d in names.items() if n.endswith(b"_" + umi))           # marked pairs under that UMI
    code = lambda t: sum((b"ACGTN+-".index(c) + 1) << 3 * (len(t) - 1 - k) for k, c in enumerate(t))
    # the suffix: no sep, empty, 21 and 22 letters, lower case, + and -, sep inside the UMI, another byte, a name that is nothing but sep and UMI
    _, st, _, got = run("suffix", 0)
    U = dict(zip(udi.names_of(CASES["suffix"][1]), (r[5] for r in got["recs"])))
    assert U[b"nosep"] == U[b"empty_"] == U[b"lower_acgt"] == U[b"digit_AC1T"] == U[b"u22_" + b"ACGTN+-" * 3 + b"A"] == 0
    assert U[b"u21_" + b"ACGTN+-" * 3] == code(b"ACGTN+-" * 3) and U[b"u21_" + b"ACGTN+-" * 3] >> 60 == 1 and U[b"pm_A+-"] == 0o167
    assert U[b"in_side_ACG"] == 0o123 and U[b"x_AC_GT"] == 0o34 and U[b"_T"] == 4 and U[b"one_N"] == 5 and st[8] == 6
    assert udi.run_program(exe, workdir, "suffix_x", 2, b"".join(CASES["suffix"][1]), 0, b"x")["recs"][[n for n in U].index(b"x_AC_GT")][5] == 0       # behind the last 'x': "_AC_GT"
    # one position, three UMIs: nobody is marked, where the plain marking keeps one pair of three
    for e in (0, 1):
        _, st, names, _ = run("different_umis", e)
        assert st[3] == st[6] == 0 and st[9] == 1 and st[7] == 1 and st[10] == 0
    assert plain("different_umis")[1][3] == 2
    # one UMI: as the plain marking
    for e in (0, 1):
        marked, st, names, _ = run("same_umi", e)
        assert marked == plain("same_umi")[0] and st[:8] == plain("same_umi")[1] and st[3] == 2 and st[9] == 0
    # 3 and 1 one letter apart join (3 >= 2 * 1 - 1); exact keeps them apart.  The better score of the absorbed group's pair makes it the cluster's survivor
    _, st, names, _ = run("join_3_1", 1)
    assert st[3] == 3 and st[10] == 3 and st[7] == 4 and dups(names, b"ACGTAA") == 0 and dups(names, b"ACGTAC") == 3        # (absorbed: the pair family and both end families)
    _, st, names, _ = run("join_3_1", 0)
    assert st[3] == 2 and st[10] == 0 and st[7] == 3
    # 2 and 2 stay apart (2 < 2 * 2 - 1); distance 2 and other lengths stay apart; U = 0 takes nobody in and joins nobody
    # (zero_never_joins: four pairs have U = 0, the suffix "bad" among them: one group; the pair under "A" is the other)
    for name, marked_pairs in (("apart_2_2", 2), ("distance_2", 2), ("lengths", 2), ("zero_never_joins", 3)):
        _, st, names, _ = run(name, 1)
        assert st[3] == marked_pairs and st[10] == 0, name
    # A(10) - B(4) - C(1): B joins A, C's only neighbour is no root: C stays one
    _, st, names, _ = run("one_hop_chain", 1)
    assert st[3] == 13 and st[10] == 3 and st[7] == 14 and dups(names, b"ACGTTA") == 0 and dups(names, b"ACGTAA") == 4 and dups(names, b"ACGTAC") == 9
    # three groups of one pair: the smaller U is walked first, so {AAAAAA, AAAAAC} and {AAAACC}, not {AAAAAA} and {AAAAAC, AAAACC}
    _, st, names, _ = run("count_ties", 1)
    assert (dups(names, b"AAAAAA"), dups(names, b"AAAAAC"), dups(names, b"AAAACC")) == (1, 0, 0) and st[10] == 3
    # a fragment loses to a pair end of its cluster, not to one of another cluster at the same E; within a cluster the best fragment stays
    _, st, names, _ = run("fragment_and_pair_end", 0)
    assert names[b"f_same_AAAAAA"] == [True] and names[b"f_other_CCCCCC"] == [False] and names[b"f_other_worse_CCCCCC"] == [True] and names[b"f_near_AAAAAC"] == [False]
    _, st, names, _ = run("fragment_and_pair_end", 1)
    assert names[b"f_same_AAAAAA"] == [True] and names[b"f_other_CCCCCC"] == [False] and names[b"f_near_AAAAAC"] == [True]
    assert plain("fragment_and_pair_end")[1][4] == 4                     # by position alone all four fragments lose to the pair
    # 64 groups are clustered, 65 are crowded
    _, st, names, _ = run("family_of_64", 1)
    assert st[10] == 3 and st[11] == 0 and st[3] == 3 and st[7] == 4
    _, st, names, _ = run("family_of_65", 1)
    assert st[10] == 0 and st[11] == 3 and st[3] == 2 and st[7] == 3
    assert run("family_of_65", 0)[1][11] == 3
    assert run("empty", 1)[1] == (0,) * 12


@pytest.mark.parametrize("name", sorted(n for n in PLAIN if n != "range"))
def test_without_any_umi_the_result_is_the_plain_marking(name, exe, workdir):
    n_chr, recs, hash_bits, _ = PLAIN[name]
    raw = b"".join(recs)
    for max_edit in (0, 1):
        marked, st, _, _ = _check(exe, workdir, "plain_" + name, n_chr, recs, max_edit, b"_", hash_bits)
        assert st[8] == 0 and (marked, st[:8]) == mdi.twin(raw, n_chr, hash_bits)[:2] and st[9] == st[10] == 0


def test_the_range_error_names_the_first_record(exe, workdir):
    n_chr, recs, hash_bits, _ = PLAIN["range"]
    raw = b"".join(recs)
    got = udi.run_program(exe, workdir, "range", n_chr, raw, 1)
    with pytest.raises(mdi.RangeError) as x:
        udi.twin(raw, n_chr, 1)
    assert got["bad"] == x.value.args[0] == 0 and got["marked"] == raw


def test_random_records_and_their_shuffled_copy(exe, workdir):
    rng = random.Random(22)
    recs = sorted(udi.random_records(rng, 3000, 3), key=lambda r: bsi.key(r, 3))
    _, s0, _, _ = _check(exe, workdir, "random", 3, recs, 0)
    _, s1, _, _ = _check(exe, workdir, "random", 3, recs, 1)
    plain = mdi.twin(b"".join(recs), 3)[1]
    assert s0[0] > 2500 and s0[1] > 800 and 0.85 * s0[0] < s0[8] < 0.95 * s0[0] and s0[9] > 100 and s0[10] == 0 and s1[10] > 50
    assert 0 < s0[3] < s1[3] < plain[3] and 0 < s0[4] <= s1[4] < plain[4]
    assert _check(exe, workdir, "random7", 3, recs, 1, hash_bits=7)[1][1] > 400               # 128 runs: different names side by side in every run, some runs crowded
    assert _check(exe, workdir, "random4", 3, recs, 1, hash_bits=4)[1][1] == 0                # 16 runs of more than a hundred: every run crowded, no pair left
    assert _check(exe, workdir, "random_colon", 3, recs, 1, sep=b":")[1][8] == 0
    # where scores differ, the verdict does not depend on the order of equal keys
    recs = udi.random_records(rng, 3000, 3, distinct_scores=True)
    one = _check(exe, workdir, "distinct", 3, sorted(recs, key=lambda r: bsi.key(r, 3)), 1)
    rng.shuffle(recs)
    two = _check(exe, workdir, "distinct_shuffled", 3, sorted(recs, key=lambda r: bsi.key(r, 3)), 1)
    assert mdi.flags_by_name(one[0]) == mdi.flags_by_name(two[0]) and one[1] == two[1] and one[1][3] > 100


def test_sanitized_program_over_every_case(workdir):
    san = udi.build_program(workdir, sanitize=True)
    rng = random.Random(23)
    cases = [(k,) + CASES[k] + (udi.HASH_BITS,) for k in sorted(CASES)] + [("plain_" + k,) + PLAIN[k][:3] for k in sorted(PLAIN)] + \
            [("random", 3, sorted(udi.random_records(rng, 1500, 3), key=lambda r: bsi.key(r, 3)), 5)]
    for name, n_chr, recs, hash_bits in cases:
        raw = b"".join(recs)
        for max_edit in (0, 1):
            got = udi.run_program(san, workdir, "san_" + name, n_chr, raw, max_edit, b"_", hash_bits)
            if name == "plain_range":
                assert got["bad"] == 0
            else:
                assert got["marked"] == udi.twin(raw, n_chr, max_edit, b"_", hash_bits)[0]
