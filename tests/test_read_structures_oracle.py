"""CPU suite: every class of tests/read_structures.py reaches the path of the reference algorithm it was made for.  The classes are mapped with the
oracle (never the GPU) and judged by its records, so that an identical GPU result on them is an identical result on that path and not on plain
reads.  Shares the committed 101-base set gives (N_PER_CLASS = 70 pairs per class, one event read per pair), next to the bound asserted:

  two_junctions, middle exon >= 16, -mis 12 -m: two or more N         32 of 34        (bound: half)
  two_junctions, middle exon 6-11, -mis 12 -m: an I >= 4 and an N     16 of 18        (half)
  overhang 1-13: soft-clipped, no junction                            32 of 35        (80 %; the other three match the text by chance: 101M)
  overhang 14-19: a junction in 22, a clip in 13 of 35                                (15 % each)
  del_4_30 / del_31_120: an N or a D                                  68 / 69 of 70   (80 %)
  ins_4_30, -mis 30: an I >= 4                                        66 of 70        (60 %)
  ins_4_30, -mis 5: unmapped                                          66 of 70        (a third)
  noise_island / two_noise_islands, -mis 30: three or more operations 68 / 65 of 70   (half)
  chimera_other_strand / chimera_other_chromosome: clipped at 35-65   68 / 66 of 70   (60 %)
  pair_mate_noise: mate 1 mapped 70 of 70, mate 2 mapped 0 of 70, under every flag set (all; none)
  the other pair classes: both mates mapped in 70 of 70 pairs, under every flag set   (all, see PAIR_BOTH_MAPPED)
  pair_unequal_length, under every flag set: 101 bases 70 of 70, 36 bases 35 of 35, 14 bases 0 of 35 mapped   (all; all; none)
  junction tuples over the set, -mis 12 -m: type 0: 66, type 1: 81, type 2: 2, type 3: 1   (20 of each strand type)

and the 250-base set (the pair classes as above under -mis 5, -mis 12 -m, -mis 30 and -mis 100: 70 of 70, the noise mate 0 of 70, mates of 50 bases 70 of 70):

  three_junctions, both middle exons >= 16, every flag set: three N   22 of 30        (half; over the whole class 24 of 70 carry three N, 35 two)
  ins_31_80, -mis 5 / -mis 12 -m / -mis 30: unmapped                  70 of 70        (80 %)
  ins_31_80, -mis 100: an I >= 31                                     70 of 70        (half); an I >= 65 in 25 (five: a class of 31-80 must keep some beyond 64)
"""
import numpy as np
import pytest
import common, oracle_py, read_structures as rs, read_structure_inputs as rsi
from dart_amd import host

# The mates of these classes are copies of the text without errors and the reads are pinned by their digest, so every mate maps: the whole class, not a share of it.
# (pair_mate_noise and pair_unequal_length are judged by mate: a random mate and a mate of 14 bases, fewer than any seed, stay unmapped.)
PAIR_BOTH_MAPPED = ("pair_same_strand", "pair_outie", "pair_contained", "pair_dovetail", "pair_identical_mates", "pair_other_chromosome",
                    "pair_far", "pair_mate_high_copy", "pair_swapped_files", "pair_both_multi")


def _map_set(name, workdir):
    """({(class, flags): (per-read best CIGARs, junction tuples)}, {class: info}) of one set, every class mapped on its own, paired, under the set's flag sets"""
    c, classes, info = rsi.read_set(name, workdir)
    orc = oracle_py.Oracle(c["prefix"])
    out = {}
    for flags in rsi.SET_FLAGS[name]:
        p, _ = common.parse_flags(flags)
        for cls, pairs in classes.items():
            so, rl, flat = host.pack_reads(rs.as_reads(pairs))
            reads, rep, cig, sj = orc.map_batch(orc.params(paired=1, **p), so, rl, flat, threads=4)
            out[cls, " ".join(flags)] = (rsi.best_cigars(reads, rep, cig), sj)
    orc.close()
    return out, info


@pytest.fixture(scope="module")
def mapped(workdir):
    """the 101-base set"""
    return _map_set("rs101", workdir)


@pytest.fixture(scope="module")
def mapped250(workdir):
    """the 250-base set"""
    return _map_set("rs250", workdir)


def _event_cigars(mapped, name, flags, keep=lambda inf: True):
    out, info = mapped
    best, _ = out[name, flags]
    return [best[2 * i + inf["event_mate"]] for i, inf in enumerate(info[name]) if keep(inf)]


def _count(cigars, pred):
    return sum(1 for c in cigars if c is not None and pred(c))


def _n_ops(c, op, at_least=1):
    return sum(1 for l, o in c if o == op and l >= at_least)


def test_two_junction_reads_take_both_forms(mapped):
    wide = _event_cigars(mapped, "two_junctions", "-mis 12 -m", lambda inf: inf["middle_exon"] >= 16)
    got = _count(wide, lambda c: _n_ops(c, "N") >= 2)
    print("middle exon >= 16: two N in %d of %d" % (got, len(wide)))
    assert len(wide) >= 30 and got >= 0.5 * len(wide)
    narrow = _event_cigars(mapped, "two_junctions", "-mis 12 -m", lambda inf: inf["middle_exon"] <= 11)
    got = _count(narrow, lambda c: _n_ops(c, "I", 4) >= 1 and _n_ops(c, "N") >= 1)
    print("middle exon 6-11: I >= 4 with N in %d of %d" % (got, len(narrow)))
    assert len(narrow) >= 15 and got >= 0.5 * len(narrow)


def test_overhangs_are_clipped_or_spliced(mapped):
    for flags in ("-mis 5", "-mis 12 -m"):
        short = _event_cigars(mapped, "overhang", flags, lambda inf: inf["overhang"] <= 13)
        clipped = _count(short, lambda c: _n_ops(c, "S") >= 1 and _n_ops(c, "N") == 0)
        print("%s overhang 1-13: clipped %d of %d" % (flags, clipped, len(short)))
        assert len(short) >= 30 and clipped >= 0.8 * len(short)
        longer = _event_cigars(mapped, "overhang", flags, lambda inf: inf["overhang"] >= 14)
        spliced = _count(longer, lambda c: _n_ops(c, "N") >= 1)
        clipped = _count(longer, lambda c: _n_ops(c, "S") >= 1 and _n_ops(c, "N") == 0)
        print("%s overhang 14-19: junction %d, clipped %d of %d" % (flags, spliced, clipped, len(longer)))
        assert len(longer) >= 30 and spliced >= 0.15 * len(longer) and clipped >= 0.15 * len(longer)


def test_long_indels(mapped):
    for name in ("del_4_30", "del_31_120"):
        ev = _event_cigars(mapped, name, "-mis 12 -m")
        got = _count(ev, lambda c: _n_ops(c, "N") + _n_ops(c, "D") >= 1)
        print("%s: N or D in %d of %d" % (name, got, len(ev)))
        assert got >= 0.8 * len(ev)
    ev = _event_cigars(mapped, "ins_4_30", "-mis 30")
    got = _count(ev, lambda c: _n_ops(c, "I", 4) >= 1)
    print("ins_4_30 -mis 30: I >= 4 in %d of %d" % (got, len(ev)))
    assert got >= 0.6 * len(ev)
    ev = _event_cigars(mapped, "ins_4_30", "-mis 5")
    un = sum(1 for c in ev if c is None)
    print("ins_4_30 -mis 5: unmapped %d of %d" % (un, len(ev)))
    assert un >= len(ev) / 3


def test_noise_islands_map_through_chains_of_small_pairs(mapped):
    for name in ("noise_island", "two_noise_islands"):
        ev = _event_cigars(mapped, name, "-mis 30")
        got = _count(ev, lambda c: len(c) >= 3)
        print("%s -mis 30: three or more operations in %d of %d" % (name, got, len(ev)))
        assert got >= 0.5 * len(ev)


def test_chimeras_are_clipped_at_the_join(mapped):
    for name in ("chimera_other_strand", "chimera_other_chromosome"):
        ev = _event_cigars(mapped, name, "-mis 12 -m")
        got = _count(ev, lambda c: any(o == "S" and 35 <= l <= 65 for l, o in c))
        print("%s: clipped at 35-65 in %d of %d" % (name, got, len(ev)))
        assert got >= 0.6 * len(ev)


def _assert_pair_classes(out, info, flag_sets, short_unmapped):
    for flags in flag_sets:
        best, _ = out["pair_mate_noise", flags]
        n = len(best) // 2
        m1 = sum(1 for c in best[0::2] if c is not None); m2 = sum(1 for c in best[1::2] if c is not None)
        print("%s pair_mate_noise: mate 1 mapped %d, mate 2 mapped %d of %d" % (flags, m1, m2, n))
        assert m2 == 0 and m1 == n, flags
        for name in PAIR_BOTH_MAPPED:
            best, _ = out[name, flags]
            both = sum(1 for a, b in zip(best[0::2], best[1::2]) if a is not None and b is not None)
            print("%s %s: both mates mapped in %d of %d" % (flags, name, both, len(best) // 2))
            assert both == len(best) // 2, (name, flags)
        # unequal lengths: the long mate maps, and so does the short one, but for the mate of 14 bases (shorter than any seed)
        best, _ = out["pair_unequal_length", flags]
        mates = [(len_, best[2 * i + m]) for i, inf in enumerate(info["pair_unequal_length"]) for m, len_ in enumerate(inf["lengths"])]
        print("%s pair_unequal_length: mapped mates by length %s" % (flags, {l: "%d of %d" % (sum(1 for a, c in mates if a == l and c is not None), sum(1 for a, c in mates if a == l))
                                                                         for l in sorted(set(a for a, c in mates))}))
        for l, c in mates:
            assert (c is None) == (l == short_unmapped), (flags, l)
    assert short_unmapped is None or any(l == short_unmapped for l, c in mates)


def test_pair_classes_map_as_meant(mapped):
    out, info = mapped
    _assert_pair_classes(out, info, ("-mis 5", "-mis 12 -m", "-mis 30"), 14)


def test_pair_classes_of_250_base_reads_map_as_meant(mapped250):
    """(250 + 50 bases: both mates map)"""
    out, info = mapped250
    _assert_pair_classes(out, info, ("-mis 5", "-mis 12 -m", "-mis 30", "-mis 100"), None)


def test_classes_of_250_base_reads_only(mapped250):
    """three_junctions: with both middle exons of at least 16 bases the read carries three N operations (the bound of two_junctions, half, taken over: a middle exon of at
    least 16 bases gives its two N there).  ins_31_80: unmapped under every flag set up to -mis 30, since the inserted bases count against -mis; at -mis 100 the read maps
    through the wave-wide alignment of a segment pair wider than 64 columns and carries an I of at least 31 (bound: half, as for the issue's other shares of this kind --
    an insertion whose random bases happen to continue the text comes out shorter, and a few reads are clipped instead)."""
    for flags in ("-mis 12 -m", "-mis 30", "-mis 100"):
        wide = _event_cigars(mapped250, "three_junctions", flags, lambda inf: min(inf["middle_exons"]) >= 16)
        got = _count(wide, lambda c: _n_ops(c, "N") >= 3)
        print("three_junctions %s, both middle exons >= 16: three N in %d of %d" % (flags, got, len(wide)))
        assert len(wide) >= 25 and got >= 0.5 * len(wide)
    every = _event_cigars(mapped250, "three_junctions", "-mis 30")
    print("three_junctions -mis 30, all: three N in %d, two N in %d of %d" % (_count(every, lambda c: _n_ops(c, "N") >= 3), _count(every, lambda c: _n_ops(c, "N") == 2), len(every)))
    for flags in ("-mis 5", "-mis 12 -m", "-mis 30"):
        ev = _event_cigars(mapped250, "ins_31_80", flags)
        un = sum(1 for c in ev if c is None)
        print("ins_31_80 %s: unmapped %d of %d" % (flags, un, len(ev)))
        assert un >= 0.8 * len(ev)
    ev = _event_cigars(mapped250, "ins_31_80", "-mis 100")
    got = _count(ev, lambda c: _n_ops(c, "I", 31) >= 1)
    over64 = _count(ev, lambda c: _n_ops(c, "I", 65) >= 1)
    print("ins_31_80 -mis 100: I >= 31 in %d, I >= 65 in %d of %d" % (got, over64, len(ev)))
    assert got >= 0.5 * len(ev) and over64 >= 5


def test_junction_tuples_of_both_strand_types_occur(mapped):
    out, _ = mapped
    types = np.concatenate([sj["type"] for (name, flags), (best, sj) in out.items() if flags == "-mis 12 -m"])
    kinds = set(types.tolist())
    print("junction tuple types:", {k: int((types == k).sum()) for k in sorted(kinds)})
    assert {0, 1} <= kinds and (types == 0).sum() >= 20 and (types == 1).sum() >= 20


def test_generator_is_a_pure_function_of_its_seed(workdir):
    c, classes, _ = rsi.read_set("rs101", workdir)
    again = rs.make(c["genome"], rsi.SEED, 101, rsi.N_PER_CLASS)
    assert rs.digest(again) == rs.digest(classes) == rsi.gold()["sets"]["rs101"]["reads_sha256"]
    other = rs.make(c["genome"], rsi.SEED + 1, 101, 5, only=("two_junctions", "pair_far"))
    assert list(other) == ["two_junctions", "pair_far"] and rs.digest(other) != rs.digest(rs.make(c["genome"], rsi.SEED, 101, 5, only=("two_junctions", "pair_far")))
    for name in rs.SPLICED_AND_INDEL + rs.NOISE + rs.TANDEM + rs.CHIMERA + rs.SEAMS + rs.PAIRS:
        assert name in classes or name in ("three_junctions", "ins_31_80"), name      # (the two classes of 250-base reads only)
    c250, classes250, _ = rsi.read_set("rs250", workdir)
    assert "three_junctions" in classes250 and "ins_31_80" in classes250
    for cl in (classes, classes250):
        assert all(len(v) == rsi.N_PER_CLASS for v in cl.values())
    assert list(classes) == rs.class_names(101) and list(classes250) == rs.class_names(250)
