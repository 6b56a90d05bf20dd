"""CPU suite: the host-callable code of the device's gene counts (dart_amd/csrc/dg_genecount.h) through tests/native/genecount_checks.hip -- the flattening of
the annotation, the check of host records, every unit's rows -- against the sequential Python twin of tests/genecount_inputs.py, and the twin's segments
against a per-base painter.  The table is the definition in the header's comment (modelled on `htseq-count --mode union`, STAR's layout); neither tool is run."""
import random
import numpy as np
import pytest
import genecount_inputs as gci
from genecount_inputs import M, I, D, N, S, H, P, EQ, X

UN, MU, NF, AM = 0, 1, 2, 3
G = lambda g: 4 + g
MIN_MAPQ = 4

# ---- the crafted annotation: four chromosomes, chromosome 2 without exons ----
A, B, C1, C2, FOREIGN, W1, W2, WFOREIGN, OPP_PLUS, OPP_MINUS, DUP, LASTCHR, ATZERO = range(13)
N_CHR, N_GENES = 4, 13


def _annotation():
    ex = [(0, 1000, 1100, 0, A), (0, 1200, 1300, 0, A), (0, 2000, 2100, 0, B)]
    ex += [(0, 10000 + 3 * i, 10010 + 3 * i, 0, C1) for i in range(300)]                       # 300 ten-base exons, a new one every 3 bases: [10000, 10907)
    ex += [(0, 30000 + 3 * i, 30010 + 3 * i, 0, C2) for i in range(300)] + [(0, 30450, 30460, 0, FOREIGN)]
    ex += [(0, 50000 + 20 * i, 50010 + 20 * i, 0, W1) for i in range(300)]                     # the same with gaps: 599 segments under one 6000-base block
    ex += [(0, 70000 + 20 * i, 70010 + 20 * i, 0, W2) for i in range(300)] + [(0, 73012, 73018, 1, WFOREIGN)]
    ex += [(0, 90000, 90200, 0, OPP_PLUS), (0, 90100, 90300, 1, OPP_MINUS)]
    ex += [(1, 500, 600, 1, DUP), (1, 550, 650, 1, DUP), (1, 500, 600, 1, DUP), (1, 0, 50, 0, ATZERO)]
    ex += [(3, 100, 200, 0, LASTCHR)]
    return ex


EXONS = _annotation()


def _cases():
    """name -> (reads of the unit as Records.read keyword dicts, the rows the unit is there for)"""
    fwd = lambda c, pos, ops, **kw: dict(reports=[(c, pos, 0, ops)], **kw)
    m1 = lambda c, pos, ops, flag=0x41, **kw: dict(reports=[(c, pos, flag, ops)], **kw)
    m2 = lambda c, pos, ops, flag=0x91, **kw: dict(reports=[(c, pos, flag, ops)], **kw)
    un = dict(reports=[])
    plus = lambda g: (G(g), G(g), NF)
    singles = {
        "block_ends_on_a_segment_start": ([fwd(0, 901, [(100, M)])], (NF,) * 3),                # [900, 1000) and A begins at 1000
        "block_ends_one_behind_it": ([fwd(0, 902, [(100, M)])], plus(A)),
        "block_starts_on_a_segment_end": ([fwd(0, 1101, [(50, M)])], (NF,) * 3),                # [1100, 1150) and A's exon ends at 1100
        "block_starts_one_in_front": ([fwd(0, 1100, [(50, M)])], plus(A)),
        "in_front_of_the_first_segment": ([fwd(0, 5, [(50, M)])], (NF,) * 3),
        "behind_the_last_segment": ([fwd(0, 200001, [(50, M)])], (NF,) * 3),
        "chromosome_without_exons": ([fwd(2, 1001, [(50, M)])], (NF,) * 3),
        "last_chromosome": ([fwd(3, 151, [(20, M)])], plus(LASTCHR)),
        "chromosome_behind_the_last": ([fwd(4, 151, [(20, M)])], (NF,) * 3),
        "chromosome_minus_one": ([fwd(-1, 151, [(20, M)])], (NF,) * 3),
        "thousand_bases_over_300_exons": ([fwd(0, 9951, [(1000, M)])], plus(C1)),
        "the_same_with_a_foreign_exon": ([fwd(0, 29951, [(1000, M)])], (AM, AM, NF)),
        "six_thousand_over_300_exons_with_gaps": ([fwd(0, 49991, [(6020, M)])], plus(W1)),
        "the_same_with_a_foreign_exon_in_a_gap": ([fwd(0, 69991, [(6020, M)])], (AM, G(W2), G(WFOREIGN))),
        "all_ops": ([fwd(0, 1001, [(5, S), (10, M), (2, I), (3, D), (187, N), (4, EQ), (1, X), (6, P), (7, H)])], plus(A)),
        "eq_alone_makes_a_block": ([fwd(0, 1951, [(40, N), (5, EQ)])], (NF,) * 3),              # [1990, 1995)
        "eq_reaches_the_gene": ([fwd(0, 1951, [(50, N), (5, EQ)])], plus(B)),
        "x_reaches_the_gene": ([fwd(0, 1951, [(50, N), (5, X)])], plus(B)),
        "i_does_not_move": ([fwd(0, 1991, [(5, M), (10, I), (4, M)])], (NF,) * 3),              # [1990, 1995) [1995, 1999); moved: [2005, 2009) in B
        "s_does_not_move": ([fwd(0, 1996, [(10, S), (4, M)])], (NF,) * 3),
        "h_and_p_do_not_move": ([fwd(0, 1996, [(10, H), (10, P), (4, M)])], (NF,) * 3),
        "d_moves": ([fwd(0, 1991, [(4, M), (10, D), (4, M)])], plus(B)),
        "n_moves": ([fwd(0, 1991, [(4, M), (10, N), (4, M)])], plus(B)),
        "d_makes_no_block": ([fwd(0, 1951, [(4, M), (100, D)])], (NF,) * 3),                    # the D lies over B
        "op_9_and_above_change_nothing": ([fwd(0, 1996, [(10, 9), (10, 15), (4, M)])], (NF,) * 3),
        "zero_length_m_inside_a_gene": ([fwd(0, 2051, [(0, M)])], (NF,) * 3),
        "zero_length_m_then_a_block": ([fwd(0, 1951, [(0, M), (10, M)])], (NF,) * 3),
        "pos_1": ([fwd(1, 1, [(10, M)])], plus(ATZERO)),
        "pos_0": ([fwd(1, 0, [(10, M)])], (NF,) * 3),
        "pos_negative": ([fwd(1, -5, [(30, M)])], (NF,) * 3),
        "mapq_equal_to_min_counts": ([fwd(0, 2001, [(50, M)], mapq=MIN_MAPQ)], plus(B)),
        "mapq_one_below_does_not": ([fwd(0, 2001, [(50, M)], mapq=MIN_MAPQ - 1)], (MU,) * 3),
        "opposite_strands_overlap": ([fwd(0, 90121, [(50, M)])], (AM, G(OPP_PLUS), G(OPP_MINUS))),
        "the_same_from_a_reverse_read": ([dict(reports=[(0, 90121, 16, [(50, M)])])], (AM, G(OPP_MINUS), G(OPP_PLUS))),
        "overlapping_and_duplicate_exons": ([dict(reports=[(1, 521, 16, [(100, M)])])], plus(DUP)),      # a reverse read on a minus gene
        "unmapped_single": ([un], (UN,) * 3),
        "single_mode_shows_the_report_that_has_the_score": ([dict(reports=[(0, 2001, 0, [(50, M)], 90), (0, 1001, 0, [(50, M)], 100)], score=100)], plus(A)),
        "single_mode_no_report_has_the_score": ([dict(reports=[(0, 2001, 0, [(50, M)], 90)], score=100)], (UN,) * 3),
        "reports_in_front_of_best_are_not_looked_at": ([dict(reports=[(0, 2001, 0, [(50, M)], 100), (0, 1001, 0, [(50, M)], 100)], best=1)], plus(A)),
        "tail_read_a": ([fwd(0, 1001, [(50, M)])], plus(A)),                                     # two neighbours behind n_pair_mode are two units, not a pair
        "tail_read_b": ([fwd(0, 2001, [(50, M)])], plus(B)),
    }
    pairs = {
        "mates_in_the_same_gene": ([m1(0, 1001, [(50, M)]), m2(0, 1201, [(50, M)])], plus(A)),
        "mates_in_two_genes": ([m1(0, 1001, [(50, M)]), m2(0, 2001, [(50, M)])], (AM, AM, NF)),
        "one_mate_in_a_gene_one_in_nothing": ([m1(0, 1001, [(50, M)]), m2(0, 5001, [(50, M)])], plus(A)),
        "one_mate_unaligned": ([un, m2(0, 1201, [(50, M)])], plus(A)),
        "the_other_mate_unaligned": ([m1(0, 1001, [(50, M)]), un], plus(A)),
        "both_unaligned": ([un, un], (UN,) * 3),
        "one_mate_below_min_mapq": ([m1(0, 1001, [(50, M)]), m2(0, 1201, [(50, M)], mapq=3)], (MU,) * 3),
        "an_unaligned_mates_mapq_is_not_looked_at": ([dict(reports=[(0, 1001, 0x41, [(50, M)], 0)], score=50, mapq=0), m2(0, 1201, [(50, M)])], plus(A)),
        "mates_with_different_s": ([m1(0, 1001, [(50, M)]), m2(0, 1201, [(50, M)], flag=0x81)], (G(A),) * 3),
        "mate_2_forward_alone": ([un, m2(0, 1201, [(50, M)], flag=0x81)], (G(A), NF, G(A))),
        "pair_mode_shows_a_positive_score": ([dict(reports=[(0, 2001, 0x41, [(50, M)], 0), (0, 1001, 0x41, [(50, M)], 37)], score=100), un], plus(A)),
        "spliced_mate_over_both_exons": ([m1(0, 1051, [(50, M), (100, N), (50, M)]), m2(0, 1251, [(40, M)])], plus(A)),
    }
    return pairs, singles


PAIRS, SINGLES = _cases()


def _records(pairs, singles):
    rec = gci.Records()
    for reads in list(pairs) + list(singles):
        for kw in reads:
            rec.read(**kw)
    return rec.arrays(), 2 * len(pairs)


@pytest.fixture(scope="module")
def exe(workdir):
    return gci.build_program(workdir)


def _check(exe, workdir, tag, n_chr, n_genes, exons, arrays, n_pair_mode, min_mapq=MIN_MAPQ):
    reads, reports, cigar = arrays
    got = gci.run_program(exe, workdir, tag, n_chr, n_genes, exons, reads, reports, cigar, n_pair_mode, min_mapq)
    segs = gci.flatten(n_chr, exons)
    assert got["err"] is None and got["bad"] is None and got["segs"] == segs
    counts, rows = gci.twin(n_chr, n_genes, exons, reads, reports, cigar, n_pair_mode, min_mapq, segs=segs, want_rows=True)
    assert got["rows"] == rows
    assert np.array_equal(got["counts"], counts) and (got["counts"].sum(axis=0) == len(rows)).all()
    return got


def test_the_flattening_equals_the_twin_and_the_painter(exe, workdir):
    got = _check(exe, workdir, "flat", N_CHR, N_GENES, EXONS, _records([], [])[0], 0)
    gci.assert_painter_agrees(N_CHR, N_GENES, EXONS, got["segs"], limit=1 << 17)
    s0 = got["segs"][0]
    assert s0[:5] == [(1000, A, A, gci.NONE), (1100,) + (gci.NONE,) * 3, (1200, A, A, gci.NONE), (1300,) + (gci.NONE,) * 3, (2000, B, B, gci.NONE)]
    assert (10000, C1, C1, gci.NONE) in s0 and (10907,) + (gci.NONE,) * 3 in s0 and not any(10000 < s[0] < 10907 for s in s0)      # 300 overlapping exons: one segment
    assert [s for s in s0 if 30000 <= s[0] <= 30907] == [(30000, C2, C2, gci.NONE), (30450, gci.AMBIG, gci.AMBIG, gci.NONE), (30460, C2, C2, gci.NONE), (30907,) + (gci.NONE,) * 3]
    assert len([s for s in s0 if 50000 <= s[0] < 56000]) == 600
    assert [s for s in s0 if 90000 <= s[0] <= 90300] == [(90000, OPP_PLUS, OPP_PLUS, gci.NONE), (90100, gci.AMBIG, OPP_PLUS, OPP_MINUS), (90200, OPP_MINUS, gci.NONE, OPP_MINUS),
                                                         (90300,) + (gci.NONE,) * 3]
    assert got["segs"][1] == [(0, ATZERO, ATZERO, gci.NONE), (50,) + (gci.NONE,) * 3, (500, DUP, gci.NONE, DUP), (650,) + (gci.NONE,) * 3]      # overlapping and repeated exons: one segment
    assert got["segs"][2] == [] and got["segs"][3] == [(100, LASTCHR, LASTCHR, gci.NONE), (200,) + (gci.NONE,) * 3]
    # the input's order does not matter
    shuffled = list(EXONS); random.Random(3).shuffle(shuffled)
    assert _check(exe, workdir, "flat_shuffled", N_CHR, N_GENES, shuffled, _records([], [])[0], 0)["segs"] == got["segs"]


def test_what_the_crafted_units_are_there_for(exe, workdir):
    p_names, s_names = sorted(PAIRS), sorted(SINGLES)
    arrays, npm = _records([PAIRS[k][0] for k in p_names], [SINGLES[k][0] for k in s_names])
    assert npm == 2 * len(p_names) and len(arrays[0]) > npm and (len(arrays[0]) - npm) % 2 == 1      # an odd tail behind n_pair_mode
    got = _check(exe, workdir, "crafted", N_CHR, N_GENES, EXONS, arrays, npm)
    for k, name in enumerate(p_names):
        assert got["rows"][k] == PAIRS[name][1], name
    for k, name in enumerate(s_names):
        assert got["rows"][len(p_names) + k] == SINGLES[name][1], name
    # the same reads with n_pair_mode 0: every read a unit of its own (the mates in two genes are two counted units)
    alone = _check(exe, workdir, "crafted_alone", N_CHR, N_GENES, EXONS, arrays, 0)
    k = 2 * p_names.index("mates_in_two_genes")
    assert alone["rows"][k] == (G(A), G(A), NF) and alone["rows"][k + 1] == (G(B), G(B), NF)
    # each unit alone in a batch gives the same rows (nothing leaks from a neighbour)
    for name in ("mates_with_different_s", "one_mate_below_min_mapq"):
        one, npm1 = _records([PAIRS[name][0]], [])
        assert _check(exe, workdir, "one_" + name, N_CHR, N_GENES, EXONS, one, npm1)["rows"] == [PAIRS[name][1]]
    # min_mapq 0 counts everything that is aligned
    zero = _check(exe, workdir, "crafted_q0", N_CHR, N_GENES, EXONS, arrays, npm, min_mapq=0)
    assert zero["counts"][MU].sum() == 0 and zero["rows"][p_names.index("one_mate_below_min_mapq")] == (G(A), G(A), NF)


def test_one_gene_and_no_exons(exe, workdir):
    arrays, npm = _records([PAIRS[k][0] for k in sorted(PAIRS)], [SINGLES[k][0] for k in sorted(SINGLES)])
    got = _check(exe, workdir, "one_gene", N_CHR, 1, [(0, 1000, 1300, 0, 0)], arrays, npm)
    assert got["counts"].shape == (5, 3) and got["counts"][4, 0] > 5 and got["counts"][AM].sum() == 0
    got = _check(exe, workdir, "no_exons", N_CHR, 3, [], arrays, npm)
    assert got["segs"] == [[], [], [], []] and got["counts"][4:].sum() == 0 and got["counts"][AM].sum() == 0
    want = gci.twin(N_CHR, N_GENES, EXONS, *arrays, npm, MIN_MAPQ)
    assert got["counts"][UN, 0] == want[UN, 0] and got["counts"][MU, 0] == want[MU, 0] and (got["counts"][NF] == len(PAIRS) + len(SINGLES) - int(want[UN, 0]) - int(want[MU, 0])).all()


@pytest.mark.parametrize("k, exon, word", [(1, (4, 10, 20, 0, 0), "chromosome"), (0, (-1, 10, 20, 0, 0), "chromosome"), (2, (0, 20, 20, 0, 0), "start < end"),
                                            (1, (0, 30, 20, 0, 0), "start < end"), (3, (0, 10, 20, 2, 0), "strand"), (0, (0, 10, 20, 0, 13), "gene")])
def test_a_bad_exon_is_named(k, exon, word, exe, workdir):
    exons = list(EXONS[:5]); exons.insert(k, exon); exons.append((9, 5, 1, 7, 99))          # (a later one, worse: the first is named)
    arrays, _ = _records([], [])
    got = gci.run_program(exe, workdir, "badexon_%d_%s" % (k, word[:4]), N_CHR, N_GENES, exons, *arrays, 0, MIN_MAPQ)
    assert got["err"] is not None and got["err"].startswith("exon %d " % k) and word in got["err"] and not any(got["segs"])


def test_no_gene_is_refused_and_the_largest_coordinates_fit(exe, workdir):
    arrays, _ = _records([], [])
    assert gci.run_program(exe, workdir, "nogene", N_CHR, 0, [], *arrays, 0, MIN_MAPQ)["err"] is not None
    top = (1 << 32) - 1
    rec = gci.Records().read(reports=[(0, top - 9, 0, [(10, M)])]).read(reports=[(0, top - 9, 0, [(9, M)])]).read(reports=[(0, top + 1, 0, [(50, M)])])
    got = _check(exe, workdir, "edge", 1, 2, [(0, top - 1, top, 1, 1), (0, 0, 1, 0, 0)], rec.arrays(), 0)
    assert got["segs"][0] == [(0, 0, 0, gci.NONE), (1,) + (gci.NONE,) * 3, (top - 1, 1, gci.NONE, 1), (top,) + (gci.NONE,) * 3]
    assert got["rows"] == [(G(1), NF, G(1)), (NF,) * 3, (NF,) * 3]


def test_bad_host_records_name_the_first_bad_read(exe, workdir):
    (reads, reports, cigar), npm = _records([PAIRS["mates_in_two_genes"][0]], [SINGLES["all_ops"][0], SINGLES["unmapped_single"][0]])
    def bad(tag, change, want):
        r, p, c = reads.copy(), reports.copy(), cigar.copy()
        r, p, c = change(r, p, c) or (r, p, c)
        assert gci.run_program(exe, workdir, "badrec_" + tag, N_CHR, N_GENES, EXONS, r, p, c, npm, MIN_MAPQ)["bad"] == want
    def f1(r, p, c): r["n_rep"][2] = 3
    def f2(r, p, c): r["best"][1] = 1
    def f3(r, p, c): r["best"][1] = -1
    def f4(r, p, c): p["n_cigar"][2] = 10
    def f5(r, p, c): return r, p, c[:-1]
    def f6(r, p, c): r["rep_off"][0] = -1
    def f7(r, p, c): r["best"][3] = 5                        # an unmapped read's best is not looked at
    bad("n_rep", f1, 2); bad("best", f2, 1); bad("best_neg", f3, 1); bad("n_cigar", f4, 2); bad("short_cigar", f5, 2); bad("rep_off", f6, 0); bad("unmapped_best", f7, None)


def _random_units(rng, lengths, segs, n):
    """units near the annotation's breakpoints, CIGARs of every op, every MAPQ DART gives, some unmapped -> (pairs, singles) of Records.read keyword dicts"""
    def read(c=None, mate=0):
        if rng.random() < 0.05:
            return dict(reports=[])
        c = rng.randrange(-1, len(lengths) + 1) if rng.random() < 0.03 else (rng.randrange(len(lengths)) if c is None else c)
        sg = segs[c] if 0 <= c < len(lengths) else []
        anchor = rng.choice(sg)[0] if sg and rng.random() < 0.8 else rng.randrange(0, 150000)
        pos = max(anchor + rng.choice([-120, -101, -100, -99, -50, -1, 0, 1, 2, 30]), rng.choice([-3, 0, 1]))
        ops = [(rng.choice([0, 1, 2, 25, 50, 100, 101]), rng.choice([M, M, M, M, I, D, N, N, S, EQ, X, H, P, 9])) for _ in range(rng.randrange(1, 6))]
        flag = rng.choice([0, 16] if mate == 0 else [0x41, 0x51] if mate == 1 else [0x81, 0x91])
        reps = [(c, pos, flag, ops, rng.choice([100, 100, 100, 0, 60]))]
        if rng.random() < 0.2:
            reps.insert(rng.randrange(2), (rng.randrange(len(lengths)), rng.randrange(1, 150000), flag, [(50, M)], rng.choice([0, 100, 60])))
        return dict(reports=reps, score=100, mapq=rng.choice([0, 1, 2, 3] + [50] * 28), best=rng.randrange(len(reps)))
    pairs = []
    for _ in range(n * 2 // 3):
        c = rng.randrange(len(lengths))
        pairs.append([read(c, 1), read(c if rng.random() < 0.9 else None, 2)])
    return pairs, [[read()] for _ in range(n - len(pairs))]


def test_random_annotations_random_units_and_a_shuffled_copy(exe, workdir):
    for seed, lengths in ((1, [200000, 100000, 30000]), (2, [150000]), (3, [6000, 180000, 40000, 40000])):
        rng = random.Random(seed)
        n_genes, exons = gci.random_annotation(rng, lengths)
        segs = gci.flatten(len(lengths), exons)
        gci.assert_painter_agrees(len(lengths), n_genes, exons, segs, limit=1 << 18)
        labels = [s[1:] for sg in segs for s in sg]
        assert n_genes > 20 and any(l[0] == gci.AMBIG and l[1] != gci.AMBIG for l in labels) and any(l[1] == gci.AMBIG for l in labels)      # overlaps on opposite strands and on one
        pairs, singles = _random_units(rng, lengths, segs, 3000)
        arrays, npm = _records(pairs, singles)
        got = _check(exe, workdir, "random_%d" % seed, len(lengths), n_genes, exons, arrays, npm)
        prof = gci.outcome_profile(got["counts"])
        assert all(min(p) >= 10 for p in prof), prof                                       # every outcome, in every column
        assert len({r for r in got["rows"] if len(set(r)) == 3}) > 5                         # units whose three columns differ
        rng.shuffle(pairs); rng.shuffle(singles)
        again, npm2 = _records(pairs, singles)
        assert npm2 == npm and not np.array_equal(again[0], arrays[0])
        assert np.array_equal(_check(exe, workdir, "random_%d_shuffled" % seed, len(lengths), n_genes, exons, again, npm)["counts"], got["counts"])


def test_lane_code_under_the_sanitizers(workdir):
    """the same program with AddressSanitizer and UBSan on its host code: the record arrays and the segment table are exact-size heap copies, so a walk that
    leaves one leaves its allocation.  Stand-alone; never through python's process, never on the GPU."""
    exe = gci.build_program(workdir, sanitize=True)
    arrays, npm = _records([PAIRS[k][0] for k in sorted(PAIRS)], [SINGLES[k][0] for k in sorted(SINGLES)])
    for tag, n_genes, exons in (("full", N_GENES, EXONS), ("one", 1, [(3, 0, (1 << 32) - 1, 1, 0)]), ("none", 2, [])):
        _check(exe, workdir, "san_" + tag, N_CHR, n_genes, exons, arrays, npm)
        _check(exe, workdir, "san_alone_" + tag, N_CHR, n_genes, exons, arrays, 0)
    rng = random.Random(9)
    lengths = [50000, 8000]
    n_genes, exons = gci.random_annotation(rng, lengths)
    pairs, singles = _random_units(rng, lengths, gci.flatten(2, exons), 1500)
    arrays, npm = _records(pairs, singles)
    _check(exe, workdir, "san_random", 2, n_genes, exons, arrays, npm)
    # records whose ranges leave the arrays are refused before any lane code reads them
    reads, reports, cigar = arrays
    r = reads.copy(); r["n_rep"][len(r) - 1] += 1
    assert gci.run_program(exe, workdir, "san_bad", 2, n_genes, exons, r, reports, cigar, npm, MIN_MAPQ)["bad"] == len(r) - 1
    assert gci.run_program(exe, workdir, "san_badexon", 2, n_genes, [(0, 5, 4, 0, 0)], reads, reports, cigar, npm, MIN_MAPQ)["err"].startswith("exon 0 ")
