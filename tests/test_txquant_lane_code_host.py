"""CPU suite: the host-callable code of the device's expression stage (dart_amd/csrc/dg_txquant.h) through tests/native/txquant_checks.hip -- the flattening,
every unit's lane code in both passes, the class building with and without colliding hashes, the EM's rounds, the text -- against the sequential Python twin of
tests/txquant_inputs.py, and the twin's compatibility against a per-base painter.  The definition is the header's comment; no quantification tool is run."""
import random
import numpy as np
import pytest
import txquant_inputs as txi
from txquant_inputs import M, I, D, N, S, H, P, EQ, X, UNMAPPED, MULTI, INCOMPAT, COUNTED, F

MIN_MAPQ = 4
N_CHR = 4
TOP = (1 << 32) - 1

# ---- the crafted annotation: four chromosomes, chromosome 2 without transcripts ----
# one locus of three exons [1000, 1100) [1200, 1300) [1400, 1500): FULL, SKIP (without the middle exon), RETAIN (the first intron retained), on the plus strand
FULL, SKIP, RETAIN, MINUS, TOUCH, OVERLAP, LASTCHR, ATZERO, ATTOP, MINUS2 = range(10)
FAN0 = 10                                                   # 300 isoforms that share the first exon [5000, 5050) on chromosome 1
TRANSCRIPTS = [
    (0, 0, [(1200, 1300), (1000, 1100), (1400, 1500)]),     # FULL (its exons out of order)
    (0, 0, [(1000, 1100), (1400, 1500)]),                   # SKIP
    (0, 0, [(1000, 1300), (1400, 1500)]),                   # RETAIN
    (0, 1, [(1000, 1100), (1200, 1300), (1400, 1500)]),     # MINUS: FULL's exons on the other strand
    (0, 0, [(3000, 3050), (3050, 3100), (3200, 3300)]),     # TOUCH: two touching exons are one
    (0, 0, [(4000, 4060), (4040, 4100), (4040, 4050), (4200, 4300)]),      # OVERLAP: overlapping and nested exons are one
    (3, 0, [(100, 200)]),                                   # LASTCHR
    (1, 0, [(0, 50)]),                                      # ATZERO
    (1, 1, [(TOP - 100, TOP - 40), (TOP - 20, TOP)]),       # ATTOP: the last coordinates there are
    (0, 1, [(1250, 1300), (1400, 1450)]),                   # MINUS2: inside MINUS's exons, on its strand
] + txi.fan(300, chrom=1, at=5000)
N_TX = len(TRANSCRIPTS)


def _cases():
    """name -> (reads of the unit as Records.read keyword dicts, the outcome and the set the unit is there for under strand_mode 0)"""
    fwd = lambda c, pos, ops, **kw: dict(reports=[(c, pos, 0, ops)], **kw)
    rev = lambda c, pos, ops, **kw: dict(reports=[(c, pos, 0x10, ops)], **kw)
    m1 = lambda c, pos, ops, flag=0x61, **kw: dict(reports=[(c, pos, flag, ops)], **kw)
    m2 = lambda c, pos, ops, flag=0x91, **kw: dict(reports=[(c, pos, flag, ops)], **kw)
    un = dict(reports=[])
    ok = lambda *ids: (COUNTED, tuple(sorted(ids)))
    no = (INCOMPAT, ())
    all4 = ok(FULL, SKIP, RETAIN, MINUS)
    singles = {
        "piece_ends_one_before_the_exon_end": ([fwd(0, 1050, [(50, M)])], all4),                       # [1049, 1099)
        "piece_ends_on_the_exon_end": ([fwd(0, 1051, [(50, M)])], all4),                               # [1050, 1100)
        "piece_ends_one_behind_the_exon_end": ([fwd(0, 1052, [(50, M)])], ok(RETAIN)),                 # [1051, 1101): only the retained intron holds 1100
        "piece_starts_on_the_exon_start": ([fwd(0, 1001, [(20, M)])], all4),
        "piece_starts_one_in_front": ([fwd(0, 1000, [(20, M)])], no),
        "junction_on_the_intron": ([fwd(0, 1081, [(20, M), (100, N), (20, M)])], ok(FULL, MINUS)),     # [1080, 1100) N [1200, 1220)
        "junction_one_base_early": ([fwd(0, 1080, [(20, M), (100, N), (20, M)])], no),                # ends at 1099
        "junction_one_base_late": ([fwd(0, 1082, [(20, M), (100, N), (20, M)])], no),                 # ends at 1101
        "junction_lands_one_base_early": ([fwd(0, 1081, [(20, M), (99, N), (20, M)])], no),
        "junction_lands_one_base_late": ([fwd(0, 1081, [(20, M), (101, N), (20, M)])], no),
        "skips_an_exon": ([fwd(0, 1081, [(20, M), (300, N), (20, M)])], ok(SKIP)),                     # [1080, 1100) N [1400, 1420): SKIP's intron, two of FULL's
        "three_exons": ([fwd(0, 1091, [(10, M), (100, N), (100, M), (100, N), (10, M)])], ok(FULL, MINUS)),
        "retained_intron": ([fwd(0, 1091, [(120, M)])], ok(RETAIN)),                                   # [1090, 1210)
        "retained_then_spliced": ([fwd(0, 1091, [(210, M), (100, N), (10, M)])], ok(RETAIN)),
        "second_intron_of_all": ([fwd(0, 1291, [(10, M), (100, N), (10, M)])], ok(FULL, RETAIN, MINUS, MINUS2)),
        "d_inside_an_exon": ([fwd(0, 1011, [(10, M), (5, D), (10, M)])], all4),
        "d_across_an_intron": ([fwd(0, 1091, [(10, M), (100, D), (10, M)])], ok(RETAIN)),              # the D's bases belong to the piece: only RETAIN has them
        "i_s_h_p_change_nothing": ([fwd(0, 1081, [(3, H), (4, S), (10, M), (7, I), (2, P), (10, M), (100, N), (20, M), (5, S)])], ok(FULL, MINUS)),
        "eq_and_x_are_blocks": ([fwd(0, 1081, [(10, EQ), (10, X), (100, N), (20, EQ)])], ok(FULL, MINUS)),
        "zero_length_ops": ([fwd(0, 1081, [(0, M), (0, I), (0, D), (20, M), (0, S), (100, N), (0, M), (20, M)])], ok(FULL, MINUS)),
        "zero_length_n_ends_a_piece": ([fwd(0, 1011, [(10, M), (0, N), (10, M)])], no),                # two pieces that touch: no intron lies between them
        "leading_and_trailing_n": ([fwd(0, 981, [(20, N), (20, M), (30, N)])], all4),                  # they end no piece and begin none
        "two_n_make_one_gap": ([fwd(0, 1081, [(20, M), (60, N), (40, N), (20, M)])], ok(FULL, MINUS)),
        "only_zero_length_blocks": ([fwd(0, 1011, [(0, M), (5, S)])], no),
        "no_ops": ([fwd(0, 1011, [])], no),
        "touching_exons_are_one": ([fwd(0, 3041, [(20, M)])], ok(TOUCH)),                              # [3040, 3060) over the seam at 3050
        "overlapping_exons_are_one": ([fwd(0, 4031, [(60, M)])], ok(OVERLAP)),                         # [4030, 4090)
        "merged_exon_to_the_next": ([fwd(0, 4091, [(10, M), (100, N), (10, M)])], ok(OVERLAP)),
        "intergenic": ([fwd(0, 2001, [(50, M)])], no),
        "in_front_of_the_first_segment": ([fwd(0, 5, [(50, M)])], no),
        "behind_the_last_segment": ([fwd(0, 200001, [(50, M)])], no),
        "chromosome_without_transcripts": ([fwd(2, 1001, [(50, M)])], no),
        "last_chromosome": ([fwd(3, 151, [(20, M)])], ok(LASTCHR)),
        "chromosome_behind_the_last": ([fwd(4, 151, [(20, M)])], no),
        "chromosome_minus_one": ([fwd(-1, 151, [(20, M)])], no),
        "pos_zero": ([fwd(1, 0, [(20, M)])], no),
        "pos_one": ([fwd(1, 1, [(20, M)])], ok(ATZERO)),
        "pos_negative": ([fwd(1, -5, [(20, M)])], no),
        "at_the_top": ([fwd(1, TOP - 49, [(10, M), (20, N), (20, M)])], ok(ATTOP)),                    # [2^32 - 51, 2^32 - 41) N [2^32 - 21, 2^32 - 1)
        "over_the_top": ([fwd(1, TOP - 49, [(10, M), (20, N), (21, M)])], no),
        "far_over_the_top": ([fwd(1, TOP + 5, [(10, M)])], no),
        "fan_first_exon": ([fwd(1, 5011, [(30, M)])], ok(*range(FAN0, FAN0 + 300))),                   # a list of 300
        "fan_one_isoform": ([fwd(1, 5041, [(10, M), (100 + 30 * 7 - 50, N), (10, M)])], ok(FAN0 + 7)),
        "reverse_read": ([rev(0, 1011, [(20, M)])], all4),
        "unaligned": ([un], (UNMAPPED, ())),
        "low_mapq": ([fwd(0, 1011, [(20, M)], mapq=3)], (MULTI, ())),
        "mapq_on_the_bound": ([fwd(0, 1011, [(20, M)], mapq=4)], all4),
        "second_report_is_the_alignment": ([dict(reports=[(0, 2001, 0, [(20, M)], 50), (0, 1011, 0, [(20, M)], 100)], best=1)], all4),
    }
    pairs = {
        "mates_intersect_to_one": ([m1(0, 1081, [(20, M), (100, N), (20, M)]), m2(0, 1451, [(20, M)])], ok(FULL, MINUS)),
        "mates_intersect_to_one_isoform": ([m1(0, 1081, [(20, M), (300, N), (20, M)]), m2(0, 1451, [(20, M)])], ok(SKIP)),
        "mates_intersect_to_several": ([m1(0, 1011, [(20, M)]), m2(0, 1451, [(20, M)])], all4),
        "mates_intersect_to_none": ([m1(0, 1081, [(20, M), (300, N), (20, M)]), m2(0, 1211, [(20, M)])], no),      # SKIP alone, and everything but SKIP
        "one_mate_unaligned": ([m1(0, 1091, [(120, M)]), un], ok(RETAIN)),
        "first_mate_unaligned": ([un, m2(0, 1091, [(120, M)])], ok(RETAIN)),
        "both_unaligned": ([un, un], (UNMAPPED, ())),
        "mates_on_two_chromosomes": ([m1(0, 1011, [(20, M)]), m2(3, 151, [(20, M)])], no),
        "one_mate_low_mapq": ([m1(0, 1011, [(20, M)]), m2(0, 1451, [(20, M)], mapq=0)], (MULTI, ())),
        "unaligned_mate_low_mapq_does_not_count": ([m1(0, 1011, [(20, M)]), dict(reports=[], mapq=0)], all4),
        "one_mate_without_blocks": ([m1(0, 1011, [(20, M)]), m2(0, 1451, [(20, S)])], no),
        "forward_second_mate": ([m1(0, 1261, [(20, M)], flag=0x51), m2(0, 1411, [(20, M)], flag=0xA1)], ok(FULL, RETAIN, MINUS, MINUS2)),
        "mates_on_the_fan": ([m1(1, 5011, [(30, M)]), m2(1, 5000 + 100 + 30 * 299 + 1, [(19, M)])], ok(FAN0 + 299)),
    }
    return singles, pairs


SINGLES, PAIRS = _cases()


def _records(pairs, singles):
    rec = txi.Records()
    for unit in pairs:
        assert len(unit) == 2
        for kw in unit:
            kw = dict(kw)
            if not kw.get("reports") and "mapq" in kw:
                kw.pop("mapq")
            rec.read(**kw)
    for unit in singles:
        for kw in unit:
            rec.read(**kw)
    return rec.arrays(), 2 * len(pairs)


def _check(exe, workdir, tag, n_chr, transcripts, arrays, npm, strand_mode=0, hash_bits=64, painted=True, **kw):
    """the program against the twin: lengths, segments, units, classes, words, the EM's words and the text"""
    reads, reports, cigar = arrays
    got = txi.run_program(exe, workdir, tag, n_chr, transcripts, reads, reports, cigar, npm, MIN_MAPQ, strand_mode, hash_bits, **kw)
    assert got["err"] is None and got["bad"] is None
    L = txi.lengths(transcripts)
    assert got["L"] == L and got["n_ex"] == [len(txi.merged(ex)) for _, _, ex in transcripts]
    assert got["segs"] == txi.segments_twin(transcripts, n_chr)
    classes, words, units = txi.twin(transcripts, n_chr, reads, reports, cigar, npm, MIN_MAPQ, strand_mode, check_painted=painted, want_units=True)
    assert got["units"] == units, [(u, a, b) for u, (a, b) in enumerate(zip(got["units"], units)) if a != b][:5]
    assert got["classes"] == classes and got["words"] == words
    assert got["collision"] == 0 or hash_bits < 64
    res = txi.em(classes, words, L, kw.get("frag_mean", 200), kw.get("max_rounds", 1000), strand_mode)
    assert got["res"] == res, [(t, a, b) for t, (a, b) in enumerate(zip(got["res"], res)) if a != b][:5]
    assert got["text"] == txi.text(res, L, ["T%d" % t for t in range(len(L))])
    return got, units


@pytest.fixture(scope="module")
def exe(workdir):
    return txi.build_program(workdir)


def test_crafted_units_are_what_they_are_named_for(exe, workdir):
    names_p, names_s = sorted(PAIRS), sorted(SINGLES)
    arrays, npm = _records([PAIRS[k][0] for k in names_p], [SINGLES[k][0] for k in names_s])
    got, units = _check(exe, workdir, "crafted", N_CHR, TRANSCRIPTS, arrays, npm)
    for name, (o, ids, fl) in zip(names_p + names_s, units):
        want = (PAIRS if name in PAIRS else SINGLES)[name][1]
        assert (o, ids) == want, name
    by = dict(zip(names_p + names_s, units))
    # fragment lengths on the smallest id of the set: FULL's offsets; SKIP's for the pair that only SKIP holds; the fan's last isoform
    assert by["mates_intersect_to_one"][2] == (100 + 100 + 70) - 80 and by["mates_intersect_to_one_isoform"][2] == (100 + 70) - 80
    assert by["mates_on_the_fan"][2] == (50 + 19) - 10 and by["one_mate_unaligned"][2] is None and by["forward_second_mate"][2] == (200 + 30) - 160
    assert got["words"][6] == sum(1 for n in names_p if by[n][2] is not None)
    # the same units alone (no pair mode): every read a unit
    _check(exe, workdir, "crafted_alone", N_CHR, TRANSCRIPTS, arrays, 0)


@pytest.mark.parametrize("mode", [1, 2])
def test_strand_modes(exe, workdir, mode):
    names_p, names_s = sorted(PAIRS), sorted(SINGLES)
    arrays, npm = _records([PAIRS[k][0] for k in names_p], [SINGLES[k][0] for k in names_s])
    got, units = _check(exe, workdir, "strand%d" % mode, N_CHR, TRANSCRIPTS, arrays, npm, strand_mode=mode)
    by = dict(zip(names_p + names_s, units))
    plus, minus = (COUNTED, (FULL, SKIP, RETAIN)), (COUNTED, (MINUS,))
    assert by["piece_ends_on_the_exon_end"][:2] == (plus if mode == 1 else minus)                    # a forward read: s = 0
    assert by["reverse_read"][:2] == (minus if mode == 1 else plus)
    # first mate forward (s = 0), second mate reverse (0x91: s = 1 ^ 1 = 0): both count for the plus strand
    assert by["mates_intersect_to_several"][:2] == (plus if mode == 1 else minus)
    # a reverse first mate and a forward second mate: s = 1 for both
    assert by["forward_second_mate"][:2] == ((COUNTED, (MINUS, MINUS2)) if mode == 1 else (COUNTED, (FULL, RETAIN)))
    assert got["res"][N_TX + 13] == mode


def test_shuffled_units_and_colliding_hashes_give_the_same_table(exe, workdir):
    names_s = sorted(SINGLES)
    units = [SINGLES[k][0] for k in names_s] * 3
    a1, _ = _records([], units)
    random.Random(4).shuffle(units)
    a2, _ = _records([], units)
    g1, _ = _check(exe, workdir, "order1", N_CHR, TRANSCRIPTS, a1, 0, painted=False)
    g2, _ = _check(exe, workdir, "order2", N_CHR, TRANSCRIPTS, a2, 0, painted=False)
    assert g1["classes"] == g2["classes"] and g1["words"] == g2["words"] and g1["res"] == g2["res"] and g1["collision"] == 0
    for bits in (1, 2, 4):
        g3, _ = _check(exe, workdir, "bits%d" % bits, N_CHR, TRANSCRIPTS, a2, 0, hash_bits=bits, painted=False)
        assert g3["collision"] == 1 and g3["classes"] == g1["classes"] and g3["res"] == g1["res"]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_annotations_and_units_against_the_twin(exe, workdir, seed):
    rng = random.Random(seed)
    lengths = [6000, 3000]
    transcripts = txi.random_annotation(rng, lengths)
    rd, rp, cg, npm = txi.random_units(rng, transcripts, 2, 700)
    for mode in (0, 1, 2):
        got, units = _check(exe, workdir, "random%d_%d" % (seed, mode), 2, transcripts, (rd, rp, cg), npm, strand_mode=mode, max_rounds=40)
    outcomes = [u[0] for u in units]
    assert all(outcomes.count(o) >= 10 for o in range(4)), [outcomes.count(o) for o in range(4)]
    _check(exe, workdir, "random%d_bits" % seed, 2, transcripts, (rd, rp, cg), npm, hash_bits=3, max_rounds=0, painted=False)


# ---- the EM ----
def _em_input():
    """two isoforms A and B of one length that share their first exon, a class of both and a class of A alone; a third transcript with no reads"""
    tr = [(0, 0, [(1000, 1300), (1400, 1700)]), (0, 0, [(1000, 1300), (2000, 2300)]), (0, 0, [(5000, 5400)])]
    rec = txi.Records()
    for k in range(60):
        rec.read(reports=[(0, 1011 + k, 0, [(50, M)])])            # in both
    for k in range(20):
        rec.read(reports=[(0, 1411 + k, 0, [(50, M)])])            # in A alone
    return tr, rec.arrays()


@pytest.mark.parametrize("rounds", [0, 1, 15, 16, 17, 1000])
def test_em_rounds_against_the_twin_as_words(exe, workdir, rounds):
    tr, arrays = _em_input()
    got, _ = _check(exe, workdir, "em%d" % rounds, 1, tr, arrays, 0, max_rounds=rounds)
    res = got["res"]
    assert res[3 + 8] == min(rounds, 16) and res[3 + 7] == 2 and res[2] == 0      # conv_16 holds on this input: the shared class's mass shrinks by a quarter a round on B
    if rounds == 0:
        assert res[0] == res[1] == 80 * F // 2 and res[3 + 9] == 0
    if rounds == 1000:
        assert res[3 + 9] == 1
    if rounds == 15:
        assert res[3 + 9] == 0 or res[1] < F                      # `converged` is conv_r of the last round, whatever r is


def test_the_shared_class_moves_to_the_isoform_with_unique_reads(exe, workdir):
    tr, (rd, rp, cg) = _em_input()
    classes, words = txi.twin(tr, 1, rd, rp, cg, 0, MIN_MAPQ)
    assert classes == {(0, 1): 60, (0,): 20}
    L = txi.lengths(tr)
    res, trace = txi.em(classes, words, L, 200, 64, want_trace=True)
    a = [s[0] for s in trace]
    assert all(x < y for x, y in zip(a, a[1:6])) and a[0] > 40 * F and trace[-1][0] + trace[-1][1] <= 80 * F and trace[-1][0] + trace[-1][1] > 80 * F - 64 * 3
    assert trace[-1][0] > 70 * F                                   # A's unique reads pull the shared class over
    # the native rounds, one more at a time, walk the same way
    for r in (1, 2, 3, 5):
        got = txi.run_program(exe, workdir, "move%d" % r, 1, tr, rd, rp, cg, 0, max_rounds=r)
        assert got["res"][:3] == trace[r - 1] and got["res"][3 + 8] == r


def test_a_class_whose_members_are_all_zero_gives_nothing(exe, workdir):
    """D == 0.0 is out of the start values' reach (every listed transcript begins above zero and a class's largest member keeps a share), so the native program,
    as the twin, takes the S to begin from: the branch runs in the code the kernels share."""
    tr = [(0, 0, [(1000, 1500)]), (0, 0, [(3000, 3500)]), (0, 0, [(3000, 3500)])]
    rec = txi.Records()
    for k in range(10):
        rec.read(reports=[(0, 1011 + k, 0, [(50, M)])])            # in 0 alone
    for k in range(5):
        rec.read(reports=[(0, 3011 + k, 0, [(50, M)])])            # in 1 and 2
    rd, rp, cg = rec.arrays()
    classes, words = txi.twin(tr, 1, rd, rp, cg, 0, MIN_MAPQ)
    assert classes == {(0,): 10, (1, 2): 5}
    L = txi.lengths(tr)
    start = [10 * F, 0, 0]
    res, trace = txi.em(classes, words, L, 200, 3, want_trace=True, start=start)
    assert all(s == start for s in trace)                          # D == 0.0: the class's five units go nowhere, and nothing divides by zero
    got = txi.run_program(exe, workdir, "zero", 1, tr, rd, rp, cg, 0, max_rounds=3, start=start)
    assert got["classes"] == classes and got["res"] == res and got["res"][:3] == start and got["res"][3 + 8] == 3
    # a start in which one member of the shared class holds something: all five units go to it
    start = [10 * F, 0, 7]
    got = txi.run_program(exe, workdir, "zero1", 1, tr, rd, rp, cg, 0, max_rounds=1, start=start)
    assert got["res"] == txi.em(classes, words, L, 200, 1, start=start) and got["res"][:3] == [10 * F, 0, 5 * F]
    # from the definition's start values the class's units are shared out
    got = txi.run_program(exe, workdir, "zero2", 1, tr, rd, rp, cg, 0, max_rounds=1)
    assert got["res"] == txi.em(classes, words, L, 200, 1) and got["res"][0] == 10 * F and got["res"][1] + got["res"][2] == 5 * F


def test_no_active_transcript_and_the_range(exe, workdir):
    tr, (rd, rp, cg) = _em_input()
    rec = txi.Records()
    rec.read(); rec.read(reports=[(0, 3001, 0, [(50, M)])])
    got, _ = _check(exe, workdir, "m0", 1, tr, rec.arrays(), 0)
    res = got["res"]
    assert res[:3] == [0, 0, 0] and res[3 + 7] == 0 and res[3 + 8] == 0 and res[3 + 9] == 1 and res[3 + 5] == 0
    assert b"\t0.000\t0.000\n" in got["text"]                      # R = 0: every tpm is 0
    # N = 2^33 is refused, one below it is not
    one = txi.Records(); one.read(reports=[(0, 1011, 0, [(50, M)])])
    r = txi.run_program(exe, workdir, "n33", 1, tr, *one.arrays(), 0, scale=1 << 33, max_rounds=1)
    assert r["range"] and r["res"] is None
    r = txi.run_program(exe, workdir, "n33m", 1, tr, *one.arrays(), 0, scale=(1 << 33) - 1, max_rounds=17)
    classes = {(0, 1): (1 << 33) - 1}
    assert not r["range"] and r["res"] == txi.em(classes, [1, 0, 0, 0, 1, 0, 0, 0], txi.lengths(tr), 200, 17)[:3] + r["res"][3:]


def test_bad_annotations_and_records_are_refused(exe, workdir):
    tr, (rd, rp, cg) = _em_input()
    r = txi.run_program(exe, workdir, "badtx", 1, [(0, 0, [(10, 20)]), (0, 2, [(10, 20)])], rd, rp, cg, 0)
    assert r["err"].startswith("transcript 1 ") and "strand" in r["err"]
    r = txi.run_program(exe, workdir, "badex", 1, [(0, 0, [(10, 20), (30, 30)])], rd, rp, cg, 0)
    assert r["err"].startswith("transcript 0 ") and "start < end" in r["err"]
    r = txi.run_program(exe, workdir, "badchr", 1, [(1, 0, [(10, 20)])], rd, rp, cg, 0)
    assert r["err"].startswith("transcript 0 ") and "chromosome" in r["err"]
    bad = rd.copy(); bad["n_rep"][len(bad) - 1] += 1
    assert txi.run_program(exe, workdir, "badread", 1, tr, bad, rp, cg, 0)["bad"] == len(bad) - 1


def test_lane_code_under_the_sanitizers(workdir):
    """the same program with AddressSanitizer and UBSan on its host code: the record arrays and the annotation's tables are exact-size heap copies, so a walk
    that leaves one leaves its allocation.  Stand-alone; never through python's process, never on the GPU."""
    exe = txi.build_program(workdir, sanitize=True)
    arrays, npm = _records([PAIRS[k][0] for k in sorted(PAIRS)], [SINGLES[k][0] for k in sorted(SINGLES)])
    _check(exe, workdir, "san_crafted", N_CHR, TRANSCRIPTS, arrays, npm, painted=False, max_rounds=20)
    _check(exe, workdir, "san_crafted_bits", N_CHR, TRANSCRIPTS, arrays, 0, hash_bits=2, strand_mode=1, painted=False, max_rounds=3)
    rng = random.Random(9)
    transcripts = txi.random_annotation(rng, [6000, 3000])
    rd, rp, cg, npm = txi.random_units(rng, transcripts, 2, 500)
    _check(exe, workdir, "san_random", 2, transcripts, (rd, rp, cg), npm, painted=False, max_rounds=20)
