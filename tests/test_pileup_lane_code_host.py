"""CPU suite: the host-callable code of the device's allele counts (dart_amd/csrc/dg_pileup.h) through tests/native/pileup_checks.hip -- a record's filter and
walk, the sorted events, the distinct allele keys, the sites, the entries and the text's bytes -- against the sequential Python twin of tests/pileup_inputs.py,
and the twin against one row of counters per position.  The table is the definition in the header's comment; no pileup tool is run."""
import random
import pytest
import pileup_inputs as pui
from pileup_inputs import A_, C_, G_, T_, N_, DEL, INS

CASES = pui.crafted_cases()
REF = pui.REF
STATE = {"skip": 0, "counted": 1, "left_out": 2, "range": 3}


@pytest.fixture(scope="module")
def exe(workdir):
    return pui.build_program(workdir)


def _twin_events(raw, ref, flt):
    recs, ev = [], []
    for at in pui.offsets(raw):
        c = pui.classify(raw, at, ref, flt[0], flt[1])
        n = 0
        if c[0] == "counted":
            _, refid, pos, s, cigar, nib = c
            blocks, alleles = pui.observations(ref, refid, pos, s, cigar, nib)
            v = 1 + (s << 32)
            for b, e in blocks:
                ev += [(refid << 35 | b << 3, v), (refid << 35 | e << 3, -v)]
            ev += [(refid << 35 | p << 3 | a + 1, v) for p, a in alleles]
            n = 2 * len(blocks) + len(alleles)
        recs.append((STATE[c[0]], n))
    return recs, ev


def _check(exe, workdir, tag, recs, names, flt, ref=REF):
    raw = b"".join(recs)
    got = pui.run_program(exe, workdir, tag, ref, raw, names, *flt)
    entries, stats = pui.twin(raw, ref, *flt)
    t_recs, t_events = _twin_events(raw, ref, flt)
    assert got["bad"] is None and got["recs"] == t_recs
    assert [k for k, _ in got["events"]] == sorted(k for k, _ in t_events) and sorted(got["events"]) == sorted(t_events)      # (equal keys: the order of their values is the input's)
    sums = {}
    for k, v in t_events:
        if k & 7:
            sums[k] = sums.get(k, 0) + v
    assert [(k, n) for k, n, _ in got["keys"]] == sorted(sums.items())
    assert got["entries"] == entries and got["stats"] == stats
    assert [e for e in got["sites"] if e[6 + e[5]] >= flt[2]] == entries and len(got["sites"]) == stats[6]
    assert got["text"] == pui.text_of(entries, names)
    assert pui.brute(raw, ref, *flt) == entries
    return entries, stats


@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "ends_bad"))
def test_lane_code_equals_the_twin_on_the_crafted_records(name, exe, workdir):
    recs, names = CASES[name]
    for k, flt in enumerate(pui.FILTERS):
        _check(exe, workdir, "%s_%d" % (name, k), recs, names, flt)


def test_what_the_crafted_records_are_there_for(exe, workdir):
    one = pui.FILTERS[1]                                                          # min_alt 1: every site
    run = lambda name, flt=one: _check(exe, workdir, name + "_again", *CASES[name], flt)
    site = lambda e, c, p: next(x for x in e if x[:2] == (c, p))
    n = lambda x, a: x[6 + a]
    n_rev = lambda x, a: x[13 + a]
    e, st = run("ops")
    # all nine ops, on both strands: S and H and P move nothing on the reference; the mismatch at read base 7 is reference 102; the I's anchor is 109, the D covers
    # 110..112, the N is no observation, the last = base (read 20) is 816, the X base matches
    x = site(e, 0, 102); assert x[2:4] == (2, 1) and n(x, x[5]) == 2 and n_rev(x, x[5]) == 1
    x = site(e, 0, 109); assert n(x, INS) == 2 and n_rev(x, INS) == 1 and x[2] == 2
    assert [n(site(e, 0, p), DEL) for p in (110, 111, 112)] == [2, 2, 2] and site(e, 0, 110)[2] == 0          # deleted bases lie outside the depth
    assert not any(x[0] == 0 and 113 <= x[1] < 300 for x in e) and not any(x[0] == 0 and 1221 <= x[1] for x in e)         # nothing inside the N gap (813 .. 817 lie behind it)
    x = site(e, 0, 816); assert x[5] < 4 and n(x, x[5]) == 2 and not any(x[:2] == (0, 817) for x in e)
    assert site(e, 0, 300)[2] == 2 and not any(x[:2] == (0, 1210) for x in e)                                  # a zero-length M is no block; zero-length I and D observe nothing
    assert n(site(e, 0, 400), INS) == 2 and n(site(e, 0, 469), INS) == 2                                       # I at the read's start: anchored at its first position; at its end: the last base
    x = site(e, 0, 511); assert n(x, INS) == 2 and n(x, DEL) == 2 and x[5] == DEL                               # I behind a D: anchored on the last deleted base; ties go to the smaller code
    assert n(site(e, 0, 600), site(e, 0, 600)[5]) == 2 and n(site(e, 0, 619), site(e, 0, 619)[5]) == 2          # S and H at both ends: the first and last aligned base
    x = site(e, 0, 1012); assert n(x, DEL) == 2 and x[2:4] == (1, 1) and x[5] == DEL and sorted(x[6:11]) == [0, 0, 0, 0, 1] and n(x, x[4]) == 0         # a D under a second read, which has a mismatch there
    assert st[4] == 2 * 3 + 2 * 2 + 2 * 5 and st[5] == 2 + 2 + 2 + 2
    assert {x[1] for x in e if x[0] == 0 and 1100 <= x[1] < 1200} == {1109, 1160}                              # an N gap: the base in front of it and the first behind it
    e, st = run("bases")
    assert n(site(e, 0, 130), site(e, 0, 130)[5]) == 2 and n(site(e, 0, 229), site(e, 0, 229)[5]) == 2          # the last base of an odd-length and of an even-length read
    x = site(e, 0, 305); assert n(x, N_) == 2 and x[5] == N_                                                    # nibble 15
    x = site(e, 0, 308); assert n(x, N_) == 2                                                                   # IUPAC codes count as N
    assert not any(x[:2] == (0, 302) for x in e) and site(e, 0, 305)[2] == 3                                    # '=' is the reference base: never an event; it counts for the depth
    assert site(e, 0, 404)[6 + site(e, 0, 404)[5]] == 2 and len([x for x in e if x[0] == 0 and 400 <= x[1] < 410]) == 1      # the op letter plays no part
    e, st = run("seams")
    for start in range(4):
        for k in range(17):
            assert any(x[:2] == (0, 1000 + start + k) for x in e) and any(x[:2] == (0, 1000 + start + 39 - k) for x in e)
    assert st[3] == 4 * 17 * 2 + 8 * 13
    e, st = run("ends")
    assert site(e, 0, 0)[2] == 2 and n(site(e, 0, 0), INS) == 1                                                 # pos 0; an I in front of everything at pos 0
    x = site(e, 0, 2999); assert x[2] == 2 and n(x, x[5]) == 2                                                  # the last base of chromosome 0
    x = site(e, 1, 0); assert x[2] == 2 and n(x, x[5]) == 2                                                     # and the first of chromosome 1: the text's neighbour, another key
    assert n(site(e, 0, 2980), N_) == 1 and site(e, 1, 1999)[2] == 2
    assert st[8] == 2 + 2 + 1 and st[0] == 8                          # one base past the chromosome, a D past it, l_seq one short and one long, the block that ends at 2^32 - 1; l_seq 0 is no tally
    assert not any(x[:2] == (0, 2984) for x in e)
    e, st = run("nothing")
    assert [x[:2] for x in e] == [(0, 201)] and st[0] == 1 and st[8] == 0
    assert run("nothing_liar")[0] == e
    sites = lambda flt: {(x[0], x[1]): x for x in run("filters", flt)[0]}
    assert sites((4, 0, 1))[0, 105][2:4] == (5, 0) and sites(one)[0, 105][2] == 2 and sites((0x100 | 4, 0, 1))[0, 105][2] == 4 and sites((pui.DEFAULT_EXCLUDE, 10, 1))[0, 105][2] == 1
    assert sites(one)[1, 105][2:4] == (3, 1)                                                                    # the read's orientation: a reverse second mate is a reverse read
    for min_alt, want in ((1, {105, 125, 145}), (2, {125, 145}), (3, {145}), (4, set())):                       # the threshold, one either side
        assert {x[1] for x in run("min_alt", (pui.DEFAULT_EXCLUDE, 0, min_alt))[0]} == want
    e, st = run("ties")
    x = site(e, 0, 505); assert n(x, x[5]) == 2 and x[5] == min(a for a in range(4) if a != x[4])                # two alleles with two each: the smaller code
    assert site(e, 0, 605)[5] == N_ and n(site(e, 0, 605), DEL) == 2                                            # N and DEL tie: N
    assert site(e, 0, 704)[5] == DEL and n(site(e, 0, 704), INS) == 3                                           # DEL and INS tie: DEL
    assert run("empty") == ([], (0,) * 10)


def test_a_block_behind_2_32_is_refused_with_the_records_index(exe, workdir):
    recs, names = CASES["ends_bad"]
    raw = b"".join(recs)
    k = [r[36:36 + r[12] - 1] for r in recs].index(b"ends_at_2_32")
    got = pui.run_program(exe, workdir, "ends_bad", REF, raw, names)
    assert got["bad"] == k and got["text"] == b"" and not got["entries"]
    with pytest.raises(pui.RangeError) as x:
        pui.twin(raw, REF)
    assert x.value.args[0] == k
    # a record the filter drops is never out of range: the duplicate is, once duplicates count
    d = [r[36:36 + r[12] - 1] for r in recs].index(b"a_duplicate_out_of_range")
    got = pui.run_program(exe, workdir, "ends_bad_dups", REF, raw, names, exclude=4)
    assert got["bad"] == d < k
    with pytest.raises(pui.RangeError) as x:
        pui.twin(raw, REF, exclude=4)
    assert x.value.args[0] == d


def test_random_records_and_a_shuffled_copy(exe, workdir):
    ref = pui.random_ref(3, [1700, 1601, 1602])
    names = [b"c0", b"chr_one", b"2"]
    rng = random.Random(17)
    recs = pui.random_records(rng, 2500, ref)
    for k, flt in enumerate((pui.FILTERS[0], pui.FILTERS[2], pui.FILTERS[4])):
        entries, stats = _check(exe, workdir, "random_%d" % k, recs, names, flt, ref)
        assert stats[7] > 200 and stats[8] > 10 and stats[9] >= 10 and stats[4] > 100 and stats[5] > 100
    shuffled = list(recs); rng.shuffle(shuffled)
    assert shuffled != recs
    assert pui.twin(b"".join(shuffled), ref) == pui.twin(b"".join(recs), ref)
    got = pui.run_program(exe, workdir, "random_shuffled", ref, b"".join(shuffled), names)
    assert got["entries"] == pui.twin(b"".join(recs), ref)[0] and got["text"] == pui.text_of(got["entries"], names)


def test_lane_code_under_the_sanitizers(workdir):
    """the same program with AddressSanitizer and UBSan on its host code: every record walk stays inside the exact-size heap copy of the array, every fetch of the
    text inside the exact-size pac, every event, entry and line inside its exact-size array.  Stand-alone; never through python's process, never on the GPU."""
    exe = pui.build_program(workdir, sanitize=True)
    for name in sorted(CASES):
        recs, names = CASES[name]
        raw = b"".join(recs)
        for k, flt in enumerate((pui.FILTERS[0], pui.FILTERS[2])):
            got = pui.run_program(exe, workdir, "san_%s_%d" % (name, k), REF, raw, names, *flt)
            if name == "ends_bad":
                assert got["bad"] is not None
            else:
                entries, stats = pui.twin(raw, REF, *flt)
                assert got["text"] == pui.text_of(entries, names) and got["stats"] == stats
    # the liar as the array's last record, and a record cut short by the array's end: its bases lie behind the array
    recs, names = CASES["nothing"]
    raw = b"".join(recs[:4]) + pui.liar()
    assert [x[:2] for x in pui.run_program(exe, workdir, "san_liar_last", REF, raw, names, min_alt=1)["entries"]] == [x[:2] for x in pui.twin(raw, REF, min_alt=1)[0]] == [(0, 201)]
    whole = pui.rec_on(REF, 0, 900, 0, b"cut", [(30, pui.M)], {29: "!"})
    for k, (gone, want) in enumerate(((30, [(0, 201), (0, 929)]), (34, [(0, 201)]))):      # the qualities are gone: the bases still lie inside; four bytes of bases too: nothing
        raw = b"".join(recs[:4]) + whole[:len(whole) - gone]
        got = pui.run_program(exe, workdir, "san_cut_%d" % k, REF, raw, names, min_alt=1)
        assert [x[:2] for x in got["entries"]] == [x[:2] for x in pui.twin(raw, REF, min_alt=1)[0]] == want and pui.brute(raw, REF, min_alt=1) == got["entries"]
    ref = pui.random_ref(5, [1600, 1700, 1650])
    recs = pui.random_records(random.Random(5), 1200, ref)
    got = pui.run_program(exe, workdir, "san_random", ref, b"".join(recs), [b"a", b"bb", b"ccc"])
    assert got["entries"] == pui.twin(b"".join(recs), ref)[0]
