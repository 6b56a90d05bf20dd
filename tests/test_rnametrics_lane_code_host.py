"""CPU suite: the host-callable code of the device's RNA-seq metrics (dart_amd/csrc/dg_rnametrics.h) through tests/native/rnametrics_checks.hip -- the flattening,
k_rm_class's lane per record, the coverage track's event path and k_rm_body's wave per transcript, lane by lane -- against the sequential Python twin of
tests/rnametrics_inputs.py, the twin against its independent per-base restatement, and the host formatter (the native program's and the library's
dg_bam_rna_format) against the twin's text_of.  The words are the definition in the header's comment; no Picard or RSeQC is run."""
import random
import subprocess
import numpy as np
import pytest
import coverage_inputs as cvi
import rnametrics_inputs as rmi
from rnametrics_inputs import OFF, SN, M, N
from dart_amd import host

ANNOT = rmi.crafted_annotation()
CASES = rmi.crafted_cases()
EVERYTHING = b"".join(r for name in sorted(CASES) for r in CASES[name])


@pytest.fixture(scope="module")
def exe(workdir):
    return rmi.build_program(workdir)


def _check(exe, workdir, tag, raw, flt=rmi.FILTERS[0], min_cov=rmi.DEFAULT_MIN_COV, annot=ANNOT, n_chr=2, paint=True):
    res = rmi.run_program(exe, workdir, tag, n_chr, raw, annot, *flt, min_cov)
    want = rmi.twin(raw, n_chr, annot, *flt, min_cov)
    assert res["rc"] == 0 and res["bad"] is None
    assert np.array_equal(res["words"], want), [(int(k), int(res["words"][k]), int(want[k])) for k in np.flatnonzero(res["words"] != want)[:10]]
    if paint:
        assert np.array_equal(rmi.paint(raw, n_chr, annot, *flt, min_cov), want)
    assert res["text"] == rmi.text_of(want)
    segs, elig = rmi.flatten(annot, n_chr)
    assert res["segs"] == [(c, s, p[0], p[1]) for c in range(n_chr) for s, p in zip(*segs[c])] and res["elig"] == len(elig)
    return rmi.views(want), res


@pytest.mark.parametrize("name", sorted(CASES))
def test_lane_code_equals_the_twin_and_the_twin_the_restatement_on_the_crafted_records(name, exe, workdir):
    raw = b"".join(CASES[name])
    for k, flt in enumerate(rmi.FILTERS):
        _check(exe, workdir, "%s_%d" % (name, k), raw, flt, min_cov=1)


def test_the_crafted_annotation_flattens_to_what_it_is_there_for(exe, workdir):
    v, res = _check(exe, workdir, "annot", EVERYTHING)
    seg0 = [s[1:] for s in res["segs"] if s[0] == 0]
    # transcript 0: UTR, coding, rRNA over coding, coding, UTR behind the exon?  no: the CDS [120, 320) covers the exon's end; intron; 1's UTR over the intron with both strands
    assert seg0[:11] == [(100, 2, 1), (120, 3, 1), (130, 4, 1), (140, 3, 1), (200, 1, 1), (220, 2, 3), (260, 1, 1), (300, 3, 1), (320, 2, 1), (350, 0, 0), (1000, 2, 2)]
    assert seg0[-1] == (2700, 0, 0) and not [s for s in res["segs"] if s[0] == 1]
    assert res["elig"] == 6 and v["SN"][SN["transcripts"]] == 11 and v["SN"][SN["segments"]] == len(res["segs"])      # L 150, 100, 101, 100, 100, 100; 40, 10, 99, 50 and 50 are not
    # unsorted, overlapping and touching exons give the tables of the merged ones
    tidy = [dict(a, exons=rmi.merged(a)) for a in ANNOT]
    assert rmi.flatten(tidy, 2) == rmi.flatten(ANNOT, 2)
    assert rmi.run_program(exe, workdir, "tidy", 2, b"", tidy)["segs"] == res["segs"]


def test_what_the_crafted_records_are_there_for(exe, workdir):
    one = lambda r, flt=rmi.FILTERS[2], **kw: _check(exe, workdir, "one", r, flt, **kw)[0]
    ba = lambda r: [int(x) for x in one(r)["BA"]]
    rec = lambda pos, cigar, flag=0, tid=0: rmi.record(tid, pos, flag, b"r", cigar, l_seq=0, mapq=30)
    # a block that ends one base before, exactly at and one base behind a boundary (100: intergenic | UTR), and the same for its start
    assert [ba(rec(90, [(l, M)])) for l in (9, 10, 11)] == [[9, 0, 0, 0, 0], [10, 0, 0, 0, 0], [10, 0, 1, 0, 0]]
    assert [ba(rec(p, [(10, M)])) for p in (99, 100, 101)] == [[1, 0, 9, 0, 0], [0, 0, 10, 0, 0], [0, 0, 10, 0, 0]]
    assert [ba(rec(p, [(1, M)])) for p in (199, 200, 349, 350)] == [[0, 0, 0, 1, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [1, 0, 0, 0, 0]]
    v = one(rec(90, [(270, M)]))                                     # ten segments under one block
    assert [int(x) for x in v["BA"]] == [20, 60, 20 + 40 + 30, 10 + 60 + 20, 10] and v["RC"][4] == 1 and v["ST"][2] == 1
    # behind the last segment, in front of the first, on a chromosome without a transcript: intergenic
    for r in (rec(2900, [(50, M)]), rec(10, [(20, M)]), rec(100, [(50, M)], tid=1)):
        v = one(r)
        assert v["BA"][0] == v["SN"][SN["aligned_bases"]] and v["RC"][0] == 1 and v["ST"][3] == 1
    # class priority per record: the N of a spliced read spans transcript 8's exon and touches nothing of it
    v = one(rec(2230, [(20, M), (150, N), (20, M)]))
    assert [int(x) for x in v["BA"]] == [0, 0, 0, 40, 0] and v["RC"][3] == 1 and v["ST"][0] == 1 and v["SN"][SN["blocks"]] == 2
    v = one(rec(2230, [(200, M)]))                                   # the same stretch unspliced: intron, 8's UTR and coding on the other strand
    assert [int(x) for x in v["BA"]] == [0, 100, 20, 80, 0] and v["ST"][2] == 1
    # strands: a plus-only place, a minus-only place, both, none; s = reverse ^ second mate
    rows = lambda pos: [int(np.argmax(one(rec(pos, [(10, M)], f))["ST"])) for f in (0, 16, 0x41, 0x51, 0x81, 0x91)]
    assert rows(105) == [0, 1, 0, 1, 1, 0] and rows(1005) == [1, 0, 1, 0, 0, 1] and rows(225) == [2] * 6 and rows(1300) == [3] * 6
    # depth at a block's start, at its last base and at its end, on transcript 6 whose every base is a sample: in, in, out
    v = one(rec(1920, [(30, M)]), min_cov=1)
    assert v["BC"][0].tolist() == [0] * 20 + [1] * 30 + [0] * 50 and v["BC"][1].tolist() == v["BC"][0].tolist() and v["BC"][2, 20:50].tolist() == [100000 // 30] * 30
    assert v["SN"][SN["contributing_transcripts"]] == 1
    # a minus-strand transcript's samples run right to left: its 5' end is its last exon's last base
    v = one(rec(1225, [(5, M)]), min_cov=1)
    assert v["BC"][0].tolist() == [1] * 5 + [0] * 95
    v = one(rec(1000, [(1, M)]) + rec(1039, [(1, M)]) + rec(1100, [(1, M)]), min_cov=1)      # the first and last base of the leftmost exon (its 3' end) and the first of the next: offsets 0, 39, 40 from the left
    assert np.flatnonzero(v["BC"][0]).tolist() == [59, 60, 99]
    # L 101: o_b = floor((2 b + 1) 101 / 200); the one base no sample lands on is offset 50
    v = one(b"".join(rec(1700 + o, [(1, M)]) for o in range(101)), min_cov=1)
    assert v["BC"][0].tolist() == [1] * 100 and one(rec(1750, [(1, M)]), min_cov=1)["SN"][SN["contributing_transcripts"]] == 0
    # L 99 is not eligible however deep
    assert one(rec(1500, [(99, M)]) * 50, min_cov=1)["BC"].sum() == 0


def test_many_events_with_one_key_and_event_runs_that_straddle_workgroups(exe, workdir):
    rec = lambda pos, ln: rmi.record(0, pos, 0, b"r", [(ln, M)], l_seq=0, mapq=30)
    for n in (127, 128, 129, 300):                                   # 2 n events: 256 a workgroup
        raw = rec(1900, 50) * n + rec(1950, 50) * n                   # n ends and n starts share the key 1950
        v, _ = _check(exe, workdir, "pile%d" % n, raw, min_cov=1)
        assert v["BC"][0].tolist() == [n] * 100 and v["BC"][2].tolist() == [1000] * 100


def test_contribution_threshold(exe, workdir):
    raw = EVERYTHING
    words, sums = rmi.twin(raw, 2, ANNOT, want_sums=True)
    assert 0 in sums and len(sums) == 6                              # transcript 9 is never covered
    S = sorted(set(s for s in sums if s > 1))[0]
    n_at = lambda mc: int(_check(exe, workdir, "mc%d" % mc, raw, min_cov=mc)[0]["SN"][SN["contributing_transcripts"]])
    assert n_at(S - 1) == n_at(S) == n_at(S + 1) + 1                 # one below, at, one above
    assert n_at(0) == n_at(1) == sum(1 for s in sums if s > 0)       # min_cov 0: S = 0 does not contribute
    assert n_at(1 << 40) == 0


def test_records_excluded_by_each_filter_bit(exe, workdir):
    raw = b"".join(CASES["filters"])
    counted = lambda flt: int(_check(exe, workdir, "flt", raw, flt)[0]["SN"][SN["counted"]])
    assert counted((4, 0)) == 6 and counted((0x904, 0)) == 4 and counted((0x704, 0)) == 3 and counted((0x904, 10)) == 3 and counted((0x404, 0)) == 5
    assert counted((0, 0)) == 6                                      # flag 4 is left out whatever the filter says; no CIGAR, pos -1 and no chromosome too


def test_random_records_and_annotations(exe, workdir):
    rng = random.Random(5)
    for k in range(6):
        n_chr = 1 + k % 3
        annot = rmi.random_annotation(rng, n_chr, rng.choice([1, 5, 40]))
        raw = b"".join(cvi.random_records(rng, 300, n_chr))
        _check(exe, workdir, "rand%d" % k, raw, rmi.FILTERS[k % len(rmi.FILTERS)], min_cov=rng.choice([0, 1, 50, 100]), annot=annot, n_chr=n_chr)


def test_range_and_refused_annotations(exe, workdir):
    ok, bad = rmi.range_cases()
    v, _ = _check(exe, workdir, "edge_ok", b"".join(ok), paint=False)
    assert v["BA"][0] == 13
    res = rmi.run_program(exe, workdir, "edge_bad", 2, b"".join(bad), ANNOT)
    assert res["bad"] == 1 and res["words"] is None                  # (the default filter counts duplicates)
    with pytest.raises(rmi.RangeError) as x:
        rmi.twin(b"".join(bad), 2, ANNOT)
    assert x.value.args[0] == 1
    assert rmi.run_program(exe, workdir, "edge_dup", 2, b"".join(bad), ANNOT, exclude=0x704)["bad"] == 2      # with the duplicate left out, it is the next one
    for rule, annot in rmi.bad_annotations():
        res = rmi.run_program(exe, workdir, "badann", 2, b"", annot)
        assert res["rc"] == 3 and "transcript 1 " in res["err"] and rule in res["err"], (rule, res["err"])
    res = rmi.run_program(exe, workdir, "badann", 2, b"", [rmi.tx(0, 0, [(10, 20)]), rmi.tx(0, 0, [(30, 40), (50, 60)])], n_exons=2)
    assert res["rc"] == 3 and "transcript 1 " in res["err"] and "outside the exon array" in res["err"]
    assert rmi.run_program(exe, workdir, "badann", 2, b"", [])["rc"] == 3


def test_formatter_zero_denominators_and_wide_products(exe, workdir):
    import os
    lib = host._load_lib()
    big = (1 << 64) - 1
    cases = [np.zeros(OFF["words"], np.uint64)]
    w = np.zeros(OFF["words"], np.uint64); w[OFF["BA"]:OFF["BA"] + 5] = big // 5; w[OFF["SN"] + SN["aligned_bases"]] = big; w[OFF["ST"]] = big; w[OFF["ST"] + 1] = big
    w[OFF["BC"] + 200:OFF["BC"] + 210] = big; w[OFF["BC"] + 290:OFF["BC"] + 300] = big // 3; w[OFF["SN"] + SN["contributing_transcripts"]] = big
    cases.append(w)
    w = np.zeros(OFF["words"], np.uint64); w[OFF["ST"]] = 2; w[OFF["ST"] + 1] = 1; w[OFF["BC"] + 200] = 999; w[OFF["SN"] + SN["contributing_transcripts"]] = 1; w[OFF["BA"] + 3] = 7
    cases.append(w)                                                  # bins 90 .. 99 empty: five_to_three_milli has a zero denominator; aligned 0: ppm 0
    for k, w in enumerate(cases):
        want = rmi.text_of(w)
        assert host.rna_text(lib, w) == want
        src, out = os.path.join(workdir, "rm_fmt%d.bin" % k), os.path.join(workdir, "rm_fmt%d.txt" % k)
        open(src, "wb").write(w.tobytes())
        subprocess.check_call([exe, "--format", src, out])
        assert open(out, "rb").read() == want
    assert b"SN\tsense_ppm\t500000\n" in rmi.text_of(cases[1]) and b"SN\tfive_to_three_milli\t3000\n" in rmi.text_of(cases[1])
    assert b"SN\tsense_ppm\t666666\n" in rmi.text_of(cases[2]) and b"SN\tfive_to_three_milli\t0\n" in rmi.text_of(cases[2]) and b"SN\tfive_prime_milli\t99\n" in rmi.text_of(cases[2])
    nb = host.C.c_size_t(0)
    assert lib.dg_bam_rna_format(cases[0].ctypes.data, OFF["words"] - 1, None, 0, host.C.byref(nb)) == -3
    buf = np.zeros(8, np.uint8)
    assert lib.dg_bam_rna_format(cases[0].ctypes.data, OFF["words"], buf.ctypes.data, 8, host.C.byref(nb)) == -4 and not buf.any() and nb.value == len(rmi.text_of(cases[0]))
    off = (host.C.c_size_t * 6)()
    assert lib.dg_bam_rna_offsets(off) == 0 and list(off) == [OFF[k] for k in ("BA", "RC", "ST", "BC", "SN", "words")]


def test_the_program_built_with_sanitizers_on_its_host_code(workdir):
    """the same program, its host code under AddressSanitizer and UBSan, run directly on the inputs where an index could leave an array"""
    exe = rmi.build_program(workdir, sanitize=True)
    rng = random.Random(8)
    ok, bad = rmi.range_cases()
    runs = [(EVERYTHING, ANNOT, 2), (b"".join(ok), ANNOT, 2), (b"".join(bad), ANNOT, 2), (b"", ANNOT, 2), (EVERYTHING, [rmi.tx(1, 0, [(5, 6)])], 2),
            (b"".join(cvi.random_records(rng, 300, 3)), rmi.random_annotation(rng, 3, 40), 3), (b"".join(cvi.crafted_cases()["nothing_liar"][1]), ANNOT, 2)]
    for k, (raw, annot, n_chr) in enumerate(runs):
        res = rmi.run_program(exe, workdir, "san%d" % k, n_chr, raw, annot, 4, 0, 1)
        assert res["rc"] == 0
        if res["bad"] is None:
            assert np.array_equal(res["words"], rmi.twin(raw, n_chr, annot, 4, 0, 1))
    for rule, annot in rmi.bad_annotations():
        assert rmi.run_program(exe, workdir, "san_bad", 2, b"", annot)["rc"] == 3


def test_the_mapped_case_is_rich_enough_on_the_reference_records(exe, workdir):
    """the GPU suite's case over the mapper's own records, here with the records of the case's golden SAM (the reference's, which the mapper reproduces): the
    seeded annotation gives every class of BA, all four ST rows and at least ten contributing transcripts on each strand, and the lane code agrees with the twin"""
    import common
    case = common.build_case("pe101_spliced", workdir)
    names = host.Index(case["prefix"]).names
    annot = rmi.case_annotation(case, rmi.CASE_SEEDS["pe101_spliced"])
    recs = rmi.records_of_sam(common.golden_sam("pe101_spliced.run1"), names)      # run1: -mis 5, the GPU suite's flags
    assert len(recs) == 2 * case["spec"]["npairs"]
    raw = b"".join(recs)
    words, sums = rmi.twin(raw, 2, annot, min_cov=rmi.CASE_MIN_COV, want_sums=True)
    assert rmi.rich_enough(words, sums, annot, 2)
    v = rmi.views(words)
    assert v["SN"][SN["counted"]] > 2000 and v["SN"][SN["contributing_transcripts"]] >= 20 and v["SN"][SN["blocks"]] > v["SN"][SN["counted"]]      # spliced reads: more blocks than records
    res = rmi.run_program(exe, workdir, "case", 2, raw, annot, rmi.DEFAULT_EXCLUDE, 0, rmi.CASE_MIN_COV)
    assert res["rc"] == 0 and np.array_equal(res["words"], words) and res["text"] == rmi.text_of(words)
