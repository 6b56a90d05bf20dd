"""CPU suite: the host-callable code of the device's MD / NM / ts stage (dart_amd/csrc/dg_tags.h) through tests/native/tags_checks.hip -- the length pass, the scan
and the write pass lane by lane -- against the sequential Python twin of tests/tags_inputs.py, the twin against an independent restatement (per-base columns, a
generic aux decoder), and what each crafted record is there for, spelled out.  The tags are the definition in the header's comment; no samtools is run."""
import random
import struct
import pytest
import tags_inputs as tgi
from tags_inputs import M, I, D, N, S

CASES = tgi.crafted_cases()
REF = tgi.REF


@pytest.fixture(scope="module")
def exe(workdir):
    return tgi.build_program(workdir)


def _check(exe, workdir, tag, recs, flags, ref=REF):
    raw = b"".join(recs)
    want, stats = tgi.twin(raw, ref, flags)
    got = tgi.run_program(exe, workdir, tag, ref, raw, flags)
    assert got["recs"] == tgi.twin_kinds(raw, ref, flags)
    assert got["out"] == want and got["stats"] == stats
    assert tgi.restate(raw, ref, flags) == want
    again, stats2 = tgi.twin(want, ref, flags)
    assert again == want and stats2[:3] == stats[:3] and stats2[4:] == stats[4:]               # idempotence: the second pass removes what the first appended
    return {tgi.name_of(x): x for x in (want[a:a + 4 + struct.unpack_from("<I", want, a)[0]] for a in tgi.offsets(want))}, stats


@pytest.mark.parametrize("flags", tgi.FLAG_SETS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_lane_code_equals_the_twin_on_the_crafted_records(name, flags, exe, workdir):
    _check(exe, workdir, "%s_%d" % (name, flags), CASES[name], flags)


def test_what_the_crafted_records_are_there_for(exe, workdir):
    ref_letter = lambda p, tid=0: "ACGT"[REF.base(tid, p)]
    out, st = _check(exe, workdir, "step_again", CASES["step"], tgi.ALL)
    for j, n in enumerate((1, 15, 16, 17, 31, 32, 33)):                                         # a mismatch on the last base of a run that ends on, in front of and behind a step's end
        assert tgi.md_of(out[b"m%d" % n]) == "%d%s0" % (n - 1, ref_letter(100 + 50 * j + n - 1)) and tgi.nm_of(out[b"m%d" % n]) == 1
        assert tgi.md_of(out[b"m%d_clean" % n]) == "%d" % n and tgi.nm_of(out[b"m%d_clean" % n]) == 0
    assert tgi.md_of(out[b"at15"]) == "15%s24" % ref_letter(515) and tgi.md_of(out[b"at16"]) == "16%s23" % ref_letter(516)
    assert tgi.md_of(out[b"at15_16"]) == "15%s0%s23" % (ref_letter(515), ref_letter(516))                                   # the run crosses the seam, and a run of 0 across it
    assert tgi.md_of(out[b"odd_start_s"]) == "0%s15%s19%s0" % (ref_letter(600), ref_letter(616), ref_letter(636))           # the low nibble first
    for k in range(4):
        assert tgi.md_of(out[b"pos_mod4_%d" % k]).startswith("0%s" % ref_letter(1000 + k)) and tgi.nm_of(out[b"pos_mod4_%d" % k]) == 4
    L0, L1 = REF.chr_len
    assert tgi.md_of(out[b"last_of_last"]) == "19%s0" % ref_letter(L1 - 1, 1) and tgi.md_of(out[b"the_last_base"]) == "0%s0" % ref_letter(L1 - 1, 1)      # pu_ref16's base-by-base tail
    assert tgi.md_of(out[b"last_of_first"]) == "19%s0" % ref_letter(L0 - 1) and st[0] == len(CASES["step"])                 # the text's neighbour is another chromosome
    out, st = _check(exe, workdir, "text_again", CASES["text"], tgi.ALL)
    for n in (9, 10, 99, 100):
        assert tgi.md_of(out[b"run%d" % n]) == "%d%s%d" % (n, ref_letter(100 + n), n)
    assert tgi.md_of(out[b"side_by_side"]) == "5%s0%s13" % (ref_letter(405), ref_letter(406))
    assert tgi.md_of(out[b"first_and_last"]) == "0%s18%s0" % (ref_letter(400), ref_letter(419))
    assert tgi.md_of(out[b"d_then_mismatch"]) == "10^%s%s0%s9" % (ref_letter(460), ref_letter(461), ref_letter(462)) and tgi.nm_of(out[b"d_then_mismatch"]) == 3
    assert tgi.md_of(out[b"two_d"]) == "10^%s0^%s10" % ("".join(ref_letter(460 + k) for k in range(2)), "".join(ref_letter(462 + k) for k in range(3))) and tgi.nm_of(out[b"two_d"]) == 5
    assert tgi.md_of(out[b"d_zero"]) == "20" and tgi.md_of(out[b"d_first_op"]) == "0^%s%s10" % (ref_letter(450), ref_letter(451))
    assert tgi.md_of(out[b"i_first"]) == "20" and tgi.nm_of(out[b"i_first"]) == 3 and tgi.md_of(out[b"i_last"]) == "20" and tgi.nm_of(out[b"i_last"]) == 3
    assert tgi.md_of(out[b"s_both"]) == "0%s18%s0" % (ref_letter(520), ref_letter(539)) and tgi.nm_of(out[b"s_both"]) == 2
    assert tgi.md_of(out[b"h_p"]) == "9%s0%s9" % (ref_letter(549), ref_letter(550))
    assert tgi.md_of(out[b"l_seq_1"]) == "1" and tgi.md_of(out[b"l_seq_1_s"]) == "0" and tgi.nm_of(out[b"l_seq_1_s"]) == 0
    assert tgi.md_of(out[b"thousand"]) == "".join("0" + ref_letter(1600 + k) for k in range(1000)) + "0" and tgi.nm_of(out[b"thousand"]) == 1000       # the longest MD: 2 l_seq + 1
    for k in range(4):                                                                          # '=' and the reference's own letter match; the other fourteen do not
        assert tgi.nm_of(out[b"nibbles%d" % k]) == sum(1 for j in range(16) if not (j == 0 or j == 1 << REF.base(0, 700 + k + j)))
    out, st = _check(exe, workdir, "nm_again", CASES["nm"], tgi.ALL)
    width = lambda x: tgi.tags_of(x)[b"NM"][-1][:1]
    assert (tgi.nm_of(out[b"nm255"]), width(out[b"nm255"])) == (255, b"C") and (tgi.nm_of(out[b"nm256"]), width(out[b"nm256"])) == (256, b"S")
    assert (tgi.nm_of(out[b"nm255_indel"]), width(out[b"nm255_indel"])) == (255, b"C") and (tgi.nm_of(out[b"nm256_indel"]), width(out[b"nm256_indel"])) == (256, b"S")
    assert tgi.tags_of(out[b"nm0"])[b"NM"] == [b"C\0"] and st[3] == 1                            # the mapper's NM:i is gone, one NM stays
    assert len(out[b"nm256"]) == len(out[b"nm255"]) + 1 + 2                                     # one byte of NM, "0X" -> "X", and one digit more in the run behind
    out, st = _check(exe, workdir, "ts_again", CASES["ts"], tgi.ALL)
    for name, g in ((b"gtag", "+"), (b"gcag", "+"), (b"ctac", "-"), (b"ctgc", "-"), (b"four", "+")):
        flip = "-" if g == "+" else "+"
        assert tgi.ts_of(out[name]) == g and tgi.ts_of(out[name + b"_rev"]) == flip and tgi.ts_of(out[name + b"_mate2_rev"]) == flip
    for name in (b"none", b"three", b"none_rev", b"three_rev", b"two_conflict", b"old_ts_no_new"):
        assert tgi.ts_of(out[name]) is None
    assert tgi.ts_of(out[b"two_agree"]) == "+" and tgi.ts_of(out[b"two_agree_rev"]) == "-" and tgi.ts_of(out[b"two_minus"]) == "+"
    assert tgi.ts_of(out[b"canonical_and_not"]) == "-" and tgi.ts_of(out[b"not_and_short"]) == "+" and tgi.ts_of(out[b"intron_at_the_start"]) == "+"
    assert st[6] == 5 * 3 + 6 and st[7] == 3 | 1 << 32 and st[3] == 1                           # no motif: the three `none`; a length of 3 is no intron; one conflict
    assert tgi.md_of(out[b"gtag"]) == "9%s10" % ref_letter(1199) and tgi.md_of(out[b"gtag_rev"]) == "10%s9" % ref_letter(1250)           # an N prints nothing and the run goes on
    out, st = _check(exe, workdir, "aux_again", CASES["aux"], tgi.ALL)
    new = lambda x: (b"NM", b"MD") == tuple(list(tgi.tags_of(x))[-2:])
    assert out[b"every_type"].find(tgi.EVERY_TYPE) > 0 and new(out[b"every_type"]) and new(out[b"no_aux"])
    for name in (b"old_first", b"old_middle", b"old_last", b"old_twice", b"old_only", b"old_other_types"):
        t = tgi.tags_of(out[name])
        assert t[b"MD"] == [b"Z" + tgi.md_of(out[b"no_aux"]).encode() + b"\0"] and t[b"NM"] == [b"C\x01"] and b"ts" not in t and new(out[name])
    assert list(tgi.tags_of(out[b"old_twice"])) == [b"AS", b"XS", b"NM", b"MD"] and list(tgi.tags_of(out[b"old_only"])) == [b"NM", b"MD"]
    by_name = {tgi.name_of(x): x for x in CASES["aux"]}
    for name in (b"unknown_type", b"z_without_nul", b"b_past_the_end", b"b_bad_subtype", b"b_huge_count", b"two_bytes_left", b"value_cut", b"old_md_unreadable_behind"):
        assert out[name] == by_name[name]
    assert st[2] == 8 and st[3] == 3 + 3 + 3 + 6 + 1 + 3
    # one of the three names present but not selected: it stays where it is
    out, st = _check(exe, workdir, "aux_md_only", CASES["aux"], tgi.MD_)
    t = tgi.tags_of(out[b"old_first"])
    assert list(t) == [b"NM", b"ts", b"AS", b"XS", b"MD"] and t[b"NM"] == [b"i" + struct.pack("<i", 99)] and t[b"ts"] == [b"A+"]
    out, st = _check(exe, workdir, "aux_ts_only", CASES["aux"], tgi.TS_)
    assert list(tgi.tags_of(out[b"old_last"])) == [b"AS", b"XS", b"NM", b"MD"] and tgi.md_of(out[b"old_last"]) == "7" and st[6] == 0 and st[7] == 0 and st[4] == 8
    out, st = _check(exe, workdir, "ne_again", CASES["not_eligible"], tgi.ALL)
    by_name = {tgi.name_of(x): x for x in CASES["not_eligible"]}
    assert all(out[k] == v for k, v in by_name.items() if k != b"the_one_that_counts") and st[:3] == (1, len(by_name) - 1, 0)
    assert tgi.tags_of(out[b"the_one_that_counts"]) == {b"NM": [b"C\x01"], b"MD": [b"Z1%s8\0" % ref_letter(201).encode()]}
    assert _check(exe, workdir, "empty_again", [], tgi.ALL)[1] == (0,) * 8


def test_records_whose_block_size_lies_are_copied_verbatim(exe, workdir):
    good = CASES["not_eligible"][-1:]
    for k, (name, bad) in enumerate(sorted(tgi.lying_records().items())):
        for flags in (tgi.ALL, tgi.MD_):
            out, st = _check(exe, workdir, "lie_%d_%d" % (k, flags), good + [bad], flags)
            assert st[0] == 1 and st[1] == 1 and st[2] == 0, name
            assert tgi.twin(b"".join(good + [bad]), REF, flags)[0].endswith(bad)


def test_random_records(exe, workdir):
    ref = tgi.random_ref(3, [1700, 1601, 1602])
    rng = random.Random(17)
    recs = tgi.with_old_tags(tgi.pui.random_records(rng, 2500, ref), rng)
    for flags in (tgi.ALL, tgi.MD_ | tgi.TS_, tgi.NM_):
        out, st = _check(exe, workdir, "random_%d" % flags, recs, flags, ref)
        assert st[0] > 1000 and st[1] > 100 and st[4] > 300 and st[5] > 1000 and st[3] >= (st[0] if flags & tgi.NM_ else 100)      # (what the inputs hold, not what the code makes of them)
    assert tgi.twin(b"".join(recs), ref, tgi.ALL)[1][7] & 0xFFFFFFFF > 50                       # random text: introns without a motif


def test_lane_code_under_the_sanitizers(workdir):
    """the same program with AddressSanitizer and UBSan on its host code: every record walk stays inside the exact-size heap copy of the array, every fetch of the
    text inside the exact-size pac, every stored byte inside the record's own room in the exact-size new array.  Stand-alone; never through python's process, never
    on the GPU."""
    exe = tgi.build_program(workdir, sanitize=True)
    for name in sorted(CASES):
        raw = b"".join(CASES[name])
        for flags in (tgi.ALL, tgi.MD_, tgi.NM_ | tgi.TS_):
            got = tgi.run_program(exe, workdir, "san_%s_%d" % (name, flags), REF, raw, flags)
            assert (got["out"], got["stats"]) == tgi.twin(raw, REF, flags)
    for k, bad in enumerate(sorted(tgi.lying_records().values())):
        raw = b"".join(CASES["aux"][:3]) + bad
        got = tgi.run_program(exe, workdir, "san_lie_%d" % k, REF, raw, tgi.ALL)
        assert (got["out"], got["stats"]) == tgi.twin(raw, REF, tgi.ALL)
    ref = tgi.random_ref(5, [1600, 1700, 1650])
    rng = random.Random(5)
    recs = tgi.with_old_tags(tgi.pui.random_records(rng, 1200, ref), rng)
    got = tgi.run_program(exe, workdir, "san_random", ref, b"".join(recs), tgi.ALL)
    assert (got["out"], got["stats"]) == tgi.twin(b"".join(recs), ref, tgi.ALL)
