"""CPU suite: the host-callable code of the device's coverage track (dart_amd/csrc/dg_coverage.h) through tests/native/coverage_checks.hip -- a record's filter
and blocks, the sorted events, the breakpoints, the entries and the text's bytes -- against the sequential Python twin of tests/coverage_inputs.py, and the twin
against a per-base depth array.  The track is the definition in the header's comment (modelled on `bedtools genomecov -bg -split` with the default filter of
`samtools depth`); neither tool is run."""
import random
import pytest
import coverage_inputs as cvi

CASES = cvi.crafted_cases()


@pytest.fixture(scope="module")
def exe(workdir):
    return cvi.build_program(workdir)


def _twin_events(raw, n_chr, flt):
    ev, recs, blocks = [], [], []
    for i, at in enumerate(cvi.offsets(raw)):
        c = cvi.counted(raw, at, n_chr, *flt)
        b = cvi.blocks_of(c[1], c[2]) if c else []
        recs.append((1 if c else 0, len(b)))
        for s, e in b:
            blocks.append((i, s, e)); ev += [(c[0] << 32 | s, 1), (c[0] << 32 | e, -1)]
    return recs, blocks, sorted(ev, key=lambda x: x[0])


def _check(exe, workdir, tag, n_chr, recs, names, flt):
    raw = b"".join(recs)
    got = cvi.run_program(exe, workdir, tag, n_chr, raw, names, *flt)
    entries, stats = cvi.twin(raw, n_chr, *flt)
    t_recs, t_blocks, t_events = _twin_events(raw, n_chr, flt)
    assert got["bad"] is None and got["recs"] == t_recs and got["blocks"] == t_blocks
    assert [k for k, _ in got["events"]] == [k for k, _ in t_events] and sorted(got["events"]) == sorted(t_events)       # (equal keys: the order of their deltas is the input's)
    depth, bps = 0, []
    sums = {}
    for k, d in t_events:
        sums[k] = sums.get(k, 0) + d
    for k in sorted(sums):
        depth += sums[k]
        if sums[k]:
            bps.append((k, depth))
    assert got["bps"] == bps
    assert got["entries"] == entries and got["stats"] == stats
    assert got["text"] == cvi.text_of(entries, names)
    assert cvi.per_base(raw, n_chr, *flt) == cvi.clip(entries)
    return entries, stats


@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "edge_bad"))
def test_lane_code_equals_the_twin_on_the_crafted_records(name, exe, workdir):
    n_chr, recs, names = CASES[name]
    for k, flt in enumerate(cvi.FILTERS):
        _check(exe, workdir, "%s_%d" % (name, k), n_chr, recs, names, flt)


def test_what_the_crafted_records_are_there_for(exe, workdir):
    dflt = cvi.FILTERS[0]
    run = lambda name, flt=dflt: _check(exe, workdir, name + "_again", *CASES[name], flt)
    e, st = run("cigar")
    on0 = [(s, en, d) for c, s, en, d in e if c == 0]
    assert (100, 110, 1) in on0 and (813, 818, 1) in on0                       # all nine ops: S, I, P, H change nothing; = and X abut into one interval
    assert (300, 305, 1) in on0 and not any(s <= 320 < en for s, en, _ in on0)  # a zero-length M is no block
    assert (400, 420, 1) in on0                                                 # blocks abutting across an I: one interval
    assert (500, 510, 1) in on0 and (560, 570, 1) in on0                        # an N gap: two
    assert [(1000, 1010, 2), (1010, 1015, 1), (1015, 1025, 2)] == [x for x in on0 if 1000 <= x[0] < 1025]      # a D under a second read: depth drops by one
    assert (2000, 2010, 1) in on0 and (2015, 2025, 1) in on0 and not any(s <= 2012 < en for s, en, _ in on0)    # a D alone: a hole
    assert st[0] == 8 and st[1] == 3 + 1 + 0 + 2 + 2 + 2 + 1 + 2
    e, st = run("depth")
    on0 = [(s, en, d) for c, s, en, d in e if c == 0]
    assert (100, 200, 1) in on0                                                 # a read ending where another begins, equal depth: merged
    assert (300, 350, 1) in on0 and (350, 400, 2) in on0                        # different depth: split; identical reads: depth 2
    assert (1000, 1050, 12) in on0 and st[6] == 12
    text = cvi.text_of(e, CASES["depth"][2])
    assert b"chrA\t1000\t1050\t12\n" in text
    assert sorted(len(str(s)) for c, s, _, _ in e if c == 1) == list(range(1, 11)) and b"b\t2000000000\t2000000003\t1\n" in text
    e, st = run("edge")
    assert (0, 0, 5, 1) in e and e[-1] == (1, cvi.MAX_POS - 8, cvi.MAX_POS, 1)  # pos 0; a block that ends exactly at 2^32 - 1
    e, st = run("nothing")
    assert e == [(0, 200, 210, 1)] and st[0] == 1                               # pos -1, no CIGAR, placed unmapped, unplaced: nothing
    assert run("nothing_liar")[0] == e                                          # n_cigar_op larger than block_size allows: nothing, and no read behind the record
    names = [r[36:36 + r[12] - 1] for r in CASES["filters"][1]]
    starts = lambda flt: {(c, s) for c, s, _, _ in run("filters", flt)[0]}
    pos = {nm: (int.from_bytes(r[4:8], "little"), int.from_bytes(r[8:12], "little")) for nm, r in zip(names, CASES["filters"][1])}
    everything = starts((4, 0, None))
    assert len(everything) == len(names) == 11
    for bit, nm in ((0x100, b"secondary"), (0x200, b"qcfail"), (0x400, b"duplicate")):
        assert everything - starts((bit | 4, 0, None)) == {pos[nm]}              # each of the three bits alone
    assert everything - starts(dflt) == {(0, 100), (0, 200), (0, 300)}
    assert starts(dflt) - starts((cvi.DEFAULT_EXCLUDE, 10, None)) == {pos[b"mapq9"]}      # mapq == min_mapq counts, min_mapq - 1 does not
    fwd, rev = starts((cvi.DEFAULT_EXCLUDE, 0, "+")), starts((cvi.DEFAULT_EXCLUDE, 0, "-"))
    assert {x for x in fwd if x[0] == 1} == {pos[b"unpaired_fwd"], pos[b"mate1_fwd"], pos[b"mate2_rev"]}
    assert {x for x in rev if x[0] == 1} == {pos[b"unpaired_rev"], pos[b"mate1_rev"], pos[b"mate2_fwd"]}
    e, st = run("refs")
    assert [c for c, _, _, _ in e] == [0, 2, 3] and e == [(0, 90, 100, 1), (2, 100, 110, 1), (3, 110, 115, 1)]       # an empty middle chromosome; equal positions on neighbouring references
    assert cvi.text_of(e, CASES["refs"][2]) == b"one\t90\t100\t1\nthree\t100\t110\t1\na_longer_name_4\t110\t115\t1\n"
    assert run("empty") == ([], (0,) * 7)


def test_a_block_behind_2_32_is_refused_with_the_records_index(exe, workdir):
    n_chr, recs, names = CASES["edge_bad"]
    raw = b"".join(recs)
    k = [r[36:36 + r[12] - 1] for r in recs].index(b"ends_at_2_32")
    got = cvi.run_program(exe, workdir, "edge_bad", n_chr, raw, names)
    assert got["bad"] == k and got["text"] == b"" and not got["entries"]
    with pytest.raises(cvi.RangeError) as x:
        cvi.twin(raw, n_chr)
    assert x.value.args[0] == k
    # a record that is not counted is never out of range: the duplicate in front is, once duplicates count
    got = cvi.run_program(exe, workdir, "edge_bad_dups", n_chr, raw, names, exclude=4)
    assert got["bad"] == k - 1
    with pytest.raises(cvi.RangeError) as x:
        cvi.twin(raw, n_chr, exclude=4)
    assert x.value.args[0] == k - 1


def _random_raw(seed, n, n_chr):
    rng = random.Random(seed)
    recs = cvi.random_records(rng, n, n_chr)
    return recs, rng


def test_random_records_and_a_shuffled_copy(exe, workdir):
    n_chr = 3
    names = [b"c0", b"chr_one", b"2"]
    recs, rng = _random_raw(17, 3000, n_chr)
    for k, flt in enumerate((cvi.FILTERS[0], cvi.FILTERS[1], cvi.FILTERS[5], cvi.FILTERS[7])):
        entries, stats = _check(exe, workdir, "random_%d" % k, n_chr, recs, names, flt)
        assert stats[3] > 500 and stats[2] < 2 * stats[1] and (k or stats[6] >= 10)      # events that share a key, and deep piles
    # the result is a function of the record set, not of its order
    shuffled = list(recs); rng.shuffle(shuffled)
    assert shuffled != recs
    assert cvi.twin(b"".join(shuffled), n_chr) == cvi.twin(b"".join(recs), n_chr)
    got = cvi.run_program(exe, workdir, "random_shuffled", n_chr, b"".join(shuffled), names)
    assert got["entries"] == cvi.twin(b"".join(recs), n_chr)[0] and got["text"] == cvi.text_of(got["entries"], names)


def test_lane_code_under_the_sanitizers(workdir):
    """the same program with AddressSanitizer and UBSan on its host code: every record walk stays inside the exact-size heap copy of the array, every event,
    entry and line inside its exact-size array.  Stand-alone; never through python's process, never on the GPU."""
    exe = cvi.build_program(workdir, sanitize=True)
    for name in sorted(CASES):
        n_chr, recs, names = CASES[name]
        raw = b"".join(recs)
        for k, flt in enumerate((cvi.FILTERS[0], cvi.FILTERS[1])):
            got = cvi.run_program(exe, workdir, "san_%s_%d" % (name, k), n_chr, raw, names, *flt)
            if name == "edge_bad":
                assert got["bad"] is not None
            else:
                entries, stats = cvi.twin(raw, n_chr, *flt)
                assert got["text"] == cvi.text_of(entries, names) and got["stats"] == stats
    # the liar as the array's last record, and a record cut short by the array's end
    n_chr, recs, names = CASES["nothing"]
    raw = b"".join(recs[:4]) + cvi.liar()
    assert cvi.run_program(exe, workdir, "san_liar_last", n_chr, raw, names)["entries"] == cvi.twin(raw, n_chr)[0] == [(0, 200, 210, 1)]
    recs, _ = _random_raw(5, 1500, 3)
    got = cvi.run_program(exe, workdir, "san_random", 3, b"".join(recs), [b"a", b"bb", b"ccc"])
    assert got["entries"] == cvi.twin(b"".join(recs), 3)[0]
