"""CPU suite: the host-callable code of the device's BAM index (dart_amd/csrc/dg_bamidx.h) through tests/native/bamidx_checks.hip -- a record's beg / end /
bin and virtual offset, the chunks before and after the merge, the filled linear index and the final bytes -- against the sequential Python twin of
tests/bamidx_inputs.py, and the twin against an independent reader that answers region queries through the index.  The index is the definition in the
header's comment (what `samtools index` writes, with two named differences); no samtools is run."""
import random, struct
import pytest
import bamidx_inputs as bii

CASES = bii.crafted_cases()


@pytest.fixture(scope="module")
def exe(workdir):
    return bii.build_program(workdir)


def _check(exe, workdir, tag, n_chr, recs, first, sizes=None):
    raw = b"".join(recs)
    sizes = bii.stored_sizes(raw) if sizes is None else sizes
    got = bii.run_program(exe, workdir, tag, n_chr, raw, sizes, first)
    refs, n_no_coor, per_record = bii.walk(raw, sizes, first, n_chr)
    done = bii.finish(refs)
    assert got["bad"] is None and got["recs"] == per_record
    before = [(t << 16 | b, beg, end) for t, r in enumerate(refs) for b in sorted(r["bins"]) for beg, end in r["bins"][b]]
    after = [(t << 16 | b, beg, end) for t, (bins, _, _) in enumerate(done) for b, chunks in bins for beg, end in chunks]
    assert got["chunks"] == before and got["merged"] == after
    assert got["lin"] == {(t, w): v for t, (_, intv, _) in enumerate(done) for w, v in enumerate(intv)}
    want = bii.build_bai(raw, sizes, first, n_chr)
    assert got["bytes"] == want
    return raw, sizes, want, refs, done


@pytest.mark.parametrize("name", sorted(CASES))
def test_lane_code_equals_the_twin_on_the_crafted_records(name, exe, workdir):
    n_chr, recs, first = CASES[name]
    _check(exe, workdir, name, n_chr, recs, first)


def test_what_the_crafted_records_are_there_for(exe, workdir):
    n_chr, recs, first = CASES["main"]
    raw, sizes, bai, refs, done = _check(exe, workdir, "main_again", n_chr, recs, first)
    f = {r[36:36 + r[12] - 1]: bii.fields(r, 0, n_chr) for r in recs}
    g = lambda name: (f[name]["beg"], f[name]["end"], f[name]["bin"])
    assert f[b"all_ops"]["rlen"] == 10 + 3 + 700 + 4 + 1
    assert g(b"pos_m1") == (0, 9, 4681) and g(b"pos_m1_unmapped_placed") == (0, 1, 4681) and g(b"no_cigar_mapped") == (0, 1, 4681)
    assert g(b"ends_at_16k") == (16284, 16384, 4681) and g(b"crosses_16k_by_one") == (16284, 16385, 585)
    assert g(b"spans_level1")[2] == 0 and g(b"ends_at_2_29")[1] == bii.MAX_END and f[b"n" * 254]["rlen"] == 30
    assert f[b"placed_unmapped"]["placed"] and not f[b"placed_unmapped"]["mapped"]
    ix = bii.parse_bai(bai)
    assert ix["n_no_coor"] == 2 and [len(r["bins"]) for r in ix["refs"]][1] == 0 and ix["refs"][1]["pseudo"] is None and ix["refs"][1]["intv"] == []
    assert ix["refs"][0]["pseudo"][2:] == (11, 2) and ix["refs"][2]["pseudo"][2:] == (1, 1)
    assert len(ix["refs"][0]["intv"]) == (bii.MAX_END >> 14) and len(ix["refs"][2]["intv"]) == 6
    assert ix["refs"][2]["intv"][:5] == [ix["refs"][2]["pseudo"][0]] * 5                    # leading empty windows: the reference's first record's start
    i0 = ix["refs"][0]["intv"]; w = ((1 << 26) >> 14) + 2
    assert i0[w] == i0[w - 1] == i0[(1 << 26) >> 14] != i0[w + 3]                           # a later empty window: its predecessor's value
    for r in ix["refs"]:
        assert [b for b, _ in r["bins"]] == sorted(b for b, _ in r["bins"])                  # ascending bin numbers
    # the placed unmapped record is binned and counted, and its window is nobody's: window 1 (pos 20000) belongs to the record that crosses into it
    assert i0[1] == dict(zip([r[36:36 + r[12] - 1] for r in recs], [v for _, _, _, v in bii.walk(raw, sizes, first, n_chr)[2]]))[b"crosses_16k_by_one"]
    # offsets of 48 bits
    far = _check(exe, workdir, "far_again", *[CASES["main_far"][k] for k in (0, 1, 2)])[2]
    assert bii.parse_bai(far)["refs"][0]["pseudo"][0] >> 16 == 1 << 40 and len(far) == len(bai) and far != bai
    # merges and non-merges, a record that ends at a block's end, one that straddles
    n_chr, recs, first = CASES["spread"]
    raw, sizes, bai, refs, done = _check(exe, workdir, "spread_again", n_chr, recs, first)
    st = bii.twin_stats(raw, sizes, first, n_chr)
    assert st[3] > st[4] > st[2], st                                                        # some neighbours merged, some bins keep several chunks
    ends = {at + s for at, s in zip(bii.offsets(raw), [len(r) for r in recs])}
    assert bii.BLOCK in ends or 2 * bii.BLOCK in ends or 3 * bii.BLOCK in ends              # a record ends exactly at a block's end
    assert any(at // bii.BLOCK != (at + len(r) - 1) // bii.BLOCK for at, r in zip(bii.offsets(raw), recs))
    last_block_start = [v for _, _, _, v in bii.walk(raw, sizes, first, n_chr)[2]][-1]
    assert last_block_start & 0xFFFF == 0                                                   # the record behind it starts the next block: offset 0 inside it
    # empty, unplaced only
    assert len(bii.build_bai(b"", [], 99, 4)) == 8 + 8 * 4 + 8
    u = bii.parse_bai(bii.build_bai(b"".join(CASES["unplaced_only"][1]), [500], 77, 2))
    assert u["n_no_coor"] == 5 and all(not r["bins"] and r["pseudo"] is None for r in u["refs"])


def test_end_behind_2_29_is_refused_with_the_records_index(exe, workdir):
    n_chr, recs, first = CASES["main"]
    recs = list(recs)
    k = [r[36:36 + r[12] - 1] for r in recs].index(b"ends_at_2_29")
    recs[k] = bii.record(0, bii.MAX_END - 40, 0, b"ends_behind", [(41, bii.M)], l_seq=41)
    raw = b"".join(recs)
    got = bii.run_program(exe, workdir, "range", n_chr, raw, bii.stored_sizes(raw), first)
    assert got["bad"] == k and got["bytes"] == b""
    with pytest.raises(bii.RangeError) as x:
        bii.build_bai(raw, bii.stored_sizes(raw), first, n_chr)
    assert x.value.args[0] == k
    with pytest.raises(bii.RangeError):
        bii.build_bai(raw[:0], [], 1 << 48, n_chr)


def test_the_reader_finds_what_a_scan_finds_through_the_twins_index():
    """the definition is an index, not just a format: region queries through the index over real BGZF blocks"""
    rng = random.Random(7)
    for name in ("main", "spread"):
        n_chr, recs, first = CASES[name]
        raw = b"".join(recs)
        first = 4242
        bam, sizes = bii.fake_file(raw, first)
        bai = bii.build_bai(raw, sizes, first, n_chr)
        regions = [(t, 0, 1) for t in range(n_chr)] + [(0, 16383, 16385), (0, 16384, 16385), (0, bii.MAX_END - 1, bii.MAX_END), (0, (1 << 26) + 2 * 16384, (1 << 26) + 2 * 16384 + 9),
                                                       (0, 30000, 30001), (2 % n_chr, 0, 5 * 16384), (0, 0, bii.MAX_END)]
        for _ in range(150):
            t = rng.randrange(n_chr); b = rng.choice([rng.randrange(0, 120000), rng.randrange(0, bii.MAX_END)]); regions.append((t, b, b + rng.choice([1, 50, 20000, 1 << 20])))
        hits = 0
        for t, b, e in regions:
            want = bii.brute(raw, n_chr, t, b, min(e, bii.MAX_END))
            assert bii.query(bai, bam, t, b, min(e, bii.MAX_END)) == want, (name, t, b, e)
            hits += len(want)
        assert hits >= 30                                      # (the whole-reference region alone finds every mapped record of reference 0)


def test_build_bai_of_file_reads_sizes_and_records_from_the_file_alone():
    n_chr, recs, _ = CASES["spread"]
    raw = b"".join(recs)
    hdr = b"BAM\1" + struct.pack("<i", 4) + b"@CO\n" + struct.pack("<i", n_chr) + b"".join(struct.pack("<i", 2) + b"c\0" + struct.pack("<i", 1 << 20) for _ in range(n_chr))
    head, hs = bii.fake_file(hdr)
    body, sizes = bii.fake_file(raw)
    eof = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    assert bii.build_bai_of_file(head + body + eof) == bii.build_bai(raw, sizes, len(head), n_chr)
    assert bii.split_file(head + body + eof) == (len(head), sizes, raw, n_chr)


def test_lane_code_under_the_sanitizers(workdir):
    """the same program with AddressSanitizer and UBSan on its host code: every record walk stays inside the exact-size heap copy of the array, every store
    inside the exact-size index.  Stand-alone; never through python's process, never on the GPU."""
    exe = bii.build_program(workdir, sanitize=True)
    for name in sorted(CASES):
        n_chr, recs, first = CASES[name]
        raw = b"".join(recs)
        got = bii.run_program(exe, workdir, "san_" + name, n_chr, raw, bii.stored_sizes(raw), first)
        assert got["bytes"] == bii.build_bai(raw, bii.stored_sizes(raw), first, n_chr)
    # a last record whose CIGAR count points behind the array: the walk stops at the record's end
    n_chr, recs, first = CASES["one"]
    liar = bytearray(recs[0]); struct.pack_into("<H", liar, 16, 60000)
    got = bii.run_program(exe, workdir, "san_liar", n_chr, bytes(liar), [100], first)
    assert got["bad"] is None and len(got["recs"]) == 1
