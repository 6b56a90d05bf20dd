"""GPU suite: `dart -bo` with DART_DEVICE_BAM=1 DART_SORT_BAM=1 DART_MARK_DUPLICATES=1 -- flag 0x400 is written into the sorted records on the device before
the file is compressed -- against the sequential twin of tests/markdup_inputs.py computed from the unmarked file alone (decoded with tests/bam_decode.py); the
index and the coverage track see the marks; what the switch needs, what it says when that is missing, and that nothing changes without it."""
import os, subprocess
import pytest
import common, bam_decode
import bamidx_inputs as bii
import coverage_inputs as cvi
import markdup_inputs as mdi

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
SWITCHES = ("DART_DEVICE_BAM", "DART_DEVICE_FASTQ", "DART_DEVICE_SAM", "DART_SORT_BAM", "DART_BAM_INDEX", "DART_BGZF_DYNAMIC", "DART_SORT_PIECE_MB", "DART_GPUS", "DART_COVERAGE",
            "DART_COVERAGE_EXCLUDE", "DART_COVERAGE_MIN_MAPQ", "DART_MARK_DUPLICATES", "DG_MARKDUP_HASH_BITS")
SORTED = {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1"}
N_COPIES = 300


def _spawn(d, args, extra):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="400", **extra)       # 400 reads per batch: several batches, the copies in the last ones
    for k in SWITCHES:
        if k not in extra:
            env.pop(k, None)
    return subprocess.run([DART] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def _run(d, args, extra):
    r = _spawn(d, args, extra)
    assert r.returncode == 0, r.stderr[-600:]
    return r, [l for l in r.stderr.decode("latin1").splitlines() if l.startswith("[dart timing]")]


def _read(d, name):
    return open(os.path.join(d, name), "rb").read()


def _write_fastq(path, seqs, mate):
    """the case's reads, then the first N_COPIES again under other names with every quality one lower"""
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b"@r%d/%d\n" % (i, mate) + s.tobytes() + b"\n+\n" + b"I" * len(s) + b"\n")
        for i, s in enumerate(seqs[:N_COPIES]):
            f.write(b"@copy%d/%d\n" % (i, mate) + s.tobytes() + b"\n+\n" + b"H" * len(s) + b"\n")


def test_dart_cli_marks_the_duplicates_of_the_sorted_file(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("pe101_spliced", workdir)
    d = os.path.join(workdir, "md_cli"); os.makedirs(d, exist_ok=True)
    _write_fastq(os.path.join(d, "1.fq"), c["m1"], 1); _write_fastq(os.path.join(d, "2.fq"), c["m2"], 2)
    args = ["-i", c["prefix"], "-f", "1.fq", "-f2", "2.fq", "-j", "o.j", "-t", "4"] + c["runs"][0]["flags"]
    # without the switch: no counts, no line
    _, timing = _run(d, args + ["-bo", "plain.bam"], SORTED)
    assert not os.path.exists(os.path.join(d, "plain.bam.markdup.txt")) and not any("markdup" in l for l in timing)
    plain = _read(d, "plain.bam")
    first, _, raw, n_chr = bii.split_file(plain)
    assert not any(flag & mdi.DUP for _, flag in mdi.flags_by_name(raw))
    want, stats, _ = mdi.twin(raw, n_chr)
    assert stats[3] >= 1 and stats[4] >= 1 and stats[6] == 2 * stats[3] + stats[4]          # (how many of the copies map with both mates is the mapper's business)
    # with it: the same file but for the bits the twin predicts
    _, timing = _run(d, args + ["-bo", "marked.bam"], dict(SORTED, DART_MARK_DUPLICATES="1"))
    marked = _read(d, "marked.bam")
    first2, _, raw2, n_chr2 = bii.split_file(marked)
    assert (first2, n_chr2) == (first, n_chr) and raw2 == want and raw2 != raw
    h0, h1 = bam_decode.decode(plain), bam_decode.decode(marked)
    assert h0[0] == h1[0] and h0[1] == h1[1] and h0[3] == h1[3]   # the header's text and references, the records' bins
    differ = [(a.split("\t"), b.split("\t")) for a, b in zip(h0[2], h1[2]) if a != b]
    assert len(h0[2]) == len(h1[2]) and len(differ) == stats[6]
    assert all(int(b[1]) == int(a[1]) | mdi.DUP and a[:1] + a[2:] == b[:1] + b[2:] for a, b in differ)
    assert _read(d, "marked.bam.markdup.txt") == b"".join(b"%s\t%d\n" % (k, v) for k, v in zip(
        (b"examined_records", b"pairs", b"fragments", b"duplicate_pairs", b"duplicate_fragments", b"candidates_in_crowded_runs", b"records_marked_duplicate", b"largest_family"), stats))
    note = [l for l in timing if l.startswith("[dart timing] markdup:")]
    assert len(note) == 1 and ("%d records marked" % stats[6]) in note[0], timing
    copies = {nm for nm, flag in mdi.flags_by_name(raw2) if flag & mdi.DUP}
    assert any(nm.startswith(b"copy") for nm in copies)
    # the index and the track of the marked file
    _, timing = _run(d, args + ["-bo", "all.bam"], dict(SORTED, DART_MARK_DUPLICATES="1", DART_BAM_INDEX="1", DART_COVERAGE="1"))
    assert _read(d, "all.bam") == marked and _read(d, "all.bam.markdup.txt") == _read(d, "marked.bam.markdup.txt")
    assert _read(d, "all.bam.bai") == bii.build_bai_of_file(marked)
    names = [n.encode() if isinstance(n, str) else n for n, _ in h1[1]]
    ent, st = cvi.twin(want, n_chr)
    assert _read(d, "all.bam.bedgraph") == cvi.text_of(ent, names)
    assert st[0] == cvi.twin(raw, n_chr)[1][0] - stats[6]          # the track leaves the duplicates out


def test_dart_cli_markdup_switch_says_what_is_missing(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("se100", workdir)
    d = os.path.join(workdir, "md_missing"); os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "1.fq"), "wb") as f:
        for i, s in enumerate(c["m1"][:50]):
            f.write(b"@r%d/1\n" % i + s.tobytes() + b"\n+\n" + b"I" * len(s) + b"\n")
    args = ["-i", c["prefix"], "-f", "1.fq", "-j", "o.j", "-t", "4"] + c["runs"][0]["flags"]
    for out, extra in ((["-bo", "a.bam"], {"DART_MARK_DUPLICATES": "1", "DART_DEVICE_BAM": "1"}), (["-bo", "b.bam"], {"DART_MARK_DUPLICATES": "1"}), (["-o", "c.sam"], {"DART_MARK_DUPLICATES": "1"})):
        r = _spawn(d, args + out, extra)
        err = r.stderr.decode("latin1").splitlines()
        assert r.returncode == 1 and len(err) == 1 and err[0].startswith("Error! DART_MARK_DUPLICATES=1 needs DART_SORT_BAM=1") and "-bo and DART_DEVICE_BAM=1" in err[0], (r.returncode, err)
        assert not os.path.exists(os.path.join(d, out[1])) and not os.path.exists(os.path.join(d, out[1] + ".markdup.txt"))
