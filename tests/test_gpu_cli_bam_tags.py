"""GPU suite: `dart -bo` with DART_DEVICE_BAM=1 DART_SORT_BAM=1 DART_BAM_TAGS=... -- the sorted file's records carry MD:Z, NM as edit distance and ts:A, written
on the device before the first piece is compressed -- against the sequential twin of tests/tags_inputs.py computed from the file written WITHOUT the switch and the
index's text alone; the index of the tagged file; what the switch needs and what it says about a word it does not know."""
import os, subprocess
import pytest
import common, bam_decode
import bamidx_inputs as bii
import bamsort_inputs as bsi
import pileup_inputs as pui
import tags_inputs as tgi
from dart_amd import synth, host

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
SWITCHES = ("DART_DEVICE_BAM", "DART_DEVICE_FASTQ", "DART_DEVICE_SAM", "DART_SORT_BAM", "DART_BAM_INDEX", "DART_BGZF_DYNAMIC", "DART_SORT_PIECE_MB", "DART_GPUS", "DART_COVERAGE",
            "DART_COVERAGE_EXCLUDE", "DART_COVERAGE_MIN_MAPQ", "DART_MARK_DUPLICATES", "DART_PILEUP", "DART_PILEUP_MIN_ALT", "DART_PILEUP_EXCLUDE", "DART_PILEUP_MIN_MAPQ", "DART_QC",
            "DART_QC_EXCLUDE", "DART_QC_MIN_MAPQ", "DART_BAM_TAGS")
INDEXED = {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_BAM_INDEX": "1"}


def _spawn(d, args, extra):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000", **extra)      # 4000 reads per batch: the case runs several batches
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


def _header_of(bam):
    """the file's bytes in front of the first record, inflated"""
    blocks = bam_decode.bgzf_blocks(bam)
    data = b"".join(b for b, _ in blocks)
    return data[:len(data) - len(bii.split_file(bam)[2])]


def test_dart_cli_tags_the_sorted_file(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("pe101_spliced", workdir)
    d = os.path.join(workdir, "tags_cli"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1); synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2)
    args = ["-i", c["prefix"], "-f", "1.fq", "-f2", "2.fq", "-j", "o.j", "-t", "4", "-mis", "5"]
    ref = pui.ref_of_index(host.Index(c["prefix"]))
    _, timing = _run(d, args + ["-bo", "plain.bam"], INDEXED)
    assert not any(" tags:" in l for l in timing)
    plain = _read(d, "plain.bam")
    raw = bii.split_file(plain)[2]
    assert all(tgi.md_of(x) is None and tgi.ts_of(x) is None for x in bsi.split(raw)[:200])
    # all three: the tagged file's records are the twin of the plain file's; the header is the same; the .bai is the index twin of the tagged file
    _, timing = _run(d, args + ["-bo", "all.bam"], dict(INDEXED, DART_BAM_TAGS="all"))
    bam = _read(d, "all.bam")
    first, sizes, got, n_chr = bii.split_file(bam)
    want, st = tgi.twin(raw, ref, tgi.ALL)
    assert got == want and _header_of(bam) == _header_of(plain)
    assert st[0] > 1000 and st[4] > 500 and st[6] > 20 and st[3] == st[0]
    assert _read(d, "all.bam.bai") == bii.build_bai(got, sizes, first, n_chr) != _read(d, "plain.bam.bai")
    note = [l for l in timing if l.startswith("[dart timing] tags:")]
    assert len(note) == 1 and ("%d records rewritten, %d + %d copied" % st[:3]) in note[0] and ("%d mismatches, %d inserted + deleted bases, %d ts written" % st[4:7]) in note[0], timing
    assert ("%d raw bytes" % len(want)) in note[0] and "length pass" in note[0] and "write pass" in note[0]
    bam_decode.decode(bam)                                                  # an independent reader takes the file: every integer tag in its smallest type, every Z with its NUL
    # a list in any order; one word (1 for all: tests/native/dart_config_tags_checks.cpp)
    _run(d, args + ["-bo", "list.bam"], dict(INDEXED, DART_BAM_TAGS="ts,MD,NM"))
    assert _read(d, "list.bam") == bam
    _run(d, args + ["-bo", "md.bam"], {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_BAM_TAGS": "MD"})
    got_md = bii.split_file(_read(d, "md.bam"))[2]
    assert got_md == tgi.twin(raw, ref, tgi.MD_)[0] and not os.path.exists(os.path.join(d, "md.bam.bai"))
    recs = bsi.split(got_md)
    assert sum(1 for x in recs if tgi.md_of(x) is not None) == st[0] and all(tgi.ts_of(x) is None for x in recs)
    assert all(tgi.tags_of(x)[b"NM"][0][:1] in (b"C", b"S") and list(tgi.tags_of(x))[0] == b"NM" for x in recs if tgi.md_of(x) is not None)     # the mapper's NM stays where it was


def test_dart_cli_tags_switch_says_what_is_wrong(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("se100", workdir)
    d = os.path.join(workdir, "tags_missing"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    args = ["-i", c["prefix"], "-f", "1.fq", "-j", "o.j", "-t", "4"] + c["runs"][0]["flags"]
    sorted_ = {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1"}
    for k, (value, word) in enumerate((("MD,XS", "XS"), ("md", "md"), ("MD,,NM", ""), ("2", "2"), ("", ""), ("NM;MD", "NM;MD"))):
        r = _spawn(d, args + ["-bo", "w%d.bam" % k], dict(sorted_, DART_BAM_TAGS=value))
        err = r.stderr.decode("latin1").splitlines()
        assert r.returncode == 1 and len(err) == 1 and err[0].startswith("Error! DART_BAM_TAGS=%s: \"%s\" is none of MD, NM, ts" % (value, word)), (r.returncode, err)
        assert not os.path.exists(os.path.join(d, "w%d.bam" % k))
    for out, extra in ((["-bo", "a.bam"], {"DART_BAM_TAGS": "all", "DART_DEVICE_BAM": "1"}), (["-bo", "b.bam"], {"DART_BAM_TAGS": "MD"}), (["-o", "c.sam"], {"DART_BAM_TAGS": "1"})):
        r = _spawn(d, args + out, extra)
        err = r.stderr.decode("latin1").splitlines()
        assert r.returncode == 1 and len(err) == 1 and err[0] == "Error! DART_BAM_TAGS=%s needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing" % extra["DART_BAM_TAGS"], (r.returncode, err)
        assert not os.path.exists(os.path.join(d, out[1]))
    # with the sort asked for but not possible, the sort's own message comes first
    r = _spawn(d, args + ["-bo", "e.bam"], {"DART_BAM_TAGS": "all", "DART_SORT_BAM": "1"})
    assert r.returncode == 1 and "DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1" in r.stderr.decode("latin1") and not os.path.exists(os.path.join(d, "e.bam"))
