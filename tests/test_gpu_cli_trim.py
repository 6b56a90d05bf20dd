"""GPU suite: `dart` with the DART_TRIM_* switches -- adapters, poly tails and low-quality ends cut on the device inside the FASTQ upload -- on a golden paired
library with adapter read-through laid over it: the SAM body (with -o) and the BAM records (with -bo) must be those `dart` without the switches gives on the
files the twin (tests/trim_inputs.py) wrote after trimming, <out>.trim.txt must hold the twin's sums over batches and libraries, and a job that could only map
untrimmed reads is refused."""
import os, subprocess
import pytest
import common, bam_decode
import sam_device_inputs as sdi
import trim_inputs as ti

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
TRIM = {"DART_TRIM_ADAPTER": "illumina", "DART_TRIM_QUAL": "20", "DART_TRIM_POLY": "G", "DART_TRIM_MIN_LEN": "20"}
P = ti.params(flags=ti.PAIRS, qual3=20, poly_mask=ti.poly_mask("G"), min_len=20, adapter=(ti.ADAPTERS["illumina"], ti.ADAPTERS["illumina"]))
DEV = {"-o": {"DART_DEVICE_FASTQ": "1", "DART_DEVICE_SAM": "1"}, "-bo": {"DART_DEVICE_FASTQ": "1", "DART_DEVICE_BAM": "1"}}


@pytest.fixture(scope="module")
def library(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("pe101_spliced", workdir)
    d = os.path.join(workdir, "cli_trim"); os.makedirs(d, exist_ok=True)
    def text(m, seed, tag):
        return b"".join(b"@r%d/%d\n%s\n+\n%s\n" % (i, tag, s, q) for i, (s, q) in enumerate(ti.spoil(m, seed, ti.ADAPTERS["illumina"] + b"ACACGTCTGAACTCCAGTCAC")))
    t1, t2 = text(c["m1"], 41, 1), text(c["m2"], 42, 2)
    kept, stats, wins, idx, plain = ti.trim_batch(ti.records(t1, t2), P, True, True)
    assert stats[5] > 0 and stats[6] > 0 and stats[7] > 0 and stats[9] > 0 and stats[12] > 0 and stats[1] < stats[0]
    w1, w2 = ti.fastq_of(plain, True)
    lines = t1.split(b"\n")
    stop = b"\n".join(lines[:4 * 20]) + b"\n@empty\n\n+\n\n" + b"\n".join(lines[4 * 20:4 * 40]) + b"\n"
    for name, data in (("1.fq", t1), ("2.fq", t2), ("t1.fq", w1), ("t2.fq", w2), ("stop.fq", stop)):
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    return c, d, stats


def _run(d, args, extra, ok=True):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000", **extra)
    r = subprocess.run([DART] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert (r.returncode == 0) == ok, r.stderr[-800:]
    return r


@pytest.mark.parametrize("out", ["-o", "-bo"])
def test_dart_cli_trim_equals_dart_on_the_twin_trimmed_files(out, library):
    c, d, stats = library
    ext = "sam" if out == "-o" else "bam"
    flags = ["-t", "4"] + c["runs"][1]["flags"]
    # two libraries (the same files twice): the sums run over batches and libraries
    r = _run(d, ["-i", c["prefix"], "-f", "1.fq", "1.fq", "-f2", "2.fq", "2.fq", out, "got." + ext, "-j", "got.j"] + flags, dict(DEV[out], **TRIM))
    w = _run(d, ["-i", c["prefix"], "-f", "t1.fq", "t1.fq", "-f2", "t2.fq", "t2.fq", out, "want." + ext, "-j", "want.j"] + flags, DEV[out])
    got, want = open(os.path.join(d, "got." + ext), "rb").read(), open(os.path.join(d, "want." + ext), "rb").read()
    if out == "-o":
        got, want = sdi.body_of(got.decode("latin1")).decode("latin1"), sdi.body_of(want.decode("latin1")).decode("latin1")
        assert got == want, common.first_diff(got, want)
        assert len(got.splitlines()) >= 2 * stats[1]
    else:
        g, w_ = bam_decode.decode(got), bam_decode.decode(want)
        assert g[1] == w_[1] and g[2] == w_[2] and len(g[2]) >= 2 * stats[1]
    assert open(os.path.join(d, "got.j")).read() == open(os.path.join(d, "want.j")).read()
    assert common.stats_block(r.stdout) == common.stats_block(w.stdout)                  # the statistics block counts what the mapper saw
    lines = open(os.path.join(d, "got.%s.trim.txt" % ext)).read().splitlines()
    assert lines == ["%s\t%d" % (k, 2 * v) for k, v in zip(ti.STAT_KEYS[:14], stats[:14])]
    assert not os.path.exists(os.path.join(d, "want.%s.trim.txt" % ext))
    timing = [l for l in r.stderr.decode("latin1").splitlines() if l.startswith("[dart trim]")]
    assert timing and "reads_in=%d reads_kept=%d " % (2 * stats[0], 2 * stats[1]) in timing[-1], r.stderr[-600:]


def test_dart_cli_trim_refuses_what_would_map_untrimmed_reads(library):
    c, d, stats = library
    args = ["-i", c["prefix"], "-f", "1.fq", "-f2", "2.fq", "-j", "no.j", "-t", "4"]
    for out, env, word in (("-o", {"DART_DEVICE_FASTQ": "1"}, "DART_DEVICE_SAM=1 is missing"), ("-o", {"DART_DEVICE_SAM": "1"}, "DART_DEVICE_FASTQ=1 is missing"),
                           ("-bo", {"DART_DEVICE_FASTQ": "1"}, "DART_DEVICE_BAM=1 is missing"), ("-o", {}, "DART_DEVICE_FASTQ=1 is missing")):
        r = _run(d, args + [out, "no.out"], dict(env, **TRIM), ok=False)
        err = r.stderr.decode("latin1")
        assert r.returncode == 1 and err.startswith("Error! DART_TRIM_* needs the device parser and a device formatter") and word in err and err.count("\n") == 1, err
        assert not os.path.exists(os.path.join(d, "no.out")) and not os.path.exists(os.path.join(d, "no.out.trim.txt"))
    # a library that falls back to the host's assembly (a record without bases): refused when its turn comes, no statistics are left
    r = _run(d, ["-i", c["prefix"], "-f", "stop.fq", "-o", "stop.sam", "-j", "stop.j", "-t", "4"], dict(DEV["-o"], **TRIM), ok=False)
    err = r.stderr.decode("latin1")
    assert "DART_TRIM_*" in err and "host's assembly" in err, err
    assert not os.path.exists(os.path.join(d, "stop.sam.trim.txt"))
    # the same file without the switches maps
    _run(d, ["-i", c["prefix"], "-f", "stop.fq", "-o", "stop.sam", "-j", "stop.j", "-t", "4"], DEV["-o"])
