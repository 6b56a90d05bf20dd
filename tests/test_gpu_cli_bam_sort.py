"""GPU suite: `dart -bo` with DART_DEVICE_BAM=1 DART_SORT_BAM=1 -- the records of every batch stay in HBM, are sorted once at the end and written in
coordinate order -- against the same run without DART_SORT_BAM, stable-sorted here by (index of RNAME in the header with `*` last, POS, FLAG & 16); the
golden statistics and junctions; what the switch needs, and what it says when that is missing."""
import os, subprocess
import pytest
import common, bam_decode
from dart_amd import synth

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
SWITCHES = ("DART_DEVICE_BAM", "DART_DEVICE_FASTQ", "DART_DEVICE_SAM", "DART_SORT_BAM", "DART_BGZF_DYNAMIC", "DART_SORT_PIECE_MB", "DART_GPUS")


def _spawn(d, args, extra):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000", **extra)      # 4000 reads per batch: every case runs several batches
    for k in SWITCHES:
        if k not in extra:
            env.pop(k, None)
    return subprocess.run([DART] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def _run(d, args, extra):
    r = _spawn(d, args, extra)
    assert r.returncode == 0, r.stderr[-600:]
    timing = [l for l in r.stderr.decode("latin1").splitlines() if l.startswith("[dart timing]")]
    assert timing, r.stderr[-600:]
    return r, timing


def _decode(path):
    hdr, refs, lines, bins = bam_decode.decode(open(path, "rb").read())      # (asserts the end-of-file block, and that the header has a block of its own)
    return hdr, [n for n, _ in refs], lines


def _sort_key(names):
    tid = {n: i for i, n in enumerate(names)}
    def key(line):
        f = line.split("\t")
        return (tid.get(f[2], len(names)) if f[2] != "*" else len(names), int(f[3]), int(f[1]) & 16)
    return key


@pytest.mark.parametrize("name", ["pe101_spliced", "se100"])
def test_dart_cli_sorted_bam_is_the_stable_sort_of_the_unsorted_file(name, workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case(name, workdir)
    d = os.path.join(workdir, "sortbam_" + name); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    files = ["-f", "1.fq"]
    if c["spec"]["paired"]:
        synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2); files += ["-f2", "2.fq"]
    run = c["runs"][0]
    args = ["-i", c["prefix"]] + files + ["-j", "o.j", "-t", "4"] + run["flags"]
    # today's file: read order
    r0, _ = _run(d, args + ["-bo", "plain.bam"], {"DART_DEVICE_BAM": "1"})
    hdr0, names, plain = _decode(os.path.join(d, "plain.bam"))
    key = _sort_key(names)
    want = sorted(plain, key=key)
    assert want != plain, "the unsorted file is in order already"
    # the switch
    r, timing = _run(d, args + ["-bo", "sorted.bam"], {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1"})
    assert all("bam=device+sorted" in t for t in timing) and len(timing) >= 2, timing
    assert "merge + finish" in timing[-1] and "compress + download + write" in timing[-1], timing[-1]
    hdr, _, lines = _decode(os.path.join(d, "sorted.bam"))
    assert hdr == "@HD\tVN:1.6\tSO:coordinate\n" + hdr0
    assert lines == want
    assert open(os.path.join(d, "o.j")).read() == common.golden_junctions(run["base"])
    assert common.stats_block(r.stdout) == common.golden_stats(run["base"]) == common.stats_block(r0.stdout), r.stdout[-600:]
    default_bytes = open(os.path.join(d, "sorted.bam"), "rb").read()
    # the resident form: the same file content
    r, timing = _run(d, args + ["-bo", "both.bam"], {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_DEVICE_FASTQ": "1"})
    assert "assemble=device" in timing[0] and "bam=device+sorted" in timing[0], timing
    assert _decode(os.path.join(d, "both.bam")) == (hdr, names, lines)
    assert common.stats_block(r.stdout) == common.golden_stats(run["base"])
    # dynamic codes: the same records
    r, timing = _run(d, args + ["-bo", "dyn.bam"], {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_BGZF_DYNAMIC": "1"})
    assert "bam=device+sorted+dyn" in timing[-1], timing
    assert _decode(os.path.join(d, "dyn.bam")) == (hdr, names, lines)
    assert os.path.getsize(os.path.join(d, "dyn.bam")) < len(default_bytes)
    # the smallest piece: the same file bytes
    r, timing = _run(d, args + ["-bo", "piece.bam"], {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_SORT_PIECE_MB": "0"})
    assert "pieces of 65280 bytes" in timing[-1], timing[-1]
    assert open(os.path.join(d, "piece.bam"), "rb").read() == default_bytes


def test_dart_cli_sort_switch_says_what_is_missing(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("se100", workdir)
    d = os.path.join(workdir, "sortbam_missing"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    args = ["-i", c["prefix"], "-f", "1.fq", "-j", "o.j", "-t", "4"] + c["runs"][0]["flags"]
    for out, extra, word in ((["-bo", "a.bam"], {"DART_SORT_BAM": "1"}, "DART_DEVICE_BAM=1 is missing"),
                             (["-o", "b.sam"], {"DART_SORT_BAM": "1", "DART_DEVICE_BAM": "1"}, "-bo is missing"),
                             (["-o", "c.sam"], {"DART_SORT_BAM": "1"}, "both are missing")):
        r = _spawn(d, args + out, extra)
        err = r.stderr.decode("latin1").splitlines()
        assert r.returncode == 1 and len(err) == 1 and "DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1" in err[0] and word in err[0], (r.returncode, err)
        assert not os.path.exists(os.path.join(d, out[1]))
