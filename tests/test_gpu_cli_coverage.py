"""GPU suite: `dart -bo` with DART_DEVICE_BAM=1 DART_SORT_BAM=1 DART_COVERAGE=1 (or 2) -- the sorted file's coverage track is built on the device and written
beside it -- against the sequential twin of tests/coverage_inputs.py computed from the BAM file alone (decoded with tests/bam_decode.py); what the switch needs,
what it says when that is missing, and that nothing changes without it."""
import os, subprocess
import pytest
import common, bam_decode
import bamidx_inputs as bii
import coverage_inputs as cvi
from dart_amd import synth

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
SWITCHES = ("DART_DEVICE_BAM", "DART_DEVICE_FASTQ", "DART_DEVICE_SAM", "DART_SORT_BAM", "DART_BAM_INDEX", "DART_BGZF_DYNAMIC", "DART_SORT_PIECE_MB", "DART_GPUS", "DART_COVERAGE",
            "DART_COVERAGE_EXCLUDE", "DART_COVERAGE_MIN_MAPQ")
INDEXED = {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_BAM_INDEX": "1"}
TRACKS = (".bedgraph", ".plus.bedgraph", ".minus.bedgraph")


def _spawn(d, args, extra):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000", **extra)      # 4000 reads per batch: every case runs several batches
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


def _tracks(d, out):
    return [t for t in TRACKS if os.path.exists(os.path.join(d, out + t))]


@pytest.mark.parametrize("name", ["pe101_spliced", "se100"])
def test_dart_cli_writes_the_coverage_of_the_sorted_file(name, workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case(name, workdir)
    d = os.path.join(workdir, "cov_" + name); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    files = ["-f", "1.fq"]
    if c["spec"]["paired"]:
        synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2); files += ["-f2", "2.fq"]
    run = c["runs"][0]
    args = ["-i", c["prefix"]] + files + ["-j", "o.j", "-t", "4"] + run["flags"]
    # the sorted, indexed file without the switch: no track, and the same BAM and .bai bytes with it
    _, timing = _run(d, args + ["-bo", "plain.bam"], INDEXED)
    assert _tracks(d, "plain.bam") == [] and not any("coverage" in l for l in timing)
    r, timing = _run(d, args + ["-bo", "one.bam"], dict(INDEXED, DART_COVERAGE="1"))
    assert _tracks(d, "one.bam") == [".bedgraph"]
    bam = _read(d, "one.bam")
    assert bam == _read(d, "plain.bam") and _read(d, "one.bam.bai") == _read(d, "plain.bam.bai")
    _, _, raw, n_chr = bii.split_file(bam)
    names = [n.encode() if isinstance(n, str) else n for n, _ in bam_decode.decode(bam)[1]]
    assert len(names) == n_chr
    ent, st = cvi.twin(raw, n_chr)
    track = _read(d, "one.bam.bedgraph")
    assert track == cvi.text_of(ent, names) and st[3] > 500
    note = [l for l in timing if l.startswith("[dart timing] coverage:")]
    assert len(note) == 1 and ("1 tracks, %d entries, %d bytes" % (st[3], len(track))) in note[0], timing
    assert open(os.path.join(d, "o.j")).read() == common.golden_junctions(run["base"])
    assert common.stats_block(r.stdout) == common.golden_stats(run["base"]), r.stdout[-600:]
    # one track per strand, with the filter's two variables (no index asked for: none written)
    _run(d, args + ["-bo", "two.bam"], {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_COVERAGE": "2", "DART_COVERAGE_EXCLUDE": "0x304", "DART_COVERAGE_MIN_MAPQ": "2"})
    assert _tracks(d, "two.bam") == [".plus.bedgraph", ".minus.bedgraph"] and _read(d, "two.bam") == bam and not os.path.exists(os.path.join(d, "two.bam.bai"))
    both, plus, minus = (cvi.twin(raw, n_chr, exclude=0x304, min_mapq=2, strand=s) for s in (None, "+", "-"))
    assert _read(d, "two.bam.plus.bedgraph") == cvi.text_of(plus[0], names) and _read(d, "two.bam.minus.bedgraph") == cvi.text_of(minus[0], names)
    assert plus[1][5] + minus[1][5] == both[1][5] and plus[1][0] > 0 and minus[1][0] > 0 and 0 < both[1][0] < st[0]


def test_dart_cli_coverage_switch_says_what_is_missing(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("se100", workdir)
    d = os.path.join(workdir, "cov_missing"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    args = ["-i", c["prefix"], "-f", "1.fq", "-j", "o.j", "-t", "4"] + c["runs"][0]["flags"]
    for out, extra in ((["-bo", "a.bam"], {"DART_COVERAGE": "1", "DART_DEVICE_BAM": "1"}), (["-bo", "b.bam"], {"DART_COVERAGE": "2"}), (["-o", "c.sam"], {"DART_COVERAGE": "1"})):
        r = _spawn(d, args + out, extra)
        err = r.stderr.decode("latin1").splitlines()
        assert r.returncode == 1 and len(err) == 1 and err[0].startswith("Error! DART_COVERAGE=%s needs DART_SORT_BAM=1" % extra["DART_COVERAGE"]) and "-bo and DART_DEVICE_BAM=1" in err[0], (r.returncode, err)
        assert not os.path.exists(os.path.join(d, out[1])) and _tracks(d, out[1]) == []
    # a value that is neither 1 nor 2
    r = _spawn(d, args + ["-bo", "f.bam"], {"DART_COVERAGE": "3", "DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1"})
    assert r.returncode == 1 and "DART_COVERAGE=3" in r.stderr.decode("latin1") and not os.path.exists(os.path.join(d, "f.bam")) and _tracks(d, "f.bam") == []
    # with the sort asked for but not possible, the sort's own message comes first
    r = _spawn(d, args + ["-bo", "e.bam"], {"DART_COVERAGE": "1", "DART_SORT_BAM": "1"})
    assert r.returncode == 1 and "DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1" in r.stderr.decode("latin1") and not os.path.exists(os.path.join(d, "e.bam")) and _tracks(d, "e.bam") == []
