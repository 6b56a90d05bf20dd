"""GPU suite: `dart` with DART_DEVICE_SAM=1 -- the SAM text formatted on the device (dg_batch_format_sam) in both host pipelines -- against the reference's
golden SAM, junctions and statistics; the DART_TIMING line must name the formatter that ran, so a silent fall-back to the host's cannot pass."""
import gzip, os, subprocess
import pytest
import common
from dart_amd import synth

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
PIPELINES = {"parallel": {}, "streaming": {"DART_STREAMING": "1"}}


def _run(d, args, extra):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000", **extra)      # 4000 reads per batch: every case runs several batches
    r = subprocess.run([DART] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, r.stderr[-600:]
    timing = [l for l in r.stderr.decode("latin1").splitlines() if l.startswith("[dart timing]")]
    assert timing, r.stderr[-600:]
    return r, timing[-1]


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_dart_cli_device_sam_reproduces_golden_sam(pipeline, workdir):
    import __graft_entry__ as ge
    ge.build()
    for name in sorted(common.MANIFEST["cases"]):
        c = common.build_case(name, workdir)
        d = os.path.join(workdir, "devsam_%s_%s" % (pipeline, name)); os.makedirs(d, exist_ok=True)
        synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
        files = ["-f", "1.fq"]
        if c["spec"]["paired"]:
            synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2); files += ["-f2", "2.fq"]
        for run in c["runs"]:
            r, timing = _run(d, ["-i", c["prefix"]] + files + ["-o", "o.sam", "-j", "o.j", "-t", "4"] + run["flags"], dict(PIPELINES[pipeline], DART_DEVICE_SAM="1"))
            assert "format=device" in timing and "format=host" not in timing, timing
            got, want = open(os.path.join(d, "o.sam")).read(), common.golden_sam(run["base"])
            assert got == want, common.first_diff(got, want)
            assert open(os.path.join(d, "o.j")).read() == common.golden_junctions(run["base"])
            assert common.stats_block(r.stdout) == common.golden_stats(run["base"]), (run["base"], r.stdout[-600:])
        # without the switch the host's formatter runs, and says so
        r, timing = _run(d, ["-i", c["prefix"]] + files + ["-o", "h.sam", "-j", "h.j", "-t", "4"] + c["runs"][0]["flags"], PIPELINES[pipeline])
        assert "format=host" in timing and "format=device" not in timing, timing
        assert open(os.path.join(d, "h.sam")).read() == common.golden_sam(c["runs"][0]["base"])


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_dart_cli_device_sam_on_reads_with_odd_characters(pipeline, workdir):
    c = common.build_case("pe101_spliced", workdir)
    seqs = common.odd_character_reads(c["genome"])
    d = os.path.join(workdir, "devsam_odd_" + pipeline); os.makedirs(d, exist_ok=True)
    common.write_se_fastq(os.path.join(d, "odd.fq"), seqs)
    r, timing = _run(d, ["-i", c["prefix"], "-f", "odd.fq", "-mis", "12", "-o", "o.sam", "-j", "o.j", "-t", "4"], dict(PIPELINES[pipeline], DART_DEVICE_SAM="1"))
    assert "format=device" in timing, timing
    got, want = open(os.path.join(d, "o.sam")).read(), gzip.open(os.path.join(common.GOLDEN, "odd_characters.mis12.sam.gz"), "rt").read()
    assert got == want, common.first_diff(got, want)
    assert open(os.path.join(d, "o.j")).read() == open(os.path.join(common.GOLDEN, "odd_characters.mis12.junctions.tab")).read()


def test_dart_cli_bam_output_ignores_the_switch(workdir):
    """-bo: BAM is built from the host formatter's text; the switch changes nothing and the timing line says format=host"""
    c = common.build_case("se100", workdir)
    d = os.path.join(workdir, "devsam_bam"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    args = ["-i", c["prefix"], "-f", "1.fq", "-j", "o.j", "-t", "3"] + c["runs"][0]["flags"]
    r1, timing = _run(d, args + ["-bo", "a.bam"], {"DART_DEVICE_SAM": "1"})
    assert "format=host" in timing, timing
    _run(d, args + ["-bo", "b.bam"], {})
    assert open(os.path.join(d, "a.bam"), "rb").read() == open(os.path.join(d, "b.bam"), "rb").read()
