"""GPU suite: `dart` with DART_DEVICE_SJ=1 -- the junction table counted, sorted and printed on the device (dg_batch_accumulate_sj, dg_sj_merge,
dg_sj_finish) in both host pipelines -- against the reference's golden junctions, SAM and statistics; the `[dart sj]` line must name the table that ran,
so a silent fall-back to the host's map cannot pass."""
import os, re, subprocess
import pytest
import common, cli_inputs
from dart_amd import synth

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
PIPELINES = {"parallel": {}, "streaming": {"DART_STREAMING": "1"}}


def _run(d, args, extra):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000")      # 4000 reads per batch: every case runs several batches
    env.update(extra)
    r = subprocess.run([DART] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, r.stderr[-600:]
    lines = [l for l in r.stderr.decode("latin1").splitlines() if l.startswith("[dart sj]")]
    assert len(lines) == 1, r.stderr[-600:]
    return r, lines[0]


def _tuples(line):
    return int(re.search(r"tuples=(\d+)", line).group(1))


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_dart_cli_device_sj_reproduces_golden_junctions(pipeline, workdir):
    import __graft_entry__ as ge
    ge.build()
    for name in sorted(common.MANIFEST["cases"]):
        c = common.build_case(name, workdir)
        d = os.path.join(workdir, "devsj_%s_%s" % (pipeline, name)); os.makedirs(d, exist_ok=True)
        synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
        files = ["-f", "1.fq"]
        if c["spec"]["paired"]:
            synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2); files += ["-f2", "2.fq"]
        for run in c["runs"]:
            r, sj = _run(d, ["-i", c["prefix"]] + files + ["-o", "o.sam", "-j", "o.j", "-t", "4"] + run["flags"], dict(PIPELINES[pipeline], DART_DEVICE_SJ="1"))
            assert "table=device" in sj and "table=host" not in sj and "finish_ms=" in sj, sj
            assert (_tuples(sj) > 0) == (c["spec"]["spliced"] > 0), sj
            assert open(os.path.join(d, "o.j")).read() == common.golden_junctions(run["base"]), run["base"]
            got, want = open(os.path.join(d, "o.sam")).read(), common.golden_sam(run["base"])
            assert got == want, common.first_diff(got, want)
            assert common.stats_block(r.stdout) == common.golden_stats(run["base"]), (run["base"], r.stdout[-600:])
        # without the switch the host's map runs, and says so
        r, sj = _run(d, ["-i", c["prefix"]] + files + ["-o", "h.sam", "-j", "h.j", "-t", "4"] + c["runs"][0]["flags"], PIPELINES[pipeline])
        assert "table=host" in sj and "table=device" not in sj and "map_s=" in sj, sj
        assert open(os.path.join(d, "h.j")).read() == common.golden_junctions(c["runs"][0]["base"])


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_dart_cli_device_sj_on_reads_with_odd_characters(pipeline, workdir):
    c = common.build_case("pe101_spliced", workdir)
    seqs = common.odd_character_reads(c["genome"])
    d = os.path.join(workdir, "devsj_odd_" + pipeline); os.makedirs(d, exist_ok=True)
    common.write_se_fastq(os.path.join(d, "odd.fq"), seqs)
    r, sj = _run(d, ["-i", c["prefix"], "-f", "odd.fq", "-mis", "12", "-o", "o.sam", "-j", "o.j", "-t", "4"], dict(PIPELINES[pipeline], DART_DEVICE_SJ="1"))
    assert "table=device" in sj and _tuples(sj) > 0, sj
    assert open(os.path.join(d, "o.j")).read() == open(os.path.join(common.GOLDEN, "odd_characters.mis12.junctions.tab")).read()


def test_dart_cli_device_sj_with_bam_output(workdir):
    """-bo: the junction file and the BAM are those of a run without the switch"""
    c = common.build_case("pe101_spliced", workdir)
    d = os.path.join(workdir, "devsj_bam"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1); synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2)
    run = c["runs"][0]
    args = ["-i", c["prefix"], "-f", "1.fq", "-f2", "2.fq", "-t", "3"] + run["flags"]
    r, sj = _run(d, args + ["-bo", "a.bam", "-j", "a.j"], {"DART_DEVICE_SJ": "1"})
    assert "table=device" in sj and _tuples(sj) > 0, sj
    _run(d, args + ["-bo", "b.bam", "-j", "b.j"], {})
    assert open(os.path.join(d, "a.j")).read() == common.golden_junctions(run["base"]) == open(os.path.join(d, "b.j")).read()
    assert open(os.path.join(d, "a.bam"), "rb").read() == open(os.path.join(d, "b.bam"), "rb").read()
    assert common.stats_block(r.stdout) == common.golden_stats(run["base"])


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_dart_cli_device_sj_folds_the_tables_of_two_roots(pipeline, workdir):
    """DART_SAME_DEVICE_TIMES=2 opens device 0 twice (two roots, 2 x 2 contexts): clones are merged into their roots, the second root's entries are
    downloaded and counted again in the first -- the junction file is that of a run without the switch"""
    c, d = cli_inputs.make(workdir)
    flags = ["-f", "q1.fq", "q1.fq", "q1.fq", "-f2", "q2.fq", "q2.fq", "q2.fq", "-mis", "5"]      # three libraries: several batches per library
    env = dict(PIPELINES[pipeline], DART_BATCH="3000", DART_SAME_DEVICE_TIMES="2", DART_INFLIGHT="2")
    r, sj = _run(d, ["-i", c["prefix"]] + flags + ["-o", "sj2d.sam", "-j", "sj2d.j", "-t", "4"], dict(env, DART_DEVICE_SJ="1"))
    assert "table=device" in sj and _tuples(sj) > 0, sj
    r2, sj2 = _run(d, ["-i", c["prefix"]] + flags + ["-o", "sj2h.sam", "-j", "sj2h.j", "-t", "4"], env)
    assert "table=host" in sj2 and _tuples(sj2) == _tuples(sj), (sj, sj2)
    assert open(os.path.join(d, "sj2d.j")).read() == open(os.path.join(d, "sj2h.j")).read() != ""
    assert open(os.path.join(d, "sj2d.sam")).read() == open(os.path.join(d, "sj2h.sam")).read()
    assert common.stats_block(r.stdout) == common.stats_block(r2.stdout)
