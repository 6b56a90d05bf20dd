"""GPU suite: `dart` with DART_DEVICE_FASTQ=1 -- the parallel pipeline hands every batch to the GPU as FASTQ text (dg_batch_upload_fastq), alone and together
with DART_DEVICE_SAM=1 (dg_batch_format_sam_resident: nothing is gathered on the host) -- against the reference's golden SAM, junctions and statistics and
against the oracle's command line; the DART_TIMING line must say who assembled the batches, so a silent fall-back to the host cannot pass."""
import os, subprocess
import pytest
import common, oracle_py, cli_inputs
import fastq_device_inputs as fdi
from dart_amd import synth

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
SWITCHES = {"fastq": {"DART_DEVICE_FASTQ": "1"}, "fastq+sam": {"DART_DEVICE_FASTQ": "1", "DART_DEVICE_SAM": "1"}}


def _run(d, args, extra):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000", **extra)      # 4000 reads per batch: every case runs several batches
    r = subprocess.run([DART] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, r.stderr[-600:]
    timing = [l for l in r.stderr.decode("latin1").splitlines() if l.startswith("[dart timing]")]
    assert timing, r.stderr[-600:]
    return r, timing[-1]


def _says_device(timing, switches):
    assert "assemble=device" in timing and "assemble=host" not in timing, timing
    assert ("format=device" in timing) == ("DART_DEVICE_SAM" in switches), timing
    if "DART_DEVICE_SAM" in switches:
        assert "gather" not in timing, timing


@pytest.mark.parametrize("switches", sorted(SWITCHES))
def test_dart_cli_device_fastq_reproduces_golden_sam(switches, workdir):
    import __graft_entry__ as ge
    ge.build()
    for name in sorted(common.MANIFEST["cases"]):
        c = common.build_case(name, workdir)
        d = os.path.join(workdir, "devfq_%s_%s" % (switches, name)); os.makedirs(d, exist_ok=True)
        synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
        files = ["-f", "1.fq"]
        if c["spec"]["paired"]:
            synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2); files += ["-f2", "2.fq"]
        for run in c["runs"]:
            r, timing = _run(d, ["-i", c["prefix"]] + files + ["-o", "o.sam", "-j", "o.j", "-t", "4"] + run["flags"], SWITCHES[switches])
            _says_device(timing, SWITCHES[switches])
            got, want = open(os.path.join(d, "o.sam")).read(), common.golden_sam(run["base"])
            assert got == want, common.first_diff(got, want)
            assert open(os.path.join(d, "o.j")).read() == common.golden_junctions(run["base"])
            assert common.stats_block(r.stdout) == common.golden_stats(run["base"]), (run["base"], r.stdout[-600:])
    # without the switch the assemble field is the one it always was
    r, timing = _run(d, ["-i", c["prefix"]] + files + ["-o", "h.sam", "-j", "h.j", "-t", "4"] + c["runs"][0]["flags"], {})
    assert ", assemble " in timing and "assemble=" not in timing, timing


def _awkward_files(workdir):
    c, d0 = cli_inputs.make(workdir)
    d = os.path.join(workdir, "awkward_devfq")
    if not os.path.exists(os.path.join(d, "stop.fq")):
        os.makedirs(d, exist_ok=True)
        m1, m2 = synth.make_reads(c["genome"], 4603, rlen=101, seed=78, spliced_frac=0.2)
        rec = fdi.rec
        with open(os.path.join(d, "a1.fq"), "w") as f:
            f.write("".join(rec(i, m1[i], "1") for i in range(4603))[:-1])            # no newline at the end
        with open(os.path.join(d, "a2.fq"), "w") as f:
            f.write("".join(rec(i, m2[i], "2") for i in range(4603)))
        with open(os.path.join(d, "inter_odd.fq"), "w") as f:
            f.write("".join(rec(i, m1[i], "1") + (rec(i, m2[i], "2") if i < 4302 else "") for i in range(4303)))
        with open(os.path.join(d, "stop.fq"), "w") as f:
            f.write("".join(rec(i, m1[i], "1") for i in range(700)) + "@empty\n\n+\n\n" + "".join(rec(i, m1[i], "1") for i in range(700, 900)))
    return c, d


def _against_oracle(c, d, flags, switches, tag):
    r, timing = _run(d, ["-i", c["prefix"]] + flags + ["-o", tag + ".sam", "-j", tag + ".j", "-t", "5"], switches)
    orc = "orc_" + "_".join(x.replace(".", "_") for x in flags if not x.startswith("-"))
    if not os.path.exists(os.path.join(d, orc + ".sam")):
        subprocess.run([oracle_py.ORACLE_CLI, "-i", c["prefix"]] + flags + ["-o", orc + ".sam", "-j", orc + ".j"], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
    a, b = open(os.path.join(d, orc + ".sam"), "rb").read(), open(os.path.join(d, tag + ".sam"), "rb").read()
    assert a == b, (flags, common.first_diff(b.decode("latin1"), a.decode("latin1")))
    assert open(os.path.join(d, orc + ".j")).read() == open(os.path.join(d, tag + ".j")).read()
    return timing


@pytest.mark.parametrize("switches", sorted(SWITCHES))
def test_dart_cli_device_fastq_on_awkward_files(switches, workdir):
    """the files of tests/test_gpu_cli.py::test_dart_cli_awkward_fastq: two files, an odd interlaced -p file whose tail is mapped unpaired, and a file with a
    record without bases, which the host assembles (and says so)"""
    oracle_py.build()
    c, d = _awkward_files(workdir)
    for flags in (["-f", "a1.fq", "-f2", "a2.fq", "-mis", "5"], ["-f", "inter_odd.fq", "-p", "-mis", "5"]):
        _says_device(_against_oracle(c, d, flags, SWITCHES[switches], "gpu"), SWITCHES[switches])
    timing = _against_oracle(c, d, ["-f", "stop.fq", "-mis", "3"], SWITCHES[switches], "gpu")
    assert "assemble=host" in timing and "assemble=device" not in timing, timing


@pytest.mark.parametrize("switches", sorted(SWITCHES))
def test_dart_cli_device_fastq_on_gz_files_inflated_whole(switches, workdir):
    oracle_py.build()
    c, d = cli_inputs.make(workdir)
    flags = [v[0] for v in cli_inputs.VARIANTS if v[1] == "paired fastq.gz"][0]
    _says_device(_against_oracle(c, d, flags, SWITCHES[switches], "devfq_gz"), SWITCHES[switches])


def test_dart_cli_streaming_pipeline_ignores_the_switch(workdir):
    oracle_py.build()
    c, d = cli_inputs.make(workdir)
    flags = [v[0] for v in cli_inputs.VARIANTS if v[1] == "paired fastq"][0]
    timing = _against_oracle(c, d, flags, {"DART_DEVICE_FASTQ": "1", "DART_STREAMING": "1"}, "devfq_stream")
    assert "assemble=device" not in timing and "read+parse" in timing, timing
