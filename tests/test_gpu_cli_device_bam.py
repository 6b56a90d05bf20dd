"""GPU suite: `dart -bo` with DART_DEVICE_BAM=1 -- the BAM records and their BGZF blocks made on the device (dg_batch_format_bam) in the parallel pipeline --
decoded by tests/bam_decode.py against the reference's golden SAM, with the golden statistics and junctions; the DART_TIMING line must name the BAM path
that ran.  Without the switch `-bo` is what it was: the host writer, the same bytes on every run."""
import os, subprocess
import pytest
import common, bam_decode
import bam_device_inputs as bdi
from dart_amd import synth

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")


def _run(d, args, extra):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000", **extra)      # 4000 reads per batch: every case runs several batches
    for k in ("DART_DEVICE_BAM", "DART_DEVICE_FASTQ", "DART_DEVICE_SAM"):
        if k not in extra:
            env.pop(k, None)
    r = subprocess.run([DART] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, r.stderr[-600:]
    timing = [l for l in r.stderr.decode("latin1").splitlines() if l.startswith("[dart timing]")]
    assert timing, r.stderr[-600:]
    return r, timing[-1]


def _lines(path):
    hdr, refs, lines, bins = bam_decode.decode(open(path, "rb").read())
    return hdr, lines


@pytest.mark.parametrize("name", ["pe101_spliced", "se100"])
def test_dart_cli_device_bam_decodes_to_golden_sam(name, workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case(name, workdir)
    d = os.path.join(workdir, "devbam_" + name); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    files = ["-f", "1.fq"]
    if c["spec"]["paired"]:
        synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2); files += ["-f2", "2.fq"]
    run = c["runs"][0]
    args = ["-i", c["prefix"]] + files + ["-j", "o.j", "-t", "4"] + run["flags"]
    golden = common.golden_sam(run["base"])
    want = bdi.golden_as_bam_stores_it(golden)
    want_hdr = "".join(l + "\n" for l in golden.splitlines() if l.startswith("@"))
    # the switch: the device's records and blocks
    r, timing = _run(d, args + ["-bo", "dev.bam"], {"DART_DEVICE_BAM": "1"})
    assert "bam=device" in timing and "bam=host" not in timing, timing
    hdr, lines = _lines(os.path.join(d, "dev.bam"))
    assert hdr == want_hdr and lines == want
    assert open(os.path.join(d, "o.j")).read() == common.golden_junctions(run["base"])
    assert common.stats_block(r.stdout) == common.golden_stats(run["base"]), r.stdout[-600:]
    # both device switches: the resident form, no gather -- the same content
    r, timing = _run(d, args + ["-bo", "both.bam"], {"DART_DEVICE_BAM": "1", "DART_DEVICE_FASTQ": "1"})
    assert "bam=device" in timing and "assemble=device" in timing, timing
    assert _lines(os.path.join(d, "both.bam")) == (hdr, lines)
    assert common.stats_block(r.stdout) == common.golden_stats(run["base"])
    # without the switch: the host writer, and the same bytes every time
    r, timing = _run(d, args + ["-bo", "h1.bam"], {})
    assert "bam=host" in timing and "bam=device" not in timing, timing
    _run(d, args + ["-bo", "h2.bam"], {})
    h1 = open(os.path.join(d, "h1.bam"), "rb").read()
    assert h1 == open(os.path.join(d, "h2.bam"), "rb").read()
    assert _lines(os.path.join(d, "h1.bam")) == (hdr, lines)
