"""GPU suite: `dart -bo` with DART_DEVICE_BAM=1 DART_BGZF_DYNAMIC=1 -- the device's BGZF blocks coded with dynamic Huffman codes per strip (DG_BAM_DYNAMIC) --
decoded by tests/bam_decode.py against the reference's golden SAM; the file is smaller than the fixed mode's, the DART_TIMING line names the mode, and the
variable alone changes nothing."""
import os, subprocess
import pytest
import common, bam_decode
import bam_device_inputs as bdi
from dart_amd import synth

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
SWITCHES = ("DART_DEVICE_BAM", "DART_DEVICE_FASTQ", "DART_DEVICE_SAM", "DART_DEVICE_SJ", "DART_BGZF_DYNAMIC")


def _run(d, args, extra):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000", **extra)      # 4000 reads per batch: several batches
    for k in SWITCHES:
        if k not in extra:
            env.pop(k, None)
    r = subprocess.run([DART] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, r.stderr[-600:]
    timing = [l for l in r.stderr.decode("latin1").splitlines() if l.startswith("[dart timing]")]
    assert timing, r.stderr[-600:]
    return r, timing[-1]


def test_dart_cli_dynamic_bgzf_decodes_to_golden_sam_and_is_smaller(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("se100", workdir)
    d = os.path.join(workdir, "dynbam_se100"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    run = c["runs"][0]
    args = ["-i", c["prefix"], "-f", "1.fq", "-t", "4"] + run["flags"]
    golden = common.golden_sam(run["base"])
    want = bdi.golden_as_bam_stores_it(golden)
    want_hdr = "".join(l + "\n" for l in golden.splitlines() if l.startswith("@"))
    read = lambda f: open(os.path.join(d, f), "rb").read()
    # the host writer, with and without the variable: the same bytes
    r_host, timing = _run(d, args + ["-j", "host.j", "-bo", "host.bam"], {})
    assert "bam=host" in timing and "bam=device" not in timing, timing
    r, timing = _run(d, args + ["-j", "alone.j", "-bo", "alone.bam"], {"DART_BGZF_DYNAMIC": "1"})
    assert "bam=host" in timing and "bam=device" not in timing, timing
    assert read("alone.bam") == read("host.bam")
    # the device's blocks, fixed and dynamic
    r, timing = _run(d, args + ["-j", "fixed.j", "-bo", "fixed.bam"], {"DART_DEVICE_BAM": "1"})
    assert "bam=device" in timing and "bam=device+dyn" not in timing, timing
    r_dyn, timing = _run(d, args + ["-j", "dyn.j", "-bo", "dyn.bam"], {"DART_DEVICE_BAM": "1", "DART_BGZF_DYNAMIC": "1"})
    assert "bam=device+dyn" in timing and "bam=host" not in timing, timing
    hdr, refs, lines, bins = bam_decode.decode(read("dyn.bam"))
    assert hdr == want_hdr and lines == want
    assert common.stats_block(r_dyn.stdout) == common.stats_block(r_host.stdout) == common.golden_stats(run["base"])
    assert read("dyn.j") == read("host.j") == common.golden_junctions(run["base"]).encode()
    print("se100: host writer %d bytes, device fixed %d, device dynamic %d" % (len(read("host.bam")), len(read("fixed.bam")), len(read("dyn.bam"))))
    assert len(read("dyn.bam")) < len(read("fixed.bam"))
