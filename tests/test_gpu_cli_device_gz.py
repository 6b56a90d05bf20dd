"""GPU suite: `dart` with DART_DEVICE_GZ=1 beside DART_DEVICE_FASTQ=1 and a device formatter -- BGZF-compressed read files go to the GPU as they lie on the
disk (dg_batch_upload_fastq_bgzf, tails chained from batch to batch) -- against the run of the same files without the switch: the same bytes (SAM), the same
records (BAM, decoded by tests/bam_decode.py), junctions and statistics.  The DART_TIMING line must say gz=device, so a silent fall-back cannot pass; and three
inputs that are not for this path -- a plain single-member gzip, a BGZF file with an over-long line, a BGZF file with a flipped CRC -- must fall back silently
to the same bytes."""
import gzip, os, subprocess
import pytest
import common, bam_decode, cli_inputs
import gz_device_inputs as gz

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
SAM = {"DART_DEVICE_FASTQ": "1", "DART_DEVICE_SAM": "1"}
BAM = {"DART_DEVICE_FASTQ": "1", "DART_DEVICE_BAM": "1"}
SWITCHES = ("DART_DEVICE_BAM", "DART_DEVICE_FASTQ", "DART_DEVICE_SAM", "DART_DEVICE_GZ", "DART_BGZF_DYNAMIC")


def _run(d, args, extra):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000", **extra)      # 4000 reads per batch: 3001 pairs run as two batches, with tails between them
    for k in SWITCHES:
        if k not in extra:
            env.pop(k, None)
    r = subprocess.run([DART] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    timing = [l for l in r.stderr.decode("latin1").splitlines() if l.startswith("[dart timing]")]
    return r, (timing[-1] if timing else "")


@pytest.fixture(scope="module")
def files(workdir):
    import __graft_entry__ as ge
    ge.build()
    c, d0 = cli_inputs.make(workdir)
    d = os.path.join(workdir, "cli_devgz"); os.makedirs(d, exist_ok=True)
    q1, q2 = open(os.path.join(d0, "q1.fq"), "rb").read(), open(os.path.join(d0, "q2.fq"), "rb").read()
    w = lambda name, data: open(os.path.join(d, name), "wb").write(data)
    w("b1.fq.gz", gz.bgzf(q1, eof=True)); w("b2.fq.gz", gz.bgzf(q2, block=50000, eof=True))      # (blocks of different sizes: the mates' record boundaries are skewed)
    w("p1.fq.gz", gzip.compress(q1)); w("p2.fq.gz", gzip.compress(q2))
    # record 2900 of file 1 gets a header line of 1100 bytes: the reference's gz reader cuts it into two lines
    lines = q1.split(b"\n")
    lines[11600] = lines[11600] + b" " + b"x" * 1100
    w("long1.fq.gz", gz.bgzf(b"\n".join(lines), eof=True))
    b1 = bytearray(gz.bgzf(q1, eof=True))
    first = int.from_bytes(b1[16:18], "little") + 1
    b1[first - 8] ^= 0x40                                                                            # the first block's CRC32
    w("crc1.fq.gz", bytes(b1))
    return c, d


def _same_outputs(d, a, b, bam):
    if bam:
        assert bam_decode.decode(open(os.path.join(d, a + ".bam"), "rb").read()) == bam_decode.decode(open(os.path.join(d, b + ".bam"), "rb").read())
    else:
        x, y = open(os.path.join(d, a + ".sam"), "rb").read(), open(os.path.join(d, b + ".sam"), "rb").read()
        assert x == y, common.first_diff(x.decode("latin1"), y.decode("latin1"))
        assert len(x) > 100000
    assert open(os.path.join(d, a + ".j")).read() == open(os.path.join(d, b + ".j")).read()


@pytest.mark.parametrize("out", ["sam", "bam"])
def test_dart_cli_device_gz_gives_the_bytes_of_the_host_inflate(out, files):
    c, d = files
    bam = out == "bam"
    sw = BAM if bam else SAM
    o = lambda tag: (["-bo", tag + ".bam"] if bam else ["-o", tag + ".sam"]) + ["-j", tag + ".j"]
    for tag, flags in (("pair", ["-f", "b1.fq.gz", "-f2", "b2.fq.gz", "-mis", "5", "-all_sj"]), ("single", ["-f", "b2.fq.gz", "-mis", "3"])):
        args = ["-i", c["prefix"]] + flags + ["-t", "4"]
        r0, t0 = _run(d, args + o(tag + "_host_" + out), sw)
        r1, t1 = _run(d, args + o(tag + "_dev_" + out), dict(sw, DART_DEVICE_GZ="1"))
        assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-400:], r1.stderr[-400:])
        assert "gz=device" in t1 and "assemble=device" in t1 and "format=device" in t1, t1
        assert "gz=device" not in t0, t0
        _same_outputs(d, tag + "_host_" + out, tag + "_dev_" + out, bam)
        assert common.stats_block(r0.stdout) == common.stats_block(r1.stdout)


def test_dart_cli_device_gz_needs_the_other_device_stages(files):
    c, d = files
    args = ["-i", c["prefix"], "-f", "b1.fq.gz", "-f2", "b2.fq.gz", "-mis", "5", "-t", "4"]
    r0, t0 = _run(d, args + ["-o", "alone_host.sam", "-j", "alone_host.j"], {"DART_DEVICE_FASTQ": "1"})
    for tag, sw in (("alone_gz", {"DART_DEVICE_GZ": "1"}), ("alone_fq", {"DART_DEVICE_GZ": "1", "DART_DEVICE_FASTQ": "1"}), ("alone_sam", {"DART_DEVICE_GZ": "1", "DART_DEVICE_SAM": "1"})):
        r1, t1 = _run(d, args + ["-o", tag + ".sam", "-j", tag + ".j"], sw)
        assert r1.returncode == 0 and "gz=device" not in t1, t1
        _same_outputs(d, "alone_host", tag, False)


@pytest.mark.parametrize("which", ["plain_gzip", "over_long_line", "flipped_crc"])
def test_dart_cli_device_gz_falls_back_silently(which, files):
    c, d = files
    f1 = {"plain_gzip": "p1.fq.gz", "over_long_line": "long1.fq.gz", "flipped_crc": "crc1.fq.gz"}[which]
    f2 = "p2.fq.gz" if which == "plain_gzip" else "b2.fq.gz"
    args = ["-i", c["prefix"], "-f", f1, "-f2", f2, "-mis", "5", "-t", "4"]
    r0, t0 = _run(d, args + ["-o", which + "_host.sam", "-j", which + "_host.j"], SAM)
    r1, t1 = _run(d, args + ["-o", which + "_dev.sam", "-j", which + "_dev.j"], dict(SAM, DART_DEVICE_GZ="1"))
    assert "gz=device" not in t1, t1
    assert r0.returncode == r1.returncode and common.stats_block(r0.stdout) == common.stats_block(r1.stdout)
    x, y = open(os.path.join(d, which + "_host.sam"), "rb").read(), open(os.path.join(d, which + "_dev.sam"), "rb").read()
    assert x == y, common.first_diff(x.decode("latin1"), y.decode("latin1"))
    if which == "plain_gzip":
        assert r1.returncode == 0 and len(x) > 100000
