"""GPU suite: `dart -bo` with DART_DEVICE_BAM=1 DART_SORT_BAM=1 DART_BAM_INDEX=1 -- the sorted file's .bai is built on the device and written beside it --
against the sequential twin of tests/bamidx_inputs.py computed from the BAM file alone (block sizes from the BGZF headers, records from the inflated
blocks); region queries through the files against the decoded lines filtered by hand; what the switch needs, and what it says when that is missing."""
import os, random, subprocess
import pytest
import common, bam_decode
import bamidx_inputs as bii
from dart_amd import synth

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
SWITCHES = ("DART_DEVICE_BAM", "DART_DEVICE_FASTQ", "DART_DEVICE_SAM", "DART_SORT_BAM", "DART_BAM_INDEX", "DART_BGZF_DYNAMIC", "DART_SORT_PIECE_MB", "DART_GPUS")
SORTED = {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1"}
INDEXED = dict(SORTED, DART_BAM_INDEX="1")


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


def _read(d, name):
    return open(os.path.join(d, name), "rb").read()


def _rlen(cigar):
    n, out = "", 0
    for ch in cigar:
        if ch.isdigit():
            n += ch
        else:
            out += int(n) if ch in "MDN=X" else 0
            n = ""
    return out


@pytest.mark.parametrize("name", ["pe101_spliced", "se100"])
def test_dart_cli_writes_the_index_of_the_sorted_file(name, workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case(name, workdir)
    d = os.path.join(workdir, "bamidx_" + name); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    files = ["-f", "1.fq"]
    if c["spec"]["paired"]:
        synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2); files += ["-f2", "2.fq"]
    run = c["runs"][0]
    args = ["-i", c["prefix"]] + files + ["-j", "o.j", "-t", "4"] + run["flags"]
    # the sorted file without the switch: no index, and the same BAM bytes with it
    _run(d, args + ["-bo", "plain.bam"], SORTED)
    assert not os.path.exists(os.path.join(d, "plain.bam.bai"))
    r, timing = _run(d, args + ["-bo", "sorted.bam"], INDEXED)
    assert "; index " in timing[-1] and "bytes)" in timing[-1] and "compress + download + write" in timing[-1], timing[-1]
    bam, bai = _read(d, "sorted.bam"), _read(d, "sorted.bam.bai")
    assert bam == _read(d, "plain.bam")
    assert bai == bii.build_bai_of_file(bam)
    assert ("%d bytes)" % len(bai)) in timing[-1]
    assert open(os.path.join(d, "o.j")).read() == common.golden_junctions(run["base"])
    assert common.stats_block(r.stdout) == common.golden_stats(run["base"]), r.stdout[-600:]
    # region queries through the two files against the decoded lines filtered by hand
    hdr, refs, lines, _ = bam_decode.decode(bam)
    ix = bii.parse_bai(bai)
    assert len(ix["refs"]) == len(refs) and sum(len(r["bins"]) for r in ix["refs"]) > len(refs)
    rows = []
    tid = {n: i for i, (n, _) in enumerate(refs)}
    for l in lines:
        f = l.split("\t")
        if f[2] != "*" and not int(f[1]) & 4:
            beg = max(int(f[3]) - 1, 0)
            rows.append((tid[f[2]], beg, max(int(f[3]) - 1 + (_rlen(f[5]) or 1), beg + 1), f[0], int(f[1])))
    rng = random.Random(5)
    hits = 0
    for t, (_, length) in enumerate(refs):
        regions = [(0, 1), (16383, 16385), (length - 1, length)] + [(b, b + rng.choice([1, 100, 5000])) for b in (rng.randrange(0, length) for _ in range(40))]
        for b, e in regions:
            want = [(nm, fl) for rt, rb, re_, nm, fl in rows if rt == t and rb < e and re_ > b]
            got = [(rec[36:36 + rec[12] - 1].decode(), int.from_bytes(rec[18:20], "little")) for rec in bii.query(bai, bam, t, b, e)]
            assert got == want, (t, b, e)
            hits += len(want)
    assert hits > 100
    # one block per piece, and dynamic codes: each file's index is the twin of its own file
    _run(d, args + ["-bo", "piece.bam"], dict(INDEXED, DART_SORT_PIECE_MB="0"))
    assert _read(d, "piece.bam") == bam and _read(d, "piece.bam.bai") == bai
    _run(d, args + ["-bo", "dyn.bam"], dict(INDEXED, DART_BGZF_DYNAMIC="1"))
    dyn, dyn_bai = _read(d, "dyn.bam"), _read(d, "dyn.bam.bai")
    assert len(dyn) < len(bam) and dyn_bai == bii.build_bai_of_file(dyn) != bai


def test_dart_cli_index_switch_says_what_is_missing(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("se100", workdir)
    d = os.path.join(workdir, "bamidx_missing"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    args = ["-i", c["prefix"], "-f", "1.fq", "-j", "o.j", "-t", "4"] + c["runs"][0]["flags"]
    for out, extra in ((["-bo", "a.bam"], {"DART_BAM_INDEX": "1", "DART_DEVICE_BAM": "1"}), (["-bo", "b.bam"], {"DART_BAM_INDEX": "1"}), (["-o", "c.sam"], {"DART_BAM_INDEX": "1"})):
        r = _spawn(d, args + out, extra)
        err = r.stderr.decode("latin1").splitlines()
        assert r.returncode == 1 and len(err) == 1 and err[0].startswith("Error! DART_BAM_INDEX=1 needs DART_SORT_BAM=1") and "-bo and DART_DEVICE_BAM=1" in err[0], (r.returncode, err)
        assert not os.path.exists(os.path.join(d, out[1])) and not os.path.exists(os.path.join(d, out[1] + ".bai"))
    # with the sort asked for but not possible, the sort's own message comes first
    r = _spawn(d, args + ["-bo", "e.bam"], {"DART_BAM_INDEX": "1", "DART_SORT_BAM": "1"})
    assert r.returncode == 1 and "DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1" in r.stderr.decode("latin1") and not os.path.exists(os.path.join(d, "e.bam"))
