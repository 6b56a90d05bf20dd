"""GPU suite: `dart -bo` with DART_DEVICE_BAM=1 DART_SORT_BAM=1 DART_PILEUP=1 -- the sorted file's variant-site table is built on the device and written beside
it -- against the sequential twin of tests/pileup_inputs.py computed from the BAM file and the index's text alone; what the switch needs, what it says when that
is missing, that nothing changes without it, and that a failure leaves the BAM and its index complete."""
import os, subprocess
import pytest
import common, bam_decode
import bamidx_inputs as bii
import pileup_inputs as pui
from dart_amd import synth, host

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
SWITCHES = ("DART_DEVICE_BAM", "DART_DEVICE_FASTQ", "DART_DEVICE_SAM", "DART_SORT_BAM", "DART_BAM_INDEX", "DART_BGZF_DYNAMIC", "DART_SORT_PIECE_MB", "DART_GPUS", "DART_COVERAGE",
            "DART_COVERAGE_EXCLUDE", "DART_COVERAGE_MIN_MAPQ", "DART_MARK_DUPLICATES", "DART_PILEUP", "DART_PILEUP_MIN_ALT", "DART_PILEUP_EXCLUDE", "DART_PILEUP_MIN_MAPQ")
INDEXED = {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_BAM_INDEX": "1"}
HEADER = b"#chr\tpos\tref\tdepth\tdepth_rev\tA\tC\tG\tT\tN\tDEL\tINS\tA_rev\tC_rev\tG_rev\tT_rev\tN_rev\tDEL_rev\tINS_rev\n"


def _spawn(d, args, extra):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000", **extra)      # 4000 reads per batch: the case runs several batches
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


def test_dart_cli_writes_the_site_table_of_the_sorted_file(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("pe101_spliced", workdir)
    d = os.path.join(workdir, "pu_cli"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1); synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2)
    args = ["-i", c["prefix"], "-f", "1.fq", "-f2", "2.fq", "-j", "o.j", "-t", "4", "-mis", "5"]
    ref = pui.ref_of_index(host.Index(c["prefix"]))
    # the sorted, indexed file without the switch: no table, and the same BAM and .bai bytes with it
    _, timing = _run(d, args + ["-bo", "plain.bam"], INDEXED)
    assert not os.path.exists(os.path.join(d, "plain.bam.sites.tsv")) and not any("pileup" in l for l in timing)
    _, timing = _run(d, args + ["-bo", "one.bam"], dict(INDEXED, DART_PILEUP="1"))
    bam = _read(d, "one.bam")
    assert bam == _read(d, "plain.bam") and _read(d, "one.bam.bai") == _read(d, "plain.bam.bai")
    _, _, raw, n_chr = bii.split_file(bam)
    names = [n.encode() if isinstance(n, str) else n for n, _ in bam_decode.decode(bam)[1]]
    ent, st = pui.twin(raw, ref)                                        # the defaults: min_alt 2, exclude 0x704, min_mapq 0
    table = _read(d, "one.bam.sites.tsv")
    assert table == HEADER + pui.text_of(ent, names) and st[6] > 20 and st[7] > 0
    note = [l for l in timing if l.startswith("[dart timing] pileup:")]
    assert len(note) == 1 and ("%d sites, %d kept, %d bytes" % (st[6], st[7], len(table) - len(HEADER))) in note[0], timing
    # the filter's three variables, beside the duplicate marking: the table is that of the marked file
    _run(d, args + ["-bo", "two.bam"], {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_MARK_DUPLICATES": "1", "DART_PILEUP": "1", "DART_PILEUP_MIN_ALT": "1", "DART_PILEUP_EXCLUDE": "0x304",
                                        "DART_PILEUP_MIN_MAPQ": "2"})
    _, _, raw2, _ = bii.split_file(_read(d, "two.bam"))
    ent2, st2 = pui.twin(raw2, ref, exclude=0x304, min_mapq=2, min_alt=1)
    assert _read(d, "two.bam.sites.tsv") == HEADER + pui.text_of(ent2, names) and st2[7] == st2[6] > st[7] and not os.path.exists(os.path.join(d, "two.bam.bai"))
    # a failure behind the close leaves the BAM and its index complete, and no table: the table's path is taken by a directory
    os.makedirs(os.path.join(d, "bad.bam.sites.tsv"))
    r = _spawn(d, args + ["-bo", "bad.bam"], dict(INDEXED, DART_PILEUP="1"))
    assert r.returncode == 1 and "Error while writing bad.bam.sites.tsv" in r.stderr.decode("latin1")
    assert _read(d, "bad.bam") == bam and _read(d, "bad.bam.bai") == _read(d, "plain.bam.bai")


def test_dart_cli_pileup_switch_says_what_is_missing(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("se100", workdir)
    d = os.path.join(workdir, "pu_missing"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    args = ["-i", c["prefix"], "-f", "1.fq", "-j", "o.j", "-t", "4"] + c["runs"][0]["flags"]
    for out, extra in ((["-bo", "a.bam"], {"DART_PILEUP": "1", "DART_DEVICE_BAM": "1"}), (["-bo", "b.bam"], {"DART_PILEUP": "1"}), (["-o", "c.sam"], {"DART_PILEUP": "1"})):
        r = _spawn(d, args + out, extra)
        err = r.stderr.decode("latin1").splitlines()
        assert r.returncode == 1 and len(err) == 1 and err[0].startswith("Error! DART_PILEUP=1 needs DART_SORT_BAM=1") and "-bo and DART_DEVICE_BAM=1" in err[0], (r.returncode, err)
        assert not os.path.exists(os.path.join(d, out[1])) and not os.path.exists(os.path.join(d, out[1] + ".sites.tsv"))
    r = _spawn(d, args + ["-bo", "f.bam"], {"DART_PILEUP": "1", "DART_PILEUP_MIN_ALT": "0", "DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1"})
    assert r.returncode == 1 and "DART_PILEUP_MIN_ALT=0" in r.stderr.decode("latin1") and not os.path.exists(os.path.join(d, "f.bam"))
    # with the sort asked for but not possible, the sort's own message comes first
    r = _spawn(d, args + ["-bo", "e.bam"], {"DART_PILEUP": "1", "DART_SORT_BAM": "1"})
    assert r.returncode == 1 and "DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1" in r.stderr.decode("latin1") and not os.path.exists(os.path.join(d, "e.bam"))
