"""GPU suite: `dart -bo` with DART_DEVICE_BAM=1 DART_SORT_BAM=1 DART_QC=1 -- the sorted file's QC tables are built on the device and written beside it as
<out>.qc.txt -- against the sequential twin of tests/qc_inputs.py computed from the BAM file and the index's text alone; what the switch needs, what it says when
that is missing, that nothing changes without it, and that a failure leaves the BAM and its index complete."""
import os, subprocess
import numpy as np
import pytest
import common, bam_decode
import bamidx_inputs as bii
import pileup_inputs as pui
import qc_inputs as qci
from qc_inputs import SN
from dart_amd import synth, host

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
SWITCHES = ("DART_DEVICE_BAM", "DART_DEVICE_FASTQ", "DART_DEVICE_SAM", "DART_SORT_BAM", "DART_BAM_INDEX", "DART_BGZF_DYNAMIC", "DART_SORT_PIECE_MB", "DART_GPUS", "DART_COVERAGE",
            "DART_COVERAGE_EXCLUDE", "DART_COVERAGE_MIN_MAPQ", "DART_MARK_DUPLICATES", "DART_PILEUP", "DART_PILEUP_MIN_ALT", "DART_PILEUP_EXCLUDE", "DART_PILEUP_MIN_MAPQ", "DART_QC",
            "DART_QC_EXCLUDE", "DART_QC_MIN_MAPQ")
INDEXED = {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_BAM_INDEX": "1"}


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


def _twin_of_file(bam, ref, exclude=qci.DEFAULT_EXCLUDE, min_mapq=0):
    """the twin's words and text over the file's own records, names and lengths"""
    _, _, raw, n_chr = bii.split_file(bam)
    refs = bam_decode.decode(bam)[1]
    names = [n.encode() if isinstance(n, str) else n for n, _ in refs]
    words = qci.twin(raw, ref, exclude, min_mapq)
    return words, qci.text_of(words, names, [int(l) for _, l in refs])


def test_dart_cli_writes_the_qc_tables_of_the_sorted_file(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("pe101_spliced", workdir)
    d = os.path.join(workdir, "qc_cli"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1); synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2)
    args = ["-i", c["prefix"], "-f", "1.fq", "-f2", "2.fq", "-j", "o.j", "-t", "4", "-mis", "5"]
    ref = pui.ref_of_index(host.Index(c["prefix"]))
    # the sorted, indexed file without the switch: no tables, and the same BAM and .bai bytes with it
    _, timing = _run(d, args + ["-bo", "plain.bam"], INDEXED)
    assert not os.path.exists(os.path.join(d, "plain.bam.qc.txt")) and not any(" qc:" in l for l in timing)
    _, timing = _run(d, args + ["-bo", "one.bam"], dict(INDEXED, DART_QC="1"))
    bam = _read(d, "one.bam")
    assert bam == _read(d, "plain.bam") and _read(d, "one.bam.bai") == _read(d, "plain.bam.bai")
    words, text = _twin_of_file(bam, ref)                                   # the defaults: exclude 0x904, min_mapq 0
    v = qci.views(words, ref.n_chr)
    assert _read(d, "one.bam.qc.txt") == text and v["SN"][SN["profiled"]] > 1000 and v["FS"][:, 11].sum() > 0 and v["FS"][:, 4].sum() == 0
    note = [l for l in timing if l.startswith("[dart timing] qc:")]
    assert len(note) == 1 and ("%d words, %d bytes" % (len(words), len(text))) in note[0], timing
    # the filter's two variables, beside the duplicate marking: the tables are those of the marked file.  The duplicates rows are non-zero only because the input
    # repeats pairs: the first 300 pairs are written into the FASTQ twice
    m1 = np.concatenate([c["m1"], c["m1"][:300]]); m2 = np.concatenate([c["m2"], c["m2"][:300]])
    synth.write_fastq(os.path.join(d, "d1.fq"), m1, 1); synth.write_fastq(os.path.join(d, "d2.fq"), m2, 2)
    dargs = ["-i", c["prefix"], "-f", "d1.fq", "-f2", "d2.fq", "-j", "o.j", "-t", "4", "-mis", "5"]
    _run(d, dargs + ["-bo", "two.bam"], {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_MARK_DUPLICATES": "1", "DART_QC": "1", "DART_QC_EXCLUDE": "0x704", "DART_QC_MIN_MAPQ": "2"})
    words2, text2 = _twin_of_file(_read(d, "two.bam"), ref, 0x704, 2)
    v2 = qci.views(words2, ref.n_chr)
    assert _read(d, "two.bam.qc.txt") == text2 and v2["FS"][:, 4].sum() >= 300 and v2["FS"][:, 5].sum() >= 300 and not os.path.exists(os.path.join(d, "two.bam.bai"))
    assert v2["SN"][SN["profiled"]] < v2["FS"][:, 7].sum()                   # duplicates and low MAPQ stay out of the profile
    # a failure behind the close leaves the BAM and its index complete, and no tables: the tables' path is taken by a directory
    os.makedirs(os.path.join(d, "bad.bam.qc.txt"))
    r = _spawn(d, args + ["-bo", "bad.bam"], dict(INDEXED, DART_QC="1"))
    assert r.returncode == 1 and "Error while writing bad.bam.qc.txt" in r.stderr.decode("latin1")
    assert _read(d, "bad.bam") == bam and _read(d, "bad.bam.bai") == _read(d, "plain.bam.bai") and not os.path.isfile(os.path.join(d, "bad.bam.qc.txt"))


def test_dart_cli_qc_switch_says_what_is_missing(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("se100", workdir)
    d = os.path.join(workdir, "qc_missing"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    args = ["-i", c["prefix"], "-f", "1.fq", "-j", "o.j", "-t", "4"] + c["runs"][0]["flags"]
    for out, extra in ((["-bo", "a.bam"], {"DART_QC": "1", "DART_DEVICE_BAM": "1"}), (["-bo", "b.bam"], {"DART_QC": "1"}), (["-o", "c.sam"], {"DART_QC": "1"})):
        r = _spawn(d, args + out, extra)
        err = r.stderr.decode("latin1").splitlines()
        assert r.returncode == 1 and len(err) == 1 and err[0].startswith("Error! DART_QC=1 needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): "), (r.returncode, err)
        assert not os.path.exists(os.path.join(d, out[1])) and not os.path.exists(os.path.join(d, out[1] + ".qc.txt"))
    # with the sort asked for but not possible, the sort's own message comes first
    r = _spawn(d, args + ["-bo", "e.bam"], {"DART_QC": "1", "DART_SORT_BAM": "1"})
    assert r.returncode == 1 and "DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1" in r.stderr.decode("latin1") and not os.path.exists(os.path.join(d, "e.bam")) and not os.path.exists(os.path.join(d, "e.bam.qc.txt"))
