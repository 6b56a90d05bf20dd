"""GPU suite: `dart -bo` with DART_DEVICE_BAM=1 DART_SORT_BAM=1 DART_RNA_METRICS=<annotation.gtf> -- the sorted file's RNA-seq metrics are built on the device and
written beside it as <out>.rna_metrics.txt -- against the sequential twin of tests/rnametrics_inputs.py computed from the BAM file and the annotation alone; what
the switch needs, what it says when that is missing, that no other output changes with it, and what a failure leaves."""
import os, subprocess
import numpy as np
import pytest
import common
import bamidx_inputs as bii
import rnametrics_inputs as rmi
from rnametrics_inputs import SN
from dart_amd import synth, host

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
SWITCHES = ("DART_DEVICE_BAM", "DART_DEVICE_FASTQ", "DART_DEVICE_SAM", "DART_SORT_BAM", "DART_BAM_INDEX", "DART_BGZF_DYNAMIC", "DART_SORT_PIECE_MB", "DART_GPUS", "DART_COVERAGE",
            "DART_COVERAGE_EXCLUDE", "DART_COVERAGE_MIN_MAPQ", "DART_MARK_DUPLICATES", "DART_PILEUP", "DART_PILEUP_MIN_ALT", "DART_PILEUP_EXCLUDE", "DART_PILEUP_MIN_MAPQ", "DART_QC",
            "DART_QC_EXCLUDE", "DART_QC_MIN_MAPQ", "DART_BAM_TAGS", "DART_GENE_COUNTS", "DART_RNA_METRICS", "DART_RNA_EXCLUDE", "DART_RNA_MIN_MAPQ", "DART_RNA_MIN_COV")
INDEXED = {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_BAM_INDEX": "1", "DART_QC": "1", "DART_COVERAGE": "1"}


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


def _twin_of_file(bam, annot, exclude=rmi.DEFAULT_EXCLUDE, min_mapq=0, min_cov=rmi.DEFAULT_MIN_COV):
    """the twin's words and text over the file's own records"""
    _, _, raw, n_chr = bii.split_file(bam)
    words = rmi.twin(raw, n_chr, annot, exclude, min_mapq, min_cov)
    return words, rmi.text_of(words)


def test_dart_cli_writes_the_rna_metrics_of_the_sorted_file(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("pe101_spliced", workdir)
    d = os.path.join(workdir, "rna_cli"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1); synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2)
    args = ["-i", c["prefix"], "-f", "1.fq", "-f2", "2.fq", "-t", "4", "-mis", "5"]
    annot = rmi.case_annotation(c, rmi.CASE_SEEDS["pe101_spliced"])
    rmi.write_gtf(os.path.join(d, "a.gtf"), annot, host.Index(c["prefix"]).names)
    # the sorted, indexed file with its QC tables and track, without the switch: no metrics; with it the same bytes in every other output
    others = ("", ".bai", ".qc.txt", ".bedgraph")
    _, timing = _run(d, args + ["-bo", "plain.bam", "-j", "plain.j"], INDEXED)
    assert not os.path.exists(os.path.join(d, "plain.bam.rna_metrics.txt")) and not any(" rna metrics:" in l for l in timing)
    _, timing = _run(d, args + ["-bo", "one.bam", "-j", "one.j"], dict(INDEXED, DART_RNA_METRICS="a.gtf", DART_RNA_MIN_COV=str(rmi.CASE_MIN_COV)))
    for ext in others:
        assert _read(d, "one.bam" + ext) == _read(d, "plain.bam" + ext), ext
    assert _read(d, "one.j") == _read(d, "plain.j")
    bam = _read(d, "one.bam")
    words, text = _twin_of_file(bam, annot, min_cov=rmi.CASE_MIN_COV)         # exclude 0x904 and min_mapq 0 are the defaults
    v = rmi.views(words)
    assert _read(d, "one.bam.rna_metrics.txt") == text and v["BA"].all() and v["ST"].all() and v["SN"][SN["contributing_transcripts"]] >= 20 and v["SN"][SN["counted"]] > 2000
    note = [l for l in timing if l.startswith("[dart timing] rna metrics:")]
    assert len(note) == 1 and ("%d words, %d bytes" % (len(words), len(text))) in note[0], timing
    # the default min_cov, the filter's two variables, beside the duplicate marking and the tagging: the metrics are those of the marked, tagged file
    m1 = np.concatenate([c["m1"], c["m1"][:300]]); m2 = np.concatenate([c["m2"], c["m2"][:300]])
    synth.write_fastq(os.path.join(d, "d1.fq"), m1, 1); synth.write_fastq(os.path.join(d, "d2.fq"), m2, 2)
    dargs = ["-i", c["prefix"], "-f", "d1.fq", "-f2", "d2.fq", "-j", "o.j", "-t", "4", "-mis", "5"]
    _run(d, dargs + ["-bo", "two.bam"], {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_MARK_DUPLICATES": "1", "DART_BAM_TAGS": "all", "DART_RNA_METRICS": os.path.join(d, "a.gtf"),
                                         "DART_RNA_EXCLUDE": "0x704", "DART_RNA_MIN_MAPQ": "2"})
    two = _read(d, "two.bam")
    words2, text2 = _twin_of_file(two, annot, 0x704, 2)
    assert _read(d, "two.bam.rna_metrics.txt") == text2
    assert 300 <= int(_twin_of_file(two, annot, 0x304, 2)[0][rmi.OFF["SN"] + SN["counted"]]) - int(words2[rmi.OFF["SN"] + SN["counted"]])      # the marks are seen
    # a failure behind the close leaves the BAM and its index complete, and no metrics: the text's path is taken by a directory (one that is not empty: the
    # run's first act on a stale text is to remove it)
    os.makedirs(os.path.join(d, "bad.bam.rna_metrics.txt", "x"))
    r = _spawn(d, args + ["-bo", "bad.bam", "-j", "bad.j"], dict(INDEXED, DART_RNA_METRICS="a.gtf"))
    assert r.returncode == 1 and "Error while writing bad.bam.rna_metrics.txt" in r.stderr.decode("latin1")
    assert _read(d, "bad.bam") == bam and _read(d, "bad.bam.bai") == _read(d, "plain.bam.bai") and not os.path.isfile(os.path.join(d, "bad.bam.rna_metrics.txt"))


def test_dart_cli_rna_metrics_switch_says_what_is_missing(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("se100", workdir)
    d = os.path.join(workdir, "rna_missing"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    names = host.Index(c["prefix"]).names
    rmi.write_gtf(os.path.join(d, "a.gtf"), [rmi.tx(0, 0, [(100, 300)], cds=(150, 250))], names)
    args = ["-i", c["prefix"], "-f", "1.fq", "-j", "o.j", "-t", "4"] + c["runs"][0]["flags"]
    gone = lambda out: not os.path.exists(os.path.join(d, out)) and not os.path.exists(os.path.join(d, out + ".rna_metrics.txt")) and not os.path.exists(os.path.join(d, out + ".bai"))
    for out, extra in ((["-bo", "a.bam"], {"DART_RNA_METRICS": "a.gtf", "DART_DEVICE_BAM": "1"}), (["-bo", "b.bam"], {"DART_RNA_METRICS": "a.gtf"}), (["-o", "c.sam"], {"DART_RNA_METRICS": "a.gtf"})):
        r = _spawn(d, args + out, extra)
        err = r.stderr.decode("latin1").splitlines()
        assert r.returncode == 1 and len(err) == 1 and err[0].startswith("Error! DART_RNA_METRICS=a.gtf needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): "), (r.returncode, err)
        assert gone(out[1])
    # with the sort asked for but not possible, the sort's own message comes first
    r = _spawn(d, args + ["-bo", "e.bam"], {"DART_RNA_METRICS": "a.gtf", "DART_SORT_BAM": "1"})
    assert r.returncode == 1 and "DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1" in r.stderr.decode("latin1") and gone("e.bam")
    # a GTF that cannot be used ends the run before any output exists: a missing file, a fatal line, no transcript on the index's sequences; a stale text goes too
    sorted_env = {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_BAM_INDEX": "1"}
    name0 = names[0].decode() if isinstance(names[0], bytes) else names[0]
    open(os.path.join(d, "fatal.gtf"), "w").write("%s\tt\texon\t100\t200\t.\t+\t.\ttranscript_id \"t\";\n%s\tt\texon\t300\t200\t.\t+\t.\ttranscript_id \"t\";\n" % (name0, name0))
    open(os.path.join(d, "foreign.gtf"), "w").write("elsewhere\tt\texon\t100\t200\t.\t+\t.\ttranscript_id \"t\";\n")
    for gtf, word in (("none.gtf", "cannot read"), ("fatal.gtf", "line 2: "), ("foreign.gtf", "no transcript")):
        open(os.path.join(d, "f.bam.rna_metrics.txt"), "w").write("stale\n")
        r = _spawn(d, args + ["-bo", "f.bam"], dict(sorted_env, DART_RNA_METRICS=gtf))
        assert r.returncode == 1 and ("Error! DART_RNA_METRICS=%s: " % gtf) in r.stderr.decode("latin1") and word in r.stderr.decode("latin1") and gone("f.bam"), r.stderr[-400:]
    # and a usable one on single-end reads
    _run(d, args + ["-bo", "g.bam"], dict(sorted_env, DART_RNA_METRICS="a.gtf", DART_RNA_MIN_COV="1"))
    words, text = _twin_of_file(_read(d, "g.bam"), [rmi.tx(0, 0, [(100, 300)], cds=(150, 250))], min_cov=1)
    assert _read(d, "g.bam.rna_metrics.txt") == text
