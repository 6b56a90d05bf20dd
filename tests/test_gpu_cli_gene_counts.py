"""GPU suite: `dart` with DART_GENE_COUNTS=<annotation.gtf> -- reads per gene counted on the device batch by batch (dg_batch_accumulate_genes, dg_gene_merge,
dg_gene_add) in both host pipelines -- against the Python twin (tests/genecount_inputs.py) run over the SAM file the same run wrote: first line per read, units
by name and flag & 1, blocks from the printed CIGAR.  The `[dart genes]` line must name the table that ran."""
import os, re, subprocess
import numpy as np
import pytest
import common, genecount_inputs as gci
from dart_amd import synth, sam

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
PIPELINES = {"parallel": {}, "streaming": {"DART_STREAMING": "1"}}
CASES = ["se100", "pe101_spliced", "pe151_spliced"]


def _run(d, args, extra, want_rc=0):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000")      # 4000 reads per batch, the smallest
    env.update(extra)
    r = subprocess.run([DART] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == want_rc, r.stderr[-800:]
    lines = [l for l in r.stderr.decode("latin1").splitlines() if l.startswith("[dart genes]")]
    return r, lines


def _inputs(c, workdir, tag):
    d = os.path.join(workdir, "genes_%s_%s" % (tag, c["name"])); os.makedirs(d, exist_ok=True)
    files = ["-f", "1.fq"]
    if not os.path.exists(os.path.join(d, "ann.gtf")):
        synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
        if c["spec"]["paired"]:
            synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2)
    if c["spec"]["paired"]:
        files += ["-f2", "2.fq"]
    n_genes, exons = gci.case_annotation(c, gci.CASE_SEEDS[c["name"]])
    order = gci.write_gtf(os.path.join(d, "ann.gtf"), exons, c["genome"].names)
    assert sorted(order) == list(range(n_genes))
    return d, files, n_genes, exons, order


def _expected(c, sam_text, flags, n_genes, exons, order, min_mapq=4):
    _, h = common.parse_flags(flags)
    (rd, rp, cg), npm = gci.sam_records(sam_text, len(c["reads"]), bool(c["spec"]["paired"]), c["genome"].names, h["unique"])
    counts = gci.twin(len(c["genome"].lengths), n_genes, exons, rd, rp, cg, npm, min_mapq)
    names, rows = gci.table_in_file_order(counts, order)
    return sam.gene_table(names, rows), counts


def _line_ok(lines, counts):
    assert len(lines) == 1 and "table=device" in lines[0] and "acc_ms=" in lines[0], lines
    assert int(re.search(r"units=(\d+)", lines[0]).group(1)) == int(counts[:, 0].sum()) and int(re.search(r"counted=(\d+)", lines[0]).group(1)) == int(counts[4:, 0].sum()) > 0, lines


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_dart_cli_gene_table_equals_the_twin_over_its_own_sam(pipeline, name, workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case(name, workdir)
    d, files, n_genes, exons, order = _inputs(c, workdir, pipeline)
    for run in c["runs"]:
        for stale in ("o.sam", "o.sam.genes.tab"):
            if os.path.exists(os.path.join(d, stale)):
                os.remove(os.path.join(d, stale))
        r, lines = _run(d, ["-i", c["prefix"]] + files + ["-o", "o.sam", "-j", "o.j", "-t", "4"] + run["flags"], dict(PIPELINES[pipeline], DART_GENE_COUNTS="ann.gtf"))
        got_sam = open(os.path.join(d, "o.sam")).read()
        want, counts = _expected(c, got_sam, run["flags"], n_genes, exons, order)
        got = open(os.path.join(d, "o.sam.genes.tab"), "rb").read()
        assert got == want, (run["base"], common.first_diff(got.decode(), want.decode()))
        _line_ok(lines, counts)
        want_sam = common.golden_sam(run["base"])
        assert got_sam == want_sam, common.first_diff(got_sam, want_sam)
        assert open(os.path.join(d, "o.j")).read() == common.golden_junctions(run["base"]) and common.stats_block(r.stdout) == common.golden_stats(run["base"])
    # without the switch no table is written and everything else is the goldens'
    run = c["runs"][-1]
    r, lines = _run(d, ["-i", c["prefix"]] + files + ["-o", "plain.sam", "-j", "plain.j", "-t", "4"] + run["flags"], PIPELINES[pipeline])
    assert not lines and not os.path.exists(os.path.join(d, "plain.sam.genes.tab"))
    assert open(os.path.join(d, "plain.sam")).read() == common.golden_sam(run["base"]) and open(os.path.join(d, "plain.j")).read() == common.golden_junctions(run["base"])
    assert common.stats_block(r.stdout) == common.golden_stats(run["base"])


def test_dart_cli_gene_table_beside_other_switches_and_with_bam(workdir):
    c = common.build_case("pe101_spliced", workdir)
    d, files, n_genes, exons, order = _inputs(c, workdir, "more")
    run = c["runs"][1]
    args = ["-i", c["prefix"]] + files + ["-t", "4"] + run["flags"]
    want, counts = _expected(c, common.golden_sam(run["base"]), run["flags"], n_genes, exons, order)
    # beside the device's SAM formatter, FASTQ parser and junction table
    r, lines = _run(d, args + ["-o", "dev.sam", "-j", "dev.j"], {"DART_GENE_COUNTS": "ann.gtf", "DART_DEVICE_SAM": "1", "DART_DEVICE_FASTQ": "1", "DART_DEVICE_SJ": "1"})
    assert open(os.path.join(d, "dev.sam")).read() == common.golden_sam(run["base"]) and open(os.path.join(d, "dev.j")).read() == common.golden_junctions(run["base"])
    assert open(os.path.join(d, "dev.sam.genes.tab"), "rb").read() == want
    _line_ok(lines, counts)
    # -bo with the device's BAM: the table of the -o runs; the BAM is that of a run without the switch
    r, lines = _run(d, args + ["-bo", "a.bam", "-j", "a.j"], {"DART_GENE_COUNTS": "ann.gtf", "DART_DEVICE_BAM": "1"})
    assert open(os.path.join(d, "a.bam.genes.tab"), "rb").read() == want
    _line_ok(lines, counts)
    _run(d, args + ["-bo", "b.bam", "-j", "b.j"], {"DART_DEVICE_BAM": "1"})
    assert open(os.path.join(d, "a.bam"), "rb").read() == open(os.path.join(d, "b.bam"), "rb").read() and not os.path.exists(os.path.join(d, "b.bam.genes.tab"))
    # DART_GENE_MIN_MAPQ=0: nothing is multimapping; DART_GENE_FEATURE: another feature's lines (one gene, "other_feature")
    r, lines = _run(d, args + ["-o", "q0.sam", "-j", "q0.j"], {"DART_GENE_COUNTS": "ann.gtf", "DART_GENE_MIN_MAPQ": "0"})
    want0, counts0 = _expected(c, common.golden_sam(run["base"]), run["flags"], n_genes, exons, order, min_mapq=0)
    assert open(os.path.join(d, "q0.sam.genes.tab"), "rb").read() == want0 != want and counts0[1].sum() == 0
    r, lines = _run(d, args + ["-o", "gf.sam", "-j", "gf.j"], {"DART_GENE_COUNTS": "ann.gtf", "DART_GENE_FEATURE": "gene"})
    tab = open(os.path.join(d, "gf.sam.genes.tab")).read().splitlines()
    assert len(tab) == 5 and tab[4].startswith("other_feature\t") and [sum(int(l.split("\t")[k]) for l in tab) for k in (1, 2, 3)] == [int(counts[:, 0].sum())] * 3


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_dart_cli_gene_table_over_several_batches_and_two_device_slots(pipeline, workdir):
    """6002 reads in batches of 4000: two contexts count, the clone's table is merged into the root's.  Then three such libraries over DART_SAME_DEVICE_TIMES=2
    (device 0 opened twice: two roots, 2 x 2 contexts): the second root's table is downloaded and folded into the first; every library adds the same units"""
    import cli_inputs
    c, d = cli_inputs.make(workdir)
    n_genes, exons = gci.case_annotation(c, gci.CASE_SEEDS[c["name"]])
    order = gci.write_gtf(os.path.join(d, "ann.gtf"), exons, c["genome"].names)
    env = dict(PIPELINES[pipeline], DART_GENE_COUNTS="ann.gtf")
    r, lines = _run(d, ["-i", c["prefix"], "-f", "q1.fq", "-f2", "q2.fq", "-mis", "5", "-o", "g1.sam", "-j", "g1.j", "-t", "4"], env)
    (rd, rp, cg), npm = gci.sam_records(open(os.path.join(d, "g1.sam")).read(), 6002, True, c["genome"].names, False)
    counts = gci.twin(len(c["genome"].lengths), n_genes, exons, rd, rp, cg, npm, 4)
    names, rows = gci.table_in_file_order(counts, order)
    assert open(os.path.join(d, "g1.sam.genes.tab"), "rb").read() == sam.gene_table(names, rows)
    _line_ok(lines, counts)
    flags = ["-f", "q1.fq", "q1.fq", "q1.fq", "-f2", "q2.fq", "q2.fq", "q2.fq", "-mis", "5"]
    r, lines = _run(d, ["-i", c["prefix"]] + flags + ["-o", "g3.sam", "-j", "g3.j", "-t", "4"], dict(env, DART_SAME_DEVICE_TIMES="2", DART_INFLIGHT="2"))
    assert open(os.path.join(d, "g3.sam.genes.tab"), "rb").read() == sam.gene_table(names, 3 * rows)
    _line_ok(lines, 3 * counts)
    body = lambda t: [l for l in t.splitlines() if not l.startswith("@")]
    assert body(open(os.path.join(d, "g3.sam")).read()) == 3 * body(open(os.path.join(d, "g1.sam")).read())


def test_dart_cli_fatal_gtf_leaves_no_table(workdir):
    c = common.build_case("se100", workdir)
    d, files, n_genes, exons, order = _inputs(c, workdir, "fatal")
    good = open(os.path.join(d, "ann.gtf")).read().splitlines(True)
    name = c["genome"].names[0]
    line = lambda start, end, attrs='gene_id "x";', strand="+", seq=name: "%s\tt\texon\t%s\t%s\t.\t%s\t.\t%s\n" % (seq, start, end, strand, attrs)
    args = ["-i", c["prefix"]] + files + ["-o", "f.sam", "-j", "f.j", "-t", "2"]
    for tag, text, word in (("end", good[:3] + [line(50, 49)], "line 4: "), ("start", good[:2] + [line(0, 10)], "line 3: "), ("gene_id", good[:5] + [line(5, 10, 'gene_name "x";')], "line 6: "),
                            ("none", ["# nothing\n", line(5, 10, seq="elsewhere")], "no gene"), ("missing", None, "cannot read")):
        path = "bad_%s.gtf" % tag
        if text is not None:
            open(os.path.join(d, path), "w").write("".join(text))
        open(os.path.join(d, "f.sam.genes.tab"), "w").write("stale\n")
        for f in ("f.sam",):
            if os.path.exists(os.path.join(d, f)):
                os.remove(os.path.join(d, f))
        r, lines = _run(d, args, {"DART_GENE_COUNTS": path}, want_rc=1)
        assert word in r.stderr.decode() and "DART_GENE_COUNTS" in r.stderr.decode(), r.stderr[-400:]
        assert not os.path.exists(os.path.join(d, "f.sam.genes.tab")) and not os.path.exists(os.path.join(d, "f.sam")) and not lines
    # skipped lines are counted in one note, and the run goes on
    open(os.path.join(d, "skips.gtf"), "w").write("".join(good + [line(5, 10, seq="elsewhere"), line(5, 10, strand="."), line(7, 9, strand=".")]))
    r, lines = _run(d, args, {"DART_GENE_COUNTS": "skips.gtf"})
    notes = [l for l in r.stderr.decode().splitlines() if l.startswith("DART_GENE_COUNTS: skipped")]
    assert len(notes) == 1 and "skipped 1 " in notes[0] and " and 2 " in notes[0] and len(lines) == 1
    want, _ = _expected(c, common.golden_sam(c["runs"][0]["base"]), [], n_genes, exons, order)
    assert open(os.path.join(d, "f.sam.genes.tab"), "rb").read() == want
