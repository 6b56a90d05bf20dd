"""GPU suite: `dart` with DART_TX_QUANT=<annotation.gtf> -- equivalence classes on the device batch by batch (dg_batch_accumulate_tx, dg_tx_merge), the EM at the
end of the job (dg_tx_finish) -- in both host pipelines, with -o and -bo, against the Python twin (tests/txquant_inputs.py) run over the SAM file the same run
wrote.  The alignments, the BAM and the junctions are those of a run without the switch; a GTF or a value that cannot be used ends the run with no output."""
import os, re, subprocess
import numpy as np
import pytest
import common, genecount_inputs as gci, txquant_inputs as txi
from dart_amd import synth, host

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
PIPELINES = {"parallel": {}, "streaming": {"DART_STREAMING": "1"}}
CASE = "pe101_spliced"


def _run(d, args, extra, want_rc=0):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="4000")
    env.update(extra)
    r = subprocess.run([DART] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == want_rc, r.stderr[-800:]
    return r, [l for l in r.stderr.decode("latin1").splitlines() if l.startswith("[dart timing] tx:")]


def _inputs(c, workdir, tag):
    d = os.path.join(workdir, "tx_%s_%s" % (tag, c["name"])); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1); synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2)
    tr = txi.case_annotation(c, txi.CASE_SEEDS[c["name"]])
    names = txi.write_gtf(os.path.join(d, "ann.gtf"), tr, c["genome"].names)
    return d, ["-f", "1.fq", "-f2", "2.fq"], tr, names


def _expected(c, sam_text, flags, tr, names, strand_mode=0, frag_mean=200, max_rounds=1000):
    _, h = common.parse_flags(flags)
    (rd, rp, cg), npm = gci.sam_records(sam_text, len(c["reads"]), True, c["genome"].names, h["unique"])
    classes, words = txi.twin(tr, len(c["genome"].lengths), rd, rp, cg, npm, 4, strand_mode)
    L = txi.lengths(tr)
    res = txi.em(classes, words, L, frag_mean, max_rounds, strand_mode)
    text = txi.text(res, L, names)
    tx, ex = txi.annot_arrays(tr)
    assert host.tx_text(host._load_lib(), np.array(res, np.uint64), tx, ex, names) == text          # dg_tx_format of the twin's words
    return text, res


def _line_ok(lines, res):
    assert len(lines) == 1 and "em_ms=" in lines[0], lines
    w = res[len(res) - 16:]
    for name, v in zip(txi.WORD_NAMES, w):
        assert int(re.search(r" %s=(\d+)" % name, lines[0]).group(1)) == v, (name, lines[0])


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_dart_cli_transcript_table_equals_the_twin_over_its_own_sam(pipeline, workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case(CASE, workdir)
    d, files, tr, names = _inputs(c, workdir, pipeline)
    run = c["runs"][1]
    args = ["-i", c["prefix"]] + files + ["-t", "4"] + run["flags"]
    # -o: the table against the twin over the run's own SAM; the SAM, the junctions and the statistics are the goldens'
    r, lines = _run(d, args + ["-o", "o.sam", "-j", "o.j"], dict(PIPELINES[pipeline], DART_TX_QUANT="ann.gtf"))
    got_sam = open(os.path.join(d, "o.sam")).read()
    want, res = _expected(c, got_sam, run["flags"], tr, names)
    got = open(os.path.join(d, "o.sam.transcripts.tab"), "rb").read()
    assert got == want, common.first_diff(got.decode(), want.decode())
    _line_ok(lines, res)
    assert res[len(tr) + 4] > 100 and res[len(tr) + 9] == 1
    assert got_sam == common.golden_sam(run["base"]) and open(os.path.join(d, "o.j")).read() == common.golden_junctions(run["base"])
    assert common.stats_block(r.stdout) == common.golden_stats(run["base"])
    # without the switch: no table, no line, the same files
    r, lines = _run(d, args + ["-o", "plain.sam", "-j", "plain.j"], PIPELINES[pipeline])
    assert not lines and not os.path.exists(os.path.join(d, "plain.sam.transcripts.tab"))
    assert open(os.path.join(d, "plain.sam")).read() == got_sam and open(os.path.join(d, "plain.j")).read() == open(os.path.join(d, "o.j")).read()
    # -bo: the same table; the BAM and the junctions are those of a run without the switch.  Another strand mode, mean and round count: the twin's again
    r, lines = _run(d, args + ["-bo", "a.bam", "-j", "a.j"], dict(PIPELINES[pipeline], DART_TX_QUANT="ann.gtf"))
    assert open(os.path.join(d, "a.bam.transcripts.tab"), "rb").read() == want
    _line_ok(lines, res)
    _run(d, args + ["-bo", "b.bam", "-j", "b.j"], PIPELINES[pipeline])
    assert open(os.path.join(d, "a.bam"), "rb").read() == open(os.path.join(d, "b.bam"), "rb").read() and not os.path.exists(os.path.join(d, "b.bam.transcripts.tab"))
    assert open(os.path.join(d, "a.j")).read() == open(os.path.join(d, "b.j")).read() == open(os.path.join(d, "o.j")).read()
    r, lines = _run(d, args + ["-o", "s.sam", "-j", "s.j"], dict(PIPELINES[pipeline], DART_TX_QUANT="ann.gtf", DART_TX_STRAND="2", DART_TX_FRAG_MEAN="150", DART_TX_MAX_ROUNDS="5"))
    want2, res2 = _expected(c, got_sam, run["flags"], tr, names, strand_mode=2, frag_mean=150, max_rounds=5)
    assert open(os.path.join(d, "s.sam.transcripts.tab"), "rb").read() == want2 != want
    _line_ok(lines, res2)


def test_dart_cli_tx_over_several_batches_and_two_device_slots(workdir):
    """6002 reads in batches of 4000: two contexts count, the clone's table is merged into the root's.  Then three such libraries over DART_SAME_DEVICE_TIMES=2
    (device 0 opened twice: two roots): the second root's table is downloaded and folded into the first; every library adds the same units"""
    import cli_inputs
    c, d = cli_inputs.make(workdir)
    tr = txi.case_annotation(c, txi.CASE_SEEDS[c["name"]])
    names = txi.write_gtf(os.path.join(d, "tx.gtf"), tr, c["genome"].names)
    env = dict(DART_TX_QUANT="tx.gtf", DART_TX_MAX_ROUNDS="32")
    r, lines = _run(d, ["-i", c["prefix"], "-f", "q1.fq", "-f2", "q2.fq", "-mis", "5", "-o", "t1.sam", "-j", "t1.j", "-t", "4"], env)
    (rd, rp, cg), npm = gci.sam_records(open(os.path.join(d, "t1.sam")).read(), 6002, True, c["genome"].names, False)
    one = txi.twin(tr, len(c["genome"].lengths), rd, rp, cg, npm, 4)
    L = txi.lengths(tr)
    res = txi.em(one[0], one[1], L, 200, 32)
    assert open(os.path.join(d, "t1.sam.transcripts.tab"), "rb").read() == txi.text(res, L, names)
    _line_ok(lines, res)
    flags = ["-f", "q1.fq", "q1.fq", "q1.fq", "-f2", "q2.fq", "q2.fq", "q2.fq", "-mis", "5"]
    r, lines = _run(d, ["-i", c["prefix"]] + flags + ["-o", "t3.sam", "-j", "t3.j", "-t", "4"], dict(env, DART_SAME_DEVICE_TIMES="2", DART_INFLIGHT="2"))
    three = txi.add_tables(txi.add_tables(one, one), one)
    res3 = txi.em(three[0], three[1], L, 200, 32)
    assert open(os.path.join(d, "t3.sam.transcripts.tab"), "rb").read() == txi.text(res3, L, names)
    _line_ok(lines, res3)


def test_dart_cli_a_gtf_or_a_value_that_cannot_be_used_leaves_no_output(workdir):
    c = common.build_case(CASE, workdir)
    d, files, tr, names = _inputs(c, workdir, "fatal")
    good = open(os.path.join(d, "ann.gtf")).read().splitlines(True)
    name = c["genome"].names[0]
    args = ["-i", c["prefix"]] + files + ["-o", "f.sam", "-j", "f.j", "-t", "2"]
    line = lambda start, end, attrs='transcript_id "x";': "%s\tt\texon\t%s\t%s\t.\t+\t.\t%s\n" % (name, start, end, attrs)
    for tag, text, word in (("end", good[:3] + [line(50, 49)], "line 4: "), ("id", good[:5] + [line(5, 10, 'gene_id "x";')], "line 6: "), ("none", ["# nothing\n"], "no transcript"), ("missing", None, "cannot read")):
        path = "bad_%s.gtf" % tag
        if text is not None:
            open(os.path.join(d, path), "w").write("".join(text))
        open(os.path.join(d, "f.sam.transcripts.tab"), "w").write("stale\n")
        r, lines = _run(d, args, {"DART_TX_QUANT": path}, want_rc=1)
        assert word in r.stderr.decode() and "DART_TX_QUANT" in r.stderr.decode(), r.stderr[-400:]
        assert not any(os.path.exists(os.path.join(d, f)) for f in ("f.sam.transcripts.tab", "f.sam", "f.j")) and not lines
    for var, value in (("DART_TX_STRAND", "3"), ("DART_TX_FRAG_MEAN", "0"), ("DART_TX_MAX_ROUNDS", "lots")):
        r, lines = _run(d, args, {"DART_TX_QUANT": "ann.gtf", var: value}, want_rc=1)
        assert ("%s=%s" % (var, value)) in r.stderr.decode(), r.stderr[-400:]
        assert not any(os.path.exists(os.path.join(d, f)) for f in ("f.sam.transcripts.tab", "f.sam", "f.j")) and not lines
