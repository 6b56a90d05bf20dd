"""CPU suite: the GTF reader behind `dart`'s DART_GENE_COUNTS (dart_amd/csrc/host/gtf.h) through tests/native/gtf_checks.cpp: which lines count, how genes
are numbered, what is skipped and counted, and every fatal line with its number."""
import os, subprocess
import pytest
import common

NAMES = ["chr1", "chrTwo", "3"]


@pytest.fixture(scope="module")
def exe(workdir):
    out = os.path.join(workdir, "gtf_checks")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", out, os.path.join(common.ROOT, "tests", "native", "gtf_checks.cpp")])
    return out


def _run(exe, workdir, tag, text, feature="exon", names=NAMES):
    path = os.path.join(workdir, "gtf_%s.gtf" % tag)
    with open(path, "wb") as f:
        f.write(text.encode() if isinstance(text, str) else text)
    r = subprocess.run([exe, path, feature] + list(names), capture_output=True, text=True)
    genes, exons, skipped, err = [], [], None, None
    for line in r.stdout.splitlines():
        w = line.split(" ", 1)
        if w[0] == "gene":
            genes.append(w[1].split(" ", 1)[1])
        elif w[0] == "exon":
            exons.append(tuple(int(x) for x in w[1].split()))
        elif w[0] == "skipped":
            skipped = tuple(int(x) for x in w[1].split())
        elif w[0] == "error":
            err = w[1]
    assert (r.returncode == 0) == (err is None) and r.returncode in (0, 1), r.stdout + r.stderr
    return genes, exons, skipped, err


def L(seq="chr1", feature="exon", start=101, end=200, strand="+", attrs='gene_id "g1"; transcript_id "t1";', source="src", score=".", frame="."):
    return "\t".join([seq, source, feature, str(start), str(end), score, strand, frame, attrs]) + "\n"


def test_lines_that_count_and_how_genes_are_numbered(exe, workdir):
    text = "#!genome-build x\n# a comment with\ttabs\n" + L(attrs='gene_id "zeta"; transcript_id "t";') + L(feature="gene", attrs='gene_id "never";') + L(feature="CDS", attrs='gene_id "never";') \
        + L(seq="3", start=1, end=1, strand="-", attrs='transcript_id "t9"; gene_id "alpha"; gene_name "n";') + "\n" \
        + L(seq="chrTwo", start=5000, end=5999, attrs='gene_name "other_gene_id"; other_gene_id "no"; gene_id "zeta";') \
        + L(start=300, end=400, attrs='gene_id "with space; and semicolon" ; x "y"') + L(start=7, end=9, attrs="gene_id bare; x 1") + L(start=4294967295, end=4294967295, attrs='gene_id "alpha"') \
        + L(start=11, end=12, attrs='gene_id "crlf";').replace("\n", "\r\n")
    genes, exons, skipped, err = _run(exe, workdir, "basic", text)
    assert err is None and genes == ["zeta", "alpha", "with space; and semicolon", "bare", "crlf"] and skipped == (0, 0)      # first appearance, not name order
    assert exons == [(0, 100, 200, 0, 0), (2, 0, 1, 1, 1), (1, 4999, 5999, 0, 0), (0, 299, 400, 0, 2), (0, 6, 9, 0, 3), (0, 4294967294, 4294967295, 0, 1), (0, 10, 12, 0, 4)]
    # a custom feature name: the same file through its CDS lines
    genes, exons, skipped, err = _run(exe, workdir, "cds", text, feature="CDS")
    assert err is None and genes == ["never"] and exons == [(0, 100, 200, 0, 0)]
    # no final newline
    genes, exons, _, err = _run(exe, workdir, "nonl", L().rstrip("\n"))
    assert err is None and exons == [(0, 100, 200, 0, 0)]


def test_skipped_lines_are_counted(exe, workdir):
    text = L() + L(seq="chrUn") + L(seq="chr1 ") + L(strand=".") + L(strand="?") + L(strand="+-") + L(seq="chrUn", strand=".") + L(feature="gene", seq="chrUn") \
        + L(seq="chrUn", start=0, end=-5, attrs="") + L(strand=".", start=9, end=2, attrs="")          # a skipped line is not looked at further
    genes, exons, skipped, err = _run(exe, workdir, "skipped", text)
    assert err is None and genes == ["g1"] and len(exons) == 1 and skipped == (4, 4)


@pytest.mark.parametrize("tag, bad, word", [("end_below_start", L(start=200, end=199), "below start"), ("start_zero", L(start=0, end=5), "below 1"), ("start_negative", L(start=-3, end=5), "below 1"),
                                            ("no_gene_id", L(attrs='transcript_id "t"; gene_name "g";'), "gene_id"), ("empty_gene_id", L(attrs='gene_id "";'), "gene_id"),
                                            ("other_gene_id", L(attrs='other_gene_id "x";'), "gene_id"), ("no_number", L(start="12a"), "not a number"),
                                            ("eight_fields", "chr1\tsrc\texon\t1\t2\t.\t+\t.\n", "nine"), ("end_too_large", L(end=4294967296), "2^32")])
def test_each_fatal_line_with_its_number(tag, bad, word, exe, workdir):
    text = "# header\n" + L() + L(feature="gene", start=9, end=1) + bad + L(start=0, end=0)          # (another feature's coordinates are not looked at; a later bad line is not the one named)
    genes, exons, skipped, err = _run(exe, workdir, tag, text)
    assert err is not None and err.startswith("line 4: ") and word in err and not genes and not exons


def test_no_gene_at_all(exe, workdir):
    for tag, text in (("empty", ""), ("comments", "# nothing\n"), ("other_features", L(feature="gene") + L(feature="CDS")), ("foreign", L(seq="chrUn") + L(strand="."))):
        genes, exons, skipped, err = _run(exe, workdir, "none_" + tag, text)
        assert err is not None and "no gene" in err
    r = subprocess.run([exe, os.path.join(workdir, "does_not_exist.gtf"), "exon", "chr1"], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot read" in r.stdout
