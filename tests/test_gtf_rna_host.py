"""CPU suite: the transcript reader behind `dart`'s DART_RNA_METRICS (dart_amd/csrc/host/gtf.h, gtf_parse_transcripts) through tests/native/gtf_rna_checks.cpp
against expected tables: how exon lines are grouped, where the CDS and the ribosomal flag come from, what is skipped and counted, and one failing line per
fatal rule with its number.  Built plain and with the address and undefined-behaviour sanitizers; the program stands alone."""
import os, subprocess
import pytest
import common

NAMES = ["chr1", "chrTwo", "3"]


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan+ubsan"])
def exe(request, workdir):
    out = os.path.join(workdir, "gtf_rna_checks_san" if request.param else "gtf_rna_checks")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall"] + flags + ["-o", out, os.path.join(common.ROOT, "tests", "native", "gtf_rna_checks.cpp")])
    return out


def _run(exe, workdir, tag, text, names=NAMES):
    path = os.path.join(workdir, "gtf_rna_%s.gtf" % tag)
    with open(path, "wb") as f:
        f.write(text.encode() if isinstance(text, str) else text)
    r = subprocess.run([exe, path] + list(names), capture_output=True, text=True)
    tx, exons, skipped, err = [], [], None, None
    for line in r.stdout.splitlines():
        w = line.split(" ", 1)
        if w[0] == "tx":
            f = w[1].split(" ", 8)
            tx.append(tuple(int(x) for x in f[1:8]) + (f[8],))
        elif w[0] == "exon":
            exons.append(tuple(int(x) for x in w[1].split()))
        elif w[0] == "skipped":
            skipped = tuple(int(x) for x in w[1].split())
        elif w[0] == "error":
            err = w[1]
    assert (r.returncode == 0) == (err is None) and r.returncode in (0, 1), r.stdout + r.stderr
    return tx, exons, skipped, err


def L(seq="chr1", feature="exon", start=101, end=200, strand="+", attrs='gene_id "g1"; transcript_id "t1";', source="src", score=".", frame="."):
    return "\t".join([seq, source, feature, str(start), str(end), score, strand, frame, attrs]) + "\n"


def test_transcripts_exons_cds_and_the_ribosomal_flag(exe, workdir):
    t = lambda name, more="": 'gene_id "g"; transcript_id "%s"; %s' % (name, more)
    text = "#!genome-build x\n" + L(attrs=t("zeta")) + L(feature="gene", attrs='gene_id "g";') + L(feature="transcript", start=1, end=9999, attrs=t("zeta")) \
        + L(feature="CDS", start=150, end=180, attrs=t("zeta")) + L(start=301, end=400, attrs=t("zeta")) + L(feature="stop_codon", start=398, end=400, attrs=t("zeta")) \
        + L(feature="start_codon", start=120, end=122, attrs=t("zeta")) \
        + L(seq="3", start=1, end=1, strand="-", attrs='transcript_id "alpha"; gene_biotype "rRNA";') + L(seq="chrTwo", start=5000, end=5999, attrs=t("zeta")) \
        + L(start=51, end=60, attrs=t("zeta")) + L(start=7, end=9, attrs="transcript_id bare; gene_type Mt_rRNA") + L(start=7, end=9, strand="-", attrs=t("p", 'transcript_biotype "rRNA_pseudogene";')) \
        + L(start=11, end=12, attrs=t("near", 'gene_biotype "rRNA_like"; transcript_type "rRNA";')).replace("\n", "\r\n") + L(feature="CDS", start=1, end=5, attrs=t("cds_only")) \
        + L(feature="CDS", start=20, end=30, attrs='gene_id "no transcript";') + L(start=4294967295, end=4294967295, attrs=t("alpha"))
    tx, exons, skipped, err = _run(exe, workdir, "basic", text)
    assert err is None and skipped == (0, 0)
    # first appearance, not name order; zeta on chrTwo is a transcript of its own; the CDS is the smallest start and the largest end over CDS and codon lines;
    # a transcript with only CDS lines is dropped; alpha on another sequence and strand is another transcript
    assert tx == [(0, 0, 0, 119, 400, 3, 0, "zeta"), (2, 1, 1, 0, 0, 1, 3, "alpha"), (1, 0, 0, 0, 0, 1, 4, "zeta"), (0, 0, 1, 0, 0, 1, 5, "bare"), (0, 1, 1, 0, 0, 1, 6, "p"),
                  (0, 0, 0, 0, 0, 1, 7, "near"), (0, 0, 0, 0, 0, 1, 8, "alpha")]
    assert exons == [(100, 200), (300, 400), (50, 60), (0, 1), (4999, 5999), (6, 9), (6, 9), (10, 12), (4294967294, 4294967295)]
    tx, exons, _, err = _run(exe, workdir, "nonl", L().rstrip("\n"))
    assert err is None and tx == [(0, 0, 0, 0, 0, 1, 0, "t1")] and exons == [(100, 200)]


def test_skipped_lines_are_counted(exe, workdir):
    text = L() + L(seq="chrUn") + L(seq="chr1 ") + L(strand=".") + L(strand="?", feature="CDS") + L(strand="+-") + L(seq="chrUn", strand=".") + L(feature="gene", seq="chrUn") \
        + L(seq="chrUn", start=0, end=-5, attrs="") + L(strand=".", start=9, end=2, attrs="")          # a skipped line is not looked at further
    tx, exons, skipped, err = _run(exe, workdir, "skipped", text)
    assert err is None and len(tx) == 1 and len(exons) == 1 and skipped == (4, 4)


@pytest.mark.parametrize("tag, bad, word", [("end_below_start", L(start=200, end=199), "below start"), ("start_zero", L(start=0, end=5), "below 1"), ("cds_start_negative", L(feature="CDS", start=-3, end=5), "below 1"),
                                            ("no_transcript_id", L(attrs='gene_id "g"; gene_name "n";'), "transcript_id"), ("empty_transcript_id", L(attrs='transcript_id "";'), "transcript_id"),
                                            ("other_transcript_id", L(attrs='other_transcript_id "x";'), "transcript_id"), ("no_number", L(start="12a"), "not a number"),
                                            ("eight_fields", "chr1\tsrc\texon\t1\t2\t.\t+\t.\n", "nine"), ("end_too_large", L(feature="stop_codon", end=4294967296), "2^32")])
def test_each_fatal_line_with_its_number(tag, bad, word, exe, workdir):
    text = "# header\n" + L() + L(feature="gene", start=9, end=1) + bad + L(start=0, end=0)          # (another feature's coordinates are not looked at; a later bad line is not the one named)
    tx, exons, skipped, err = _run(exe, workdir, tag, text)
    assert err is not None and err.startswith("line 4: ") and word in err and not tx and not exons


def test_no_transcript_at_all(exe, workdir):
    for tag, text in (("empty", ""), ("comments", "# nothing\n"), ("other_features", L(feature="gene") + L(feature="CDS")), ("foreign", L(seq="chrUn") + L(strand="."))):
        tx, exons, skipped, err = _run(exe, workdir, "none_" + tag, text)
        assert err is not None and "no transcript" in err
    r = subprocess.run([exe, os.path.join(workdir, "does_not_exist.gtf"), "chr1"], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot read" in r.stdout
