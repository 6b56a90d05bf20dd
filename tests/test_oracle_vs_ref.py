"""CPU suite: the oracle's command line against the reference's own object code, byte for byte, on input-format variants and a seeded
fuzz.  What the reference wrote for these runs (statistics block, SHA-256 of its SAM and junction files, its indexer's files) is recorded
in tests/golden/oracle_vs_ref.json (tests/golden/make_oracle_vs_ref.py); where oracle/_ref exists the reference also runs live beside it."""
import hashlib, json, os, subprocess
import numpy as np
import pytest
import common, oracle_py, cli_inputs
from dart_amd import synth, index_build

GOLD_PATH = os.path.join(common.GOLDEN, "oracle_vs_ref.json")
LIVE = os.path.exists(oracle_py.REF_HARNESS) and os.path.exists(oracle_py.REF_INDEXER)

FUZZ_FLAGS = ([], ["-mis", "5"], ["-mis", "4", "-unique", "-max_dup", "500"])
ODD_FLAGS = (["-f", "a.fq", "-f2", "b.fq", "-mis", "12"], ["-f", "a.fq", "-mis", "30"], ["-f", "a.fq", "b.fq", "-mis", "12", "-m"])
INDEX_EXT = ("amb", "ann", "bwt", "pac", "sa")


def gold():
    return json.load(open(GOLD_PATH))


def run_key(label, flags):
    return label + ": " + " ".join(flags)


def run_ref(d, prefix, flags):
    """the reference's object code on one run: (statistics block, SAM text, junction text)"""
    rr = subprocess.run([oracle_py.REF_HARNESS, "map", "-i", prefix] + flags + ["-o", "ref.sam", "-j", "ref.j"], cwd=d, stdout=subprocess.PIPE, check=True)
    return common.stats_block(rr.stdout), open(os.path.join(d, "ref.sam")).read(), open(os.path.join(d, "ref.j")).read()


def recorded(stats, sam, junc):
    return {"stats": stats, "sam_sha256": hashlib.sha256(sam.encode()).hexdigest(), "junctions_sha256": hashlib.sha256(junc.encode()).hexdigest()}


def run_both(d, prefix, flags, key, want=None):
    """want: the run's recorded entry where it is not one of tests/golden/oracle_vs_ref.json's"""
    ro = subprocess.run([oracle_py.ORACLE_CLI, "-i", prefix] + flags + ["-o", "orc.sam", "-j", "orc.j", "-t", "3"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    stats, sam, junc = common.stats_block(ro.stdout), open(os.path.join(d, "orc.sam")).read(), open(os.path.join(d, "orc.j")).read()
    if LIVE:
        # the statistics block of stdout (Mapping.cpp:812-822): the harness prints it from the reference's own counters
        r_stats, r_sam, r_junc = run_ref(d, prefix, flags)
        assert r_stats == stats != "", (r_stats[-600:], stats[-600:])
        assert r_sam == sam, common.first_diff(sam, r_sam)
        assert r_junc == junc
    if want is None:
        want = gold()["runs"][key]
    assert stats == want["stats"] != "", (stats, want["stats"])
    got = recorded(stats, sam, junc)
    assert got["sam_sha256"] == want["sam_sha256"], "the oracle's SAM differs from the reference's recorded output (%s)" % key
    assert got["junctions_sha256"] == want["junctions_sha256"], "the oracle's junctions differ from the reference's recorded output (%s)" % key


def index_fasta(d, name):
    """g.fa -> index prefix g: the reference's indexer where it exists, else our builder, whose five files must be the ones the reference's
    indexer wrote for this genome"""
    prefix = os.path.join(d, "g")
    if LIVE:
        subprocess.run([oracle_py.REF_INDEXER, "g.fa", "g"], cwd=d, stdout=subprocess.DEVNULL, check=True)
    else:
        index_build.build_index_from_fasta(os.path.join(d, "g.fa"), prefix, device="cpu")
    for ext, want in gold()["index_sha256"][name].items():
        assert common.sha(prefix + "." + ext) == want, "index file .%s differs from the reference indexer's (%s)" % (ext, name)
    return prefix


def fuzz_inputs(workdir):
    """a genome and reads that are in no fixture: repeats-heavy, short reads, 3 % errors"""
    d = os.path.join(workdir, "fuzz"); os.makedirs(d, exist_ok=True)
    g = synth.make_genome([700000, 300000], seed=91, repeat_scale=80.0, n_introns=200)
    g.write_fasta(os.path.join(d, "g.fa"))
    m1, m2 = synth.make_reads(g, 6000, rlen=76, seed=92, spliced_frac=0.25, sub_rate=0.03, indel_frac=0.05, n_frac=0.02)
    synth.write_fastq(os.path.join(d, "a.fq"), m1, 1); synth.write_fastq(os.path.join(d, "b.fq"), m2, 2)
    return d


def odd_inputs(workdir):
    """fresh genome, paired and single-end reads with a literal '-' (a gap to AddNewCigarElements), lower case, N and IUPAC letters planted
    at 1 % of the positions"""
    d = os.path.join(workdir, "fuzz_odd"); os.makedirs(d, exist_ok=True)
    g = synth.make_genome([500000, 250000], seed=191, repeat_scale=40.0, n_introns=300)
    g.write_fasta(os.path.join(d, "g.fa"))
    rng = np.random.default_rng(192)
    m1, m2 = synth.make_reads(g, 5000, rlen=125, seed=193, spliced_frac=0.4, sub_rate=0.01, indel_frac=0.2, n_frac=0.0)
    def odd(m):
        return np.where(rng.random(m.shape) < 0.01, rng.choice(np.frombuffer(b"---acgtRYn", np.uint8), size=m.shape), m).astype(np.uint8)
    synth.write_fastq(os.path.join(d, "a.fq"), odd(m1), 1); synth.write_fastq(os.path.join(d, "b.fq"), odd(m2), 2)
    return d


@pytest.mark.parametrize("flags,label", cli_inputs.VARIANTS, ids=[v[1] for v in cli_inputs.VARIANTS])
def test_oracle_cli_matches_reference_on_input_variants(flags, label, workdir):
    oracle_py.build()
    c, d = cli_inputs.make(workdir)
    run_both(d, c["prefix"], flags, run_key(label, flags))


def test_oracle_matches_reference_on_fresh_fuzz(workdir):
    """a genome and reads that are in no fixture: repeats-heavy, short reads, 3 % errors"""
    oracle_py.build()
    d = fuzz_inputs(workdir)
    prefix = index_fasta(d, "fuzz")
    for flags in FUZZ_FLAGS:
        flags = ["-f", "a.fq", "-f2", "b.fq"] + flags
        run_both(d, prefix, flags, run_key("fuzz", flags))


def test_oracle_matches_reference_on_reads_with_odd_characters(workdir):
    """fresh genome, paired and single-end reads with a literal '-' (a gap to AddNewCigarElements), lower case, N and IUPAC letters planted at 1 % of the positions,
    -mis 12 and 30: the reads that reach the reference's string code in ways the ACGTN fixtures do not"""
    oracle_py.build()
    d = odd_inputs(workdir)
    prefix = index_fasta(d, "fuzz_odd")
    for flags in ODD_FLAGS:
        run_both(d, prefix, flags, run_key("fuzz_odd", flags))
