"""CPU suite: the checker pinned on genomes of 32 b to 130 kb (tests/small_genome_inputs.py) before the GPU tests rely on it there
(tests/test_gpu_small_genomes.py).  Per genome: the CPU index builder's five files are the bytes the reference's indexer wrote; the
oracle's command line writes the SAM, the junctions and the statistics the reference's object code wrote for every run
(tests/golden/small_genomes.json, made by tests/golden/make_small_genomes.py; where oracle/_ref exists the reference also runs live beside
it); and the runs are worth comparing: at least half of the reads map, and from 4096 bases on re-seeding and the junction code run."""
import json, os
import numpy as np
import pytest
import common, oracle_py
import small_genome_inputs as sgi
import test_oracle_vs_ref as t
from dart_amd import index_build

GOLD_PATH = os.path.join(common.GOLDEN, "small_genomes.json")


def gold():
    return json.load(open(GOLD_PATH))


def oracle_figures(orc, name, paired, flags):
    """the counts of one run from the oracle's library on the run's batch: reads, mapped reads, re-seeding calls, junction tuples"""
    p, _ = common.parse_flags(flags)
    so, rl, flat = sgi.batch(name, paired)
    reads, rep, cig, sj = orc.map_batch(orc.params(paired=int(paired), **p), so, rl, flat)
    return {"n_reads": len(rl), "n_mapped": int((reads["score"] > 0).sum()), "n_reseed": orc.counters["n_reseed"], "n_junction_tuples": len(sj)}


def check_not_vacuous(name, fig):
    assert 2 * fig["n_mapped"] >= fig["n_reads"], (name, fig)
    if sgi.l_pac(name) >= sgi.LONG_GAP_MIN:
        assert fig["n_reseed"] > 0 and fig["n_junction_tuples"] > 0, (name, fig)


def prepare(name, workdir):
    """the genome's FASTA, reads and CPU-built index under workdir -> (directory, prefix, single-end files, paired files or None)"""
    d = os.path.join(workdir, "small_" + name)
    se, pe = sgi.write_inputs(name, d)
    prefix = os.path.join(d, "g")
    if not os.path.exists(prefix + ".sa"):
        index_build.build_index_from_genome(sgi.make_genome(name), prefix, device="cpu")
    return d, prefix, se, pe


@pytest.mark.parametrize("name", sgi.NAMES)
def test_small_genome_inputs_and_cpu_index_are_the_recorded_ones(name, workdir):
    g = gold()["genomes"][name]
    assert sgi.codes_sha256(name) == g["codes_sha256"], "the genome generator drifted from the recorded inputs"
    pe = sgi.paired_reads(name)
    assert sgi.reads_sha256(sgi.single_reads(name)) == g["reads_sha256"]["se"] and (sgi.reads_sha256(pe[0] + pe[1]) if pe else None) == g["reads_sha256"]["pe"]
    assert sgi.expected_k(name) == g["K"]
    d, prefix, se, pe_files = prepare(name, workdir)
    for ext, want in g["index_sha256"].items():
        assert common.sha(prefix + "." + ext) == want, "CPU-built .%s differs from the reference indexer's (%s)" % (ext, name)


@pytest.mark.parametrize("name", sgi.NAMES)
def test_oracle_matches_reference_on_small_genome(name, workdir):
    oracle_py.build()
    d, prefix, se, pe_files = prepare(name, workdir)
    runs = gold()["runs"]
    orc = oracle_py.Oracle(prefix)
    try:
        for key, paired, flags in sgi.runs(name):
            t.run_both(d, prefix, (pe_files if paired else se) + flags, key, want=runs[key])
            fig = oracle_figures(orc, name, paired, flags)
            assert fig == {k: runs[key][k] for k in fig}, (key, fig)
            assert fig["n_mapped"] == runs[key]["n_mapped_reference"]
            check_not_vacuous(name, fig)
    finally:
        orc.close()
