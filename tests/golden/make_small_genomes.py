"""Regenerates tests/golden/small_genomes.json: what the REFERENCE's object code (oracle/_ref, built by `make -C oracle ref` where the
reference tree exists) writes for the genomes and runs of tests/small_genome_inputs.py -- per genome the SHA-256 of the codes and of the
read sets and the digests of its indexer's five files; per run the statistics block of its stdout, the SHA-256 of its SAM and junction
files, the number of mapped reads, and the oracle's n_reseed and junction tuples for the same batch.  Digests and counts only.  It also
asserts, on the oracle alone, what keeps the GPU tests of these runs from being vacuous: at least half of the reads of every run map, and on
every genome of 4096 bases or more re-seeding runs and junction tuples are written.  Runs only where oracle/_ref exists.

  python tests/golden/make_small_genomes.py
"""
import json, os, re, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE))
import common, oracle_py
import small_genome_inputs as sgi
import test_oracle_vs_ref as t
import test_small_genomes_oracle as ts

assert t.LIVE, "oracle/_ref is not built"
oracle_py.build()
work = tempfile.mkdtemp()
out = {"genomes": {}, "runs": {}}
for name in sgi.NAMES:
    d = os.path.join(work, name)
    se_files, pe_files = sgi.write_inputs(name, d)
    subprocess.run([oracle_py.REF_INDEXER, "g.fa", "g"], cwd=d, stdout=subprocess.DEVNULL, check=True)
    pe = sgi.paired_reads(name)
    out["genomes"][name] = {"codes_sha256": sgi.codes_sha256(name), "K": sgi.expected_k(name),
                            "reads_sha256": {"se": sgi.reads_sha256(sgi.single_reads(name)), "pe": sgi.reads_sha256(pe[0] + pe[1]) if pe else None},
                            "index_sha256": {ext: common.sha(os.path.join(d, "g." + ext)) for ext in sgi.INDEX_EXT}}
    orc = oracle_py.Oracle(os.path.join(d, "g"))
    for key, paired, flags in sgi.runs(name):
        stats, sam, junc = t.run_ref(d, os.path.join(d, "g"), (pe_files if paired else se_files) + flags)
        ent = t.recorded(stats, sam, junc)
        ent.update(ts.oracle_figures(orc, name, paired, flags))
        ent["n_mapped_reference"] = int(re.search(r"# of total mapped reads = (\d+)", stats).group(1))
        ts.check_not_vacuous(name, ent)
        assert ent["n_mapped_reference"] == ent["n_mapped"], (key, ent)
        out["runs"][key] = ent
        print("%-48s reads %4d mapped %4d n_reseed %4d junction tuples %4d" % (key, ent["n_reads"], ent["n_mapped"], ent["n_reseed"], ent["n_junction_tuples"]))
    orc.close()
json.dump(out, open(os.path.join(HERE, "small_genomes.json"), "w"), indent=1, sort_keys=True)
