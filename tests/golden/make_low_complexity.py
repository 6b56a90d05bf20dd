"""Regenerates tests/golden/low_complexity.json: what the REFERENCE's object code (oracle/_ref, built by `make -C oracle ref` where the
reference tree exists) writes for the genomes and runs of tests/low_complexity_inputs.py -- per genome the SHA-256 of the codes and of the
read sets and the digests of its indexer's five files; per run the statistics block of its stdout, the SHA-256 of its SAM and junction
files, the number of mapped reads, and the oracle's counts for the same batch (mapped reads, mapped reads with more than one place, junction
tuples); for the ladder, per rung its copy count, the reads inside it and how many of them map under max_dup 100 and 1000.  Digests and counts
only.  It asserts what keeps the GPU tests of these runs from being vacuous (tests/test_low_complexity_oracle.py::check_not_vacuous,
check_ladder).  Runs only where oracle/_ref exists.

  python tests/golden/make_low_complexity.py
"""
import json, os, re, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE))
import common, oracle_py
import low_complexity_inputs as lci
import test_oracle_vs_ref as t
import test_low_complexity_oracle as tl

assert t.LIVE, "oracle/_ref is not built"
oracle_py.build()
work = tempfile.mkdtemp()
out = {"genomes": {}, "runs": {}}
for name in lci.NAMES:
    d = os.path.join(work, name)
    se_files, pe_files = lci.write_inputs(name, d)
    subprocess.run([oracle_py.REF_INDEXER, "g.fa", "g"], cwd=d, stdout=subprocess.DEVNULL, check=True)
    pe = lci.paired_reads(name)
    out["genomes"][name] = {"codes_sha256": lci.codes_sha256(name),
                            "reads_sha256": {"se": lci.reads_sha256(lci.single_reads(name)), "pe": lci.reads_sha256(pe[0] + pe[1])},
                            "index_sha256": {ext: common.sha(os.path.join(d, "g." + ext)) for ext in lci.INDEX_EXT}}
    orc = oracle_py.Oracle(os.path.join(d, "g"))
    figs, mapped = {}, {}
    for key, paired, flags in lci.runs(name):
        stats, sam, junc = t.run_ref(d, os.path.join(d, "g"), (pe_files if paired else se_files) + flags)
        ent = t.recorded(stats, sam, junc)
        rec = tl.oracle_records(orc, name, paired, flags)
        figs[key] = tl.figures_of(rec)
        mapped[key] = rec[0]["score"] > 0
        ent.update(figs[key])
        ent["n_mapped_reference"] = int(re.search(r"# of total mapped reads = (\d+)", stats).group(1))
        ent["n_sam_lines"] = sam.count("\n")
        assert ent["n_mapped_reference"] == ent["n_mapped"], (key, ent)
        out["runs"][key] = ent
        print("%-52s reads %4d mapped %4d multi %4d junction tuples %4d SAM lines %6d" % (key, ent["n_reads"], ent["n_mapped"], ent["n_multi"], ent["n_junction_tuples"], ent["n_sam_lines"]))
    tl.check_not_vacuous(name, figs)
    if name == "ladder":
        rungs = tl.ladder_figures(mapped["ladder se: -mis 5"], mapped["ladder " + lci.MULTI_RUN])
        for r in rungs: print("  rung", r)
        out["ladder"] = {"copies": lci.rung_copies(), "rungs": rungs, "n_rungs_that_differ_between_max_dup_100_and_1000": tl.check_ladder(rungs)}
    orc.close()
json.dump(out, open(os.path.join(HERE, "low_complexity.json"), "w"), indent=1, sort_keys=True)
