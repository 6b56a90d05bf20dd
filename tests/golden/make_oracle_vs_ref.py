"""Regenerates tests/golden/oracle_vs_ref.json: what the REFERENCE's object code (oracle/_ref, built by `make -C oracle ref` where the
reference tree exists) writes for the runs of tests/test_oracle_vs_ref.py -- the statistics block of its stdout, the SHA-256 of its SAM and
junction files, the SHA-256 of the files its indexer writes for the two fuzz genomes -- and what its eva / SJ_Eva / FluxEva print for the
files of tests/test_evaluate.py.  Runs only where oracle/_ref exists; the output is committed.

  python tests/golden/make_oracle_vs_ref.py
"""
import json, os, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE))
import common, oracle_py, cli_inputs
import test_oracle_vs_ref as t
import test_evaluate as te

assert t.LIVE and te.LIVE_SCORERS, "oracle/_ref is not built"
work = tempfile.mkdtemp()
out = {"runs": {}, "index_sha256": {}, "scorers": {}}


def record(label, d, prefix, flags):
    out["runs"][t.run_key(label, flags)] = t.recorded(*t.run_ref(d, prefix, flags))


c, d = cli_inputs.make(work)
for flags, label in cli_inputs.VARIANTS:
    record(label, d, c["prefix"], flags)
for name, make, runs in (("fuzz", t.fuzz_inputs, [["-f", "a.fq", "-f2", "b.fq"] + f for f in t.FUZZ_FLAGS]), ("fuzz_odd", t.odd_inputs, t.ODD_FLAGS)):
    d = make(work)
    subprocess.run([oracle_py.REF_INDEXER, "g.fa", "g"], cwd=d, stdout=subprocess.DEVNULL, check=True)
    out["index_sha256"][name] = {ext: common.sha(os.path.join(d, "g." + ext)) for ext in t.INDEX_EXT}
    for flags in runs:
        record(name, d, os.path.join(d, "g"), flags)
out["scorers"] = te.ref_eva_and_sj(work)
out["scorers"]["flux_eva"] = {str(s): te.ref_flux_eva(work, s) for s in te.FLUX_SEEDS}
json.dump(out, open(os.path.join(HERE, "oracle_vs_ref.json"), "w"), indent=1, sort_keys=True)
print(json.dumps(out["scorers"], indent=1))
