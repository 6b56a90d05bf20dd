"""Regenerates tests/golden/thresholds.json and thresholds.pe_i10.stages.gz: what the REFERENCE's object code (oracle/_ref/ref_harness and bwt_index, built by
`make -C oracle ref` where the reference tree exists) writes for the ladders of tests/threshold_inputs.py -- the digests of the genome's codes, of the reads and of its
indexer's five files; per run (paired and with every mate as its own read, under every flag set of threshold_inputs.RUNS) the statistics block, the SHA-256 of its SAM and
junction files and of the rows below over all reads; per ladder, from the run that judges it, every rung's row: what the stage dump's R line says of the event read (best
report's CIGAR, chromosome, position, strand, the read's score, sub-score and MAPQ, the best report's mate index and junction type, the number of reports and of those with
a positive score); the SAM lines of the clean 3- and 4-base deletions of A_clean_t5's first site; and the stage dump of one run.  Data only.  It asserts that every ladder
flips where it says (test_thresholds_oracle.check_flips).  Runs only where oracle/_ref exists.

  python tests/golden/make_thresholds.py
"""
import gzip, hashlib, json, os, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE))
import common, oracle_py
import threshold_inputs as ti
import test_thresholds_oracle as tt

assert os.path.exists(oracle_py.REF_HARNESS) and os.path.exists(oracle_py.REF_INDEXER), "oracle/_ref is not built"
d = tempfile.mkdtemp()
rungs = ti.all_rungs()
ti.make_genome().write_fasta(os.path.join(d, "g.fa"))
subprocess.run([oracle_py.REF_INDEXER, "g.fa", "g"], cwd=d, stdout=subprocess.DEVNULL, check=True)
ti.write_fastq(os.path.join(d, "a.fq"), os.path.join(d, "b.fq"), rungs)
ti.write_single_fastq(os.path.join(d, "s.fq"), rungs)
out = {"codes_sha256": ti.codes_sha256(), "reads_sha256": ti.reads_sha256(), "pairs": len(rungs),
       "index_sha256": {ext: common.sha(os.path.join(d, "g." + ext)) for ext in ("amb", "ann", "bwt", "pac", "sa")}, "runs": {}, "rungs": {}}
per_run = {}
for mode, files in (("pe", ["-f", "a.fq", "-f2", "b.fq"]), ("se", ["-f", "s.fq"])):
    for run, flags in ti.RUNS.items():
        key = tt.run_key(mode, run)
        r = subprocess.run([oracle_py.REF_HARNESS, "map", "-i", "g"] + files + flags + ["-o", "ref.sam", "-j", "ref.j", "-dump", "ref.dump"], cwd=d, stdout=subprocess.PIPE, check=True, env=tt.REF_ENV)
        sam = open(os.path.join(d, "ref.sam"), "rb").read(); junc = open(os.path.join(d, "ref.j"), "rb").read()
        rows = tt.rows_of_dump(open(os.path.join(d, "ref.dump")))
        assert len(rows) == 2 * len(rungs), (key, len(rows))
        per_run[mode, run] = [dict(zip(tt.FIELDS, row)) for row in rows]
        out["runs"][key] = {"stats": common.stats_block(r.stdout), "sam_sha256": hashlib.sha256(sam).hexdigest(), "junctions_sha256": hashlib.sha256(junc).hexdigest(),
                            "rows_sha256": tt.rows_digest(rows)}
        print("%-50s SAM lines %6d  junction lines %4d" % (key, sam.count(b"\n"), junc.count(b"\n")))
        if (mode, run) == ti.DUMP_RUN:
            with gzip.GzipFile(tt.DUMP, "wb", mtime=0) as f: f.write(open(os.path.join(d, "ref.dump"), "rb").read())
        if (mode, run) == ("pe", "d"):
            idx = ti.rung_index()
            lines = [l for l in sam.decode().split("\n") if l and not l.startswith("@")]
            out["clean_deletion_first_records"] = {}
            for L in (3, 4):
                i = idx["A_clean_t5", 0, L]
                out["clean_deletion_first_records"]["L=%d" % L] = [l for l in lines if l.split("\t")[0] == "t%d" % i]
table = tt.rung_table(per_run)
for name, sites in table.items():
    out["rungs"][name] = {str(site): [[v] + [s[f] for f in tt.FIELDS] for v, s in rr] for site, rr in sites.items()}
print(tt.check_flips(table))
json.dump(out, open(tt.GOLD, "w"), indent=None, separators=(",", ":"), sort_keys=True)
print(json.dumps(out["clean_deletion_first_records"], indent=1))
print(os.path.getsize(tt.GOLD), os.path.getsize(tt.DUMP))
