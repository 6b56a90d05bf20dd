"""Regenerates tests/golden/read_structures.json and read_structures.mis12m.{sam.gz,junctions.tab,stages.gz}: what the REFERENCE's object code (oracle/_ref/ref_harness, built by
`make -C oracle ref`) writes for the read sets of tests/read_structures.py (tests/read_structure_inputs.py: SEED, N_PER_CLASS) -- the 101-base set over the pe101_spliced case's
genome, paired, at -mis 5, -mis 12 -m and -mis 30; the 250-base set over the pe151_spliced case's genome at -mis 30 and at -mis 100 (under which its insertions of 31-80 bases map).  Per run the statistics block and the SHA-256 of the SAM and
junction files; of the -mis 12 -m run of the 101-base set also the files themselves and the stage dump.  Runs only where the reference's object code exists; the outputs are committed.

  python tests/golden/make_read_structures.py
"""
import gzip, hashlib, json, os, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE))
import common, read_structures as rs, read_structure_inputs as rsi

REF = os.path.join(ROOT, "oracle", "_ref")
work = tempfile.mkdtemp()
meta = {"seed": rsi.SEED, "n_per_class": rsi.N_PER_CLASS, "sets": {}, "runs": {}}
for name, (case, rlen) in rsi.SETS.items():
    c, classes, _ = rsi.read_set(name, work)
    d = os.path.join(work, name); os.makedirs(d)
    c["genome"].write_fasta(os.path.join(d, "g.fa"))
    subprocess.check_call([os.path.join(REF, "bwt_index"), "g.fa", "g"], cwd=d, stdout=subprocess.DEVNULL)
    pairs, _ = rs.all_pairs(classes)
    rs.write_fastq(os.path.join(d, "a.fq"), os.path.join(d, "b.fq"), pairs)
    meta["sets"][name] = {"case": case, "rlen": rlen, "pairs": len(pairs), "classes": {k: len(v) for k, v in classes.items()}, "reads_sha256": rs.digest(classes)}
    for flags in rsi.REF_FLAGS[name]:
        keep = name == "rs101" and list(flags) == rsi.FIXTURE_FLAGS
        out = subprocess.run([os.path.join(REF, "ref_harness"), "map", "-i", "g", "-f", "a.fq", "-f2", "b.fq"] + list(flags) + ["-o", "ref.sam", "-j", "ref.j"] + (["-dump", "ref.dump"] if keep else []),
                             cwd=d, stdout=subprocess.PIPE, check=True, env=rsi.REF_ENV).stdout
        sam = open(os.path.join(d, "ref.sam"), "rb").read(); junc = open(os.path.join(d, "ref.j"), "rb").read()
        meta["runs"][rsi.run_key(name, flags)] = {"stats": common.stats_block(out), "sam_sha256": hashlib.sha256(sam).hexdigest(), "junctions_sha256": hashlib.sha256(junc).hexdigest()}
        if keep:
            with gzip.GzipFile(rsi.BASE + ".sam.gz", "wb", mtime=0) as f: f.write(sam)
            open(rsi.BASE + ".junctions.tab", "wb").write(junc)
            with gzip.GzipFile(rsi.BASE + ".stages.gz", "wb", mtime=0) as f: f.write(open(os.path.join(d, "ref.dump"), "rb").read())
json.dump(meta, open(rsi.GOLD, "w"), indent=1, sort_keys=True)
print(json.dumps(meta["runs"], indent=1))
for ext in (".sam.gz", ".junctions.tab", ".stages.gz"):
    print(ext, os.path.getsize(rsi.BASE + ext))
