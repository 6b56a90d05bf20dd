"""CPU suite: the ladders of tests/threshold_inputs.py through the oracle (never the GPU) against what the REFERENCE's object code wrote for them
(tests/golden/thresholds.json, made by tests/golden/make_thresholds.py): every run's records, and per ladder the flip -- the outcome named in the
ladder changes between the two neighbouring rungs the ladder names, at every site, and between no other two.  That is what keeps an identical GPU
result on these reads from being vacuous: the reads do stand on the comparison.  The committed stage dump of one run replays through the chain stage's
host-compiled code (both forms: the in-memory one and k_pair's per-lane one)."""
import gzip, hashlib, json, os, shutil, subprocess
import numpy as np
import pytest
import common, oracle_py
import threshold_inputs as ti
from dart_amd import index_build

GOLD = os.path.join(common.GOLDEN, "thresholds.json")
DUMP = os.path.join(common.GOLDEN, "thresholds.%s_%s.stages.gz" % ti.DUMP_RUN)
OPS = "MIDNSHP=X"
FIELDS = ("cigar", "chr", "pos", "bdir", "score", "sub_score", "mapq", "paired_idx", "sj_type", "n_rep", "n_hit")


def gold():
    return json.load(open(GOLD))


def run_key(mode, run):
    return "%s: %s" % (mode, " ".join(ti.RUNS[run]))


def build_index(workdir):
    prefix = os.path.join(workdir, "thresholds")
    if not os.path.exists(prefix + ".sa"):
        index_build.build_index_from_genome(ti.make_genome(), prefix, device="cpu")
    return prefix


def summaries(reads, rep, cig, sj):
    """per read: what the reference's stage dump says of it (its R lines: tests/golden/make_thresholds.py) -- the best report's CIGAR, place, mate and junction type, the
    read's scores, the number of its reports and of those with a positive score.  (The junction type of an unmapped read's only report is a field the reference never
    writes: -1 here)"""
    out = []
    for r in reads:
        lo, n = int(r["rep_off"]), int(r["n_rep"])
        b = rep[lo + max(int(r["best"]), 0)]
        mapped = int(r["score"]) > 0
        ops = cig[int(b["cigar_off"]):int(b["cigar_off"]) + int(b["n_cigar"])] if mapped else []
        out.append(dict(cigar="".join("%d%s" % (int(x) >> 4, OPS[int(x) & 15]) for x in ops) if mapped else "*", chr=int(b["chr"]) if mapped else -1, pos=int(b["pos"]) if mapped else 0,
                        bdir=int(b["bdir"]) if mapped else 0, score=int(r["score"]), sub_score=int(r["sub_score"]), mapq=int(r["mapq"]), paired_idx=int(b["paired_idx"]),
                        sj_type=int(b["sj_type"]) if mapped else -1, n_rep=n, n_hit=int((rep["aln_score"][lo:lo + n] > 0).sum())))
    return out


# (the reference prints the FLAG of a report it never set as the heap left it: tests/read_structure_inputs.py)
REF_ENV = dict(os.environ, MALLOC_PERTURB_="255")


def rows_of_dump(lines):
    """the R lines of a stage dump of the reference harness -> per read its row in FIELDS' order"""
    out = []
    for line in lines:
        f = line.split()
        if not f or f[0] not in ("R1", "R2"): continue
        kv = dict(x.split("=") for x in f[2:7])
        reps = [x.strip("[]").split(",") for x in f[7:]]
        b = reps[max(int(kv["best"]), 0)]
        mapped = int(kv["score"]) > 0
        out.append([b[6] if mapped else "*", int(b[3]) if mapped else -1, int(b[4]) if mapped else 0, int(b[5]) if mapped else 0, int(kv["score"]), int(kv["sub"]), int(kv["mapq"]),
                    int(b[2]), int(b[1]) if mapped else -1, int(kv["can"]), sum(1 for x in reps if int(x[0]) > 0)])
    return out


def rows_digest(rows):
    return hashlib.sha256(json.dumps(rows, separators=(",", ":")).encode()).hexdigest()


def outcome(key, s):
    """the outcome a ladder is judged by, from a rung's summary"""
    ops = "".join(c for c in s["cigar"] if not c.isdigit())
    if key == "mapped": return s["score"] > 0
    if key == "spliced": return "N" in ops
    if key == "proper": return s["paired_idx"] >= 0
    if key == "n_hit": return s["n_hit"]
    if key == "filled": return "N" in ops and "I" not in ops          # (the read gap's bases came out aligned, not inserted)
    if key == "reseeded":             # (ladder I_reseed: the 33 gap bases the second search found are aligned with the left seed's 40, the rest of the gap is inserted)
        import re
        return re.findall(r"(\d+)M", s["cigar"]) == ["73", "50"] and "D" not in ops
    if key in ("shape", "n_reseed"): return ops
    raise KeyError(key)


def map_run(orc, mode, run, rungs=None):
    p, _ = common.parse_flags(ti.RUNS[run])
    so, rl, flat = ti.batch(ti.all_rungs() if rungs is None else rungs)
    return orc.map_batch(orc.params(paired=1 if mode == "pe" else 0, **p), so, rl, flat, threads=8)


def rung_table(per_run):
    """{ladder: {site: [(value, summary of the event read)]}} from {(mode, run): summaries of all reads}"""
    idx = ti.rung_index()
    out = {}
    for name, l in ti.ladders().items():
        s = per_run[l["mode"], l["run"]]
        for r in l["rungs"]:
            i = idx[name, r["site"], r["value"]]
            out.setdefault(name, {}).setdefault(r["site"], []).append((r["value"], s[2 * i + r["event_mate"]]))
    return out


def check_flips(table, names=None):
    """every ladder flips between the two values it names, at every site, and nowhere else; a control never flips.  -> {ladder: sites}"""
    seen = {}
    for name, l in ti.ladders().items():
        if names is not None and name not in names: continue
        assert len(table[name]) >= ti.N_SITES, name
        for site, rungs in sorted(table[name].items()):
            vals = [v for v, _ in rungs]
            assert all(0 <= b - a <= 1 for a, b in zip(vals, vals[1:])), (name, site, vals)          # no value skipped (K_product: two shapes of one product)
            if l["flip"] == "unjudged" or l["key"] == "n_reseed": continue      # (n_reseed: test_read_gap_ladders_reseed_where_they_say)
            got = [outcome(l["key"], s) for _, s in rungs]
            changes = sorted({(vals[i], vals[i + 1]) for i in range(len(vals) - 1) if got[i] != got[i + 1]})
            want = [] if l["flip"] is None else [tuple(l["flip"])]
            assert changes == want, "ladder %s site %d: outcome %s over values %s changes at %s, expected at %s" % (name, site, got, vals, changes, want)
        seen[name] = len(table[name])
    return seen


@pytest.fixture(scope="module")
def orc(workdir):
    o = oracle_py.Oracle(build_index(workdir))
    yield o
    o.close()


@pytest.fixture(scope="module")
def mapped(orc):
    """{(mode, run): the oracle's records of all rungs}"""
    return {(mode, run): map_run(orc, mode, run) for mode in ("pe", "se") for run in ti.RUNS}


def test_inputs_are_the_fixtures_and_stand_in_unique_text():
    g = gold()
    lad = ti.ladders()
    assert ti.codes_sha256() == g["codes_sha256"] and ti.reads_sha256() == g["reads_sha256"], "the generator drifted from the golden inputs"
    T = ti.text()
    assert len(ti.PIECES) > 1000
    for ladder, k, x, y, count in ti.PIECES:
        assert (ti.count16(T[x:y]) == count).all(), (ladder, k, x, y)
    n = len(ti.all_rungs())
    print("ladders %d, pairs %d" % (len(lad), n))
    assert 2 * n <= 6000
    for name, l in lad.items():
        assert len({r["site"] for r in l["rungs"]}) >= ti.N_SITES, name
        assert {r["event_mate"] for r in l["rungs"]} == {0, 1}, name


def _rows(res):
    return [[x[f] for f in FIELDS] for x in summaries(*res)]


def test_oracle_records_equal_the_reference_fixture(mapped):
    """every read of every run: the oracle's rows against the digest of the reference's; the judged rungs row by row"""
    g = gold()
    for (mode, run), res in sorted(mapped.items()):
        key = run_key(mode, run)
        rows = _rows(res)
        table = rung_table({(m, r): [dict(zip(FIELDS, row)) for row in rows] for m in ("pe", "se") for r in ti.RUNS})
        for name, l in ti.ladders().items():
            if (l["mode"], l["run"]) != (mode, run): continue
            for site, rr in table[name].items():
                got = [[v] + [s[f] for f in FIELDS] for v, s in rr]
                assert got == g["rungs"][name][str(site)], (key, name, site, got, g["rungs"][name][str(site)])
        assert rows_digest(rows) == g["runs"][key]["rows_sha256"], key


def _gold_table():
    g = gold()
    return {name: {int(site): [(row[0], dict(zip(FIELDS, row[1:]))) for row in rr] for site, rr in sites.items()} for name, sites in g["rungs"].items()}


def test_every_ladder_flips_where_it_says_in_the_reference_results():
    """judged by the fixture alone: what the reference's object code wrote"""
    table = _gold_table()
    seen = check_flips(table)
    print(seen)
    assert set(seen) == set(ti.ladders())
    for letter in "ABCDEFGHIJK":
        assert any(n.startswith(letter + "_") for n in seen) or letter in ti.LADDERS_DROPPED, letter
    assert len(ti.LADDERS_DROPPED) <= 2
    # deleting one flip from the fixture is noticed: a rung's row copied over its neighbour's across the threshold
    for name in ("A_clean_t10", "B_read_t100000", "B_read_heavy", "E_reach", "I_reseed", "K_product"):
        l = ti.ladders()[name]
        rr = table[name][3]
        at = [i for i, (v, _) in enumerate(rr) if v == l["flip"][1]]
        below = [s for v, s in rr if v == l["flip"][0]][-1]
        saved = [rr[i] for i in at]
        for i in at: rr[i] = (rr[i][0], below)
        with pytest.raises(AssertionError):
            check_flips(table, names=[name])
        for i, x in zip(at, saved): rr[i] = x
    check_flips(table)


def test_oracle_command_line_writes_the_reference_sam_of_every_run(workdir):
    """all 16 runs (8 flag sets, paired and with every mate as its own read) through the oracle's command line: the statistics block, the SAM (every report of every read,
    FLAG, NM, MAPQ) and the junction table byte for byte what the reference's object code wrote; the paired -max_intron 100000 run once more as `dart` is given it on the
    GPU (tests/test_gpu_thresholds.py): -max_intron 50000, which the parser lifts to 100 000"""
    oracle_py.build()
    prefix = build_index(workdir)
    g = gold()
    for ext, want in g["index_sha256"].items():
        assert common.sha(prefix + "." + ext) == want, "index file .%s differs from the reference indexer's" % ext
    d = os.path.join(workdir, "thresholds_cli"); os.makedirs(d, exist_ok=True)
    ti.write_fastq(os.path.join(d, "a.fq"), os.path.join(d, "b.fq"), ti.all_rungs())
    ti.write_single_fastq(os.path.join(d, "s.fq"), ti.all_rungs())
    runs = [(mode, run, ti.RUNS[run]) for mode in ("pe", "se") for run in ti.RUNS] + [("pe", "i10", ti.CLI_FLAGS)]
    for mode, run, flags in runs:
        files = ["-f", "a.fq", "-f2", "b.fq"] if mode == "pe" else ["-f", "s.fq"]
        r = subprocess.run([oracle_py.ORACLE_CLI, "-i", prefix] + files + flags + ["-o", "orc.sam", "-j", "orc.j", "-t", "4"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        want = g["runs"][run_key(mode, run)]
        assert common.stats_block(r.stdout) == want["stats"] != "", (mode, flags)
        assert common.sha(os.path.join(d, "orc.sam")) == want["sam_sha256"], "the oracle's SAM differs from the reference's (%s %s)" % (mode, " ".join(flags))
        assert common.sha(os.path.join(d, "orc.j")) == want["junctions_sha256"], "the oracle's junctions differ from the reference's (%s %s)" % (mode, " ".join(flags))


def test_every_ladder_flips_in_the_oracle(mapped):
    check_flips(rung_table({k: summaries(*v) for k, v in mapped.items()}))


def test_read_gap_ladders_reseed_where_they_say(orc):
    """ladder D stands on `PosDiff > MaxGaps && rGaps > 20` (AlignmentCandidates.cpp:693), which decides whether the read gap is searched once more.  The search finds nothing
    in these gaps (a gap of 21 .. 24 bases holds no stretch it would accept that is not a seed already), so the records do not say on which side a rung fell; the count of
    such searches does (the oracle's n_reseed, which the GPU tests hold the library's reseed_calls against): every rung mapped alone"""
    for name, l in ti.ladders().items():
        if l["key"] != "n_reseed": continue
        for site in range(ti.N_SITES):
            rr = sorted((r["value"], r) for r in l["rungs"] if r["site"] == site)
            got = []
            for v, r in rr:
                map_run(orc, "pe", l["run"], [r])
                got.append(orc.counters["n_reseed"] > 0)
            assert got == [v >= l["flip"][1] for v, _ in rr], (name, site, got)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_stage_dump_of_the_ladders_replays_through_the_chain_code(workdir):
    """the seeds the reference's object code found for the ladders (its S1/S2 lines, run DUMP_RUN: -max_intron 100000, so ladder B's rungs stand on
    `PosDiff < MaxIntronSize`) -> the candidates of its C1/C2 lines, through d_cluster_seeds and the list rules as k_pair's lane code and as the in-memory route call
    them (dg_chain.h:52-70, :100-123).  The wave forms of k_chain_heavy (:217, :239-240, :398) are device code: tests/test_gpu_thresholds.py, the *_heavy ladders"""
    import test_kernel_arith_host as tk
    exe = os.path.join(workdir, "chain_checks_thresholds")
    subprocess.run(["hipcc", "-O2", "--offload-arch=gfx950", "-std=c++17", "-w", "-o", exe, os.path.join(common.ROOT, "tests", "native", "chain_checks.hip")], check=True)
    reads = ti.stored(ti.all_rungs())
    p, _ = common.parse_flags(ti.RUNS[ti.DUMP_RUN[1]])
    n = tk._chain_check(exe, "thresholds", ti.GENOME_LENGTHS, p, 1, DUMP, lambda k: len(reads[k]))
    assert n == len(reads)
