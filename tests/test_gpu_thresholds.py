"""GPU suite (-m gpu): the ladders of tests/threshold_inputs.py -- reads that stand one base either side of each of the mapping path's comparisons -- through the HIP path,
every record against the oracle: under every flag set, paired and with every mate as its own read, through the ASCII, the packed and both compact entry points; the whole set
in one batch and every ladder as a small batch of its own (its units then meet other neighbours in a workgroup); the reference-equivalent counters, which say on which side
of `rGaps > 20` and `PosDiff > MaxGaps` ladder D's rungs fell; the counters that name the form that ran; and one run of `dart` against the oracle's command line and the
reference's recorded SAM.  tests/test_thresholds_oracle.py shows that every ladder flips in the reference's own results exactly where it says."""
import os, subprocess
import pytest
import common, oracle_py
import threshold_inputs as ti
import test_thresholds_oracle as tt
from dart_amd import host

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
# the GPU's counter -> the oracle's (as tests/test_gpu_low_complexity.py)
COUNTERS = (("steps", "n_2occ4"), ("lf_steps", "n_lf"), ("sa_lookups", "n_sa"), ("nw_calls", "n_nw"), ("nw_cells", "nw_cells"),
            ("reseed_calls", "n_reseed"), ("reseed_window", "reseed_window"))
LADDER_NAMES = [n for n in ("A_clean_t5", "A_sub_t5", "A_clean_t10", "A_sub_t10", "A_clean_t31", "A_sub_t31", "B_read_t100000", "B_mates_t100000", "B_read_t500000",
                            "B_mates_t500000", "B_chrend", "B_chrend_rev", "C_fast_m0", "C_report_m0", "C_fast_m1", "C_report_m1", "C_fast_m2", "C_report_m2", "C_fast_m5",
                            "C_report_m5", "C_fast_m12", "C_report_m12", "D_rgap", "D_jump", "E_reach", "E_ahead", "F_cov_r50", "F_cov_r100", "F_cov_r101", "F_cov_r150",
                            "F_cov_r250", "G_cut", "G_cut_single", "H_gap_r10", "H_gap_r15", "H_gap_r20", "H_gap_r25", "H_gapmis_r20", "I_reseed", "K_product",
                            "B_read_heavy", "D_jump_heavy", "F_cov_heavy", "E_reach_heavy", "E_ahead_heavy")]
# ladders whose event reads hold a junction, a read gap or an indel: their units cannot be finished by k_pair's own reports (dg_pair.h: d_unit_reports)
GENERAL_PATH = ("A_clean_", "B_read_", "C_report_", "D_", "H_", "I_reseed")


@pytest.fixture(scope="module")
def ctx(workdir):
    """the index of the 2.25 Mb genome, built once (and the reference indexer's bytes), one context and the oracle on it"""
    prefix = tt.build_index(workdir)
    for ext, want in tt.gold()["index_sha256"].items():
        assert common.sha(prefix + "." + ext) == want, ext
    ix = host.Index(prefix)
    gpu, orc = host.DartGPU(ix), oracle_py.Oracle(prefix)
    yield dict(prefix=prefix, ix=ix, gpu=gpu, orc=orc)
    gpu.close(); orc.close()


def _map_and_compare(ctx, rungs, flags, paired, every_entry_point):
    """-> (the oracle's records, the GPU's counters, the oracle's counters)"""
    gpu, orc = ctx["gpu"], ctx["orc"]
    p, _ = common.parse_flags(flags)
    reads = ti.stored(rungs)
    so, rl, flat = host.pack_reads(reads)
    want = orc.map_batch(orc.params(paired=paired, **p), so, rl, flat, threads=8)
    oc = dict(orc.counters)
    gpu.set_params(host.default_params(paired=paired, **p))
    common.assert_same(gpu.map_batch(so, rl, flat), want)
    c = gpu.counters()
    for mine, theirs in COUNTERS:
        assert c[mine] == oc[theirs], (mine, c[mine], oc[theirs])
    words, nlist, longest, lens = ti.padded_2bit(reads)
    common.assert_same(gpu.map_batch_packed(words, nlist, longest, lens), want)
    if every_entry_point:
        common.assert_same(gpu.download_compact(), want)
        common.assert_same(gpu.map_batch_compact(words, nlist, longest, lens), want)
    return want, c, oc


def test_ladder_names_are_all_of_them():
    assert LADDER_NAMES == list(ti.ladders())


@pytest.mark.parametrize("run", list(ti.RUNS))
def test_gpu_whole_set_matches_oracle(run, ctx):
    """all ladders in one batch under one flag set, paired and single: the oracle's records, which are the reference's (rows of tests/golden/thresholds.json)"""
    g = tt.gold()
    for mode, paired in (("pe", 1), ("se", 0)):
        try:
            want, c, oc = _map_and_compare(ctx, ti.all_rungs(), ti.RUNS[run], paired, True)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (tt.run_key(mode, run), str(e)[:800]))
        rows = [[x[f] for f in tt.FIELDS] for x in tt.summaries(*want)]
        assert tt.rows_digest(rows) == g["runs"][tt.run_key(mode, run)]["rows_sha256"]
        print("COUNTERS %-46s %s" % (tt.run_key(mode, run), " ".join("%s=%d" % (k, c[k]) for k in ("general_path_units", "wave_chained_units", "nw_calls", "reseed_calls", "reruns_capacity_total"))))


@pytest.mark.parametrize("name", LADDER_NAMES)
def test_gpu_ladder_alone_matches_oracle(name, ctx):
    """one ladder's 40 to 48 pairs as a batch of their own, under the flag set that judges it and under -mis 30, paired and single: the ASCII and the packed entry point
    in both modes, the two compact ones when paired (test_gpu_whole_set_matches_oracle runs all four in both modes).  Ladder H reaches two of dg_report.h's three forms of
    the gap rule: read gaps of 10, 15 and 20 bases d_gap_small (:1206), the gap of 25 bases d_gap_split_tb (:1141); d_gap_split_strings (:1081) takes wide gaps that hold
    a literal '-', which no ladder has (the packed entry points take A, C, G, T and N only; tests/golden/odd_characters.* cover that form)"""
    l = ti.ladders()[name]
    for run in dict.fromkeys((l["run"], "m30")):
        for paired in (1, 0):
            try:
                want, c, oc = _map_and_compare(ctx, l["rungs"], ti.RUNS[run], paired, paired == 1)
            except AssertionError as e:
                raise AssertionError("%s %s paired=%d: %s" % (name, run, paired, str(e)[:800]))
            print("COUNTERS %-18s %-5s paired=%d %s" % (name, run, paired, " ".join("%s=%d" % (k, c[k]) for k in ("general_path_units", "wave_chained_units", "nw_calls", "reseed_calls"))))
            if run != l["run"]: continue
            n_units = len(l["rungs"]) * (1 if paired else 2)
            if name.startswith(GENERAL_PATH):
                assert c["general_path_units"] > 0, "no unit of %s reached the report path" % name
            if name.startswith("C_fast_"):  # isolated substitutions on one diagonal: k_pair writes these units' reports itself, `mis > max_mismatch` of dg_pair.h included
                assert c["general_path_units"] == 0, "%d of %d units of %s left k_pair for the report path" % (c["general_path_units"], n_units, name)
            if name.endswith("_heavy") and paired:      # the plain mate's 17 seeds: every unit is k_chain_heavy's (d_gen_candidates_wave and the staged pairing, dg_chain.h:217, :239-240, :398)
                assert c["wave_chained_units"] == n_units, "%d of %d units of %s went through k_chain_heavy" % (c["wave_chained_units"], n_units, name)
            if name.startswith("D_"):       # the rungs above the threshold are searched once more, the others are not: 2 of the 5 rungs of every site, one read gap each
                assert c["reseed_calls"] == oc["n_reseed"] == 2 * ti.N_SITES
            if name == "K_product" and paired:
                assert c["wave_chained_units"] > 0, "no unit of K_product went through k_chain_heavy"


def test_gpu_read_gap_ladders_reseed_rung_by_rung(ctx):
    """ladder D rung by rung, each pair a batch of its own: the library searches the read gap once more exactly where the oracle does (`PosDiff > MaxGaps && rGaps > 20`)"""
    gpu, orc = ctx["gpu"], ctx["orc"]
    for name in ("D_rgap", "D_jump", "D_jump_heavy"):
        l = ti.ladders()[name]
        p, _ = common.parse_flags(ti.RUNS[l["run"]])
        gpu.set_params(host.default_params(paired=1, **p))
        for r in l["rungs"]:
            if r["site"] > 1: continue          # (two sites, one per strand: 10 small batches per ladder)
            so, rl, flat = ti.batch([r])
            want = orc.map_batch(orc.params(paired=1, **p), so, rl, flat, threads=1)
            common.assert_same(gpu.map_batch(so, rl, flat), want)
            assert (gpu.counters()["reseed_calls"] > 0) == (orc.counters["n_reseed"] > 0) == (r["value"] >= l["flip"][1]), (name, r["site"], r["value"])


def test_dart_cli_on_the_ladders_matches_oracle_cli_and_reference(ctx, workdir):
    """`dart -mis 5 -min_intron 10 -max_intron 50000` (the parser lifts 50 000 to 100 000, so ladder B's rungs around 100 000 stand on the limit): byte for byte the oracle
    command line's SAM and junctions, which are the ones the reference's object code wrote"""
    oracle_py.build()
    g = tt.gold()["runs"][tt.run_key("pe", "i10")]
    d = os.path.join(workdir, "thresholds_gpu_cli"); os.makedirs(d, exist_ok=True)
    ti.write_fastq(os.path.join(d, "a.fq"), os.path.join(d, "b.fq"), ti.all_rungs())
    files = ["-f", "a.fq", "-f2", "b.fq"] + ti.CLI_FLAGS
    rg = subprocess.run([DART, "-i", ctx["prefix"]] + files + ["-o", "gpu.sam", "-j", "gpu.j", "-t", "4"], cwd=d, stdout=subprocess.PIPE, check=True, env=dict(os.environ, DART_BATCH="1000"))
    ro = subprocess.run([oracle_py.ORACLE_CLI, "-i", ctx["prefix"]] + files + ["-o", "orc.sam", "-j", "orc.j"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    a, b = open(os.path.join(d, "orc.sam")).read(), open(os.path.join(d, "gpu.sam")).read()
    assert a == b, common.first_diff(b, a)
    assert open(os.path.join(d, "orc.j")).read() == open(os.path.join(d, "gpu.j")).read()
    assert common.stats_block(rg.stdout) == common.stats_block(ro.stdout) == g["stats"] != ""
    assert common.sha(os.path.join(d, "gpu.sam")) == g["sam_sha256"] and common.sha(os.path.join(d, "gpu.j")) == g["junctions_sha256"]
