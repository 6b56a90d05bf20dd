"""Device and wall time of the QC tables (dg_bam_qc_finish: the per-record tables, lane = record, and the per-cycle pass, a quarter wave = record) beside the duplicate
marking's record pass (k_md_rec, lane = record over the same bytes: the yardstick), the allele counts' counting walk and the BGZF kernels, all over the same
sorted array in the same run: 1 M pairs of 2x101 on the chr20-sized planted genome at -mis 5, the reads and batches of bam_sort_rate.py.  A tool, not a test.
Device time from events; prints median, min and max of --runs runs behind --warmup.

    python profiles/probes/qc_rate.py [--runs 10] [--warmup 2] [--pairs 1000000] [--batches 4] [--cache DIR] [--out profiles/qc/qc_rate.json]
    python profiles/probes/qc_rate.py --resources profiles/qc/resource_usage.txt      (cross-compiles dg_qc.h; needs no device)
"""
import argparse, json, os, re, statistics, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BLOCK = 0xFF00
STAGES = ("record_tables", "cycle_pass")


def resource_table(path):
    """registers, scratch, occupancy and LDS of every kernel of dg_qc.h, as the compiler reports them for gfx950"""
    import __graft_entry__ as ge
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "qc.hip")
        open(src, "w").write('#include "%s"\n' % os.path.join(ROOT, "dart_amd", "csrc", "dg_qc.h"))
        r = subprocess.run([ge.HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-c", "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", src,
                            "-o", os.path.join(d, "qc.o")], capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            m = re.match(r"_Z(\d+)", v)                       # _Z<length><name><parameters>
            name = v[len(m.group(0)):len(m.group(0)) + int(m.group(1))] if m else v
            cur = dict(name=name) if name.startswith("k_qc_") else None      # (the header includes the allele counts', the coverage track's, the sorter's and the formatter's kernels)
            if cur is not None:
                rows.append(cur)
        elif cur is not None:
            cur[k] = v
    cols = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch/B"), ("SGPRs Spill", "SGPRsp"), ("VGPRs Spill", "VGPRsp"),
            ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "LDS/B"), ("Dynamic Stack", "dyn.stack"))
    out = ["# hipcc -O3 --offload-arch=gfx950 -std=c++17 -Rpass-analysis=kernel-resource-usage over dart_amd/csrc/dg_qc.h (cross-compiled; no device needed)",
           "%-18s" % "kernel" + "".join("%10s" % c for _, c in cols)]
    out += ["%-18s" % r_["name"] + "".join("%10s" % r_.get(k, "?") for k, _ in cols) for r_ in rows]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(out) + "\n")
    assert len(rows) == 2 and all(r_.get("ScratchSize [bytes/lane]") == "0" and r_.get("VGPRs Spill") == "0" and r_.get("SGPRs Spill") == "0" for r_ in rows), "a kernel of dg_qc.h uses scratch or spills"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1000000); ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "dart_bench_cache")); ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    if a.resources:
        resource_table(a.resources)
        return
    import bench
    from dart_amd import host, synth
    prefix, g = bench.prepare_index(a.cache, bench.CHR20_LEN, 0, lambda: None)
    m1, m2 = synth.make_reads(g, a.pairs, rlen=101, seed=1000, sub_rate=0.01, indel_frac=0.02, n_frac=0.002)
    reads = host.interleave_pairs(m1, m2)
    n = 2 * a.pairs
    gpu = host.DartGPU(host.Index(prefix), host.default_params(paired=1, max_mismatch=5))
    ids = [("r%09d" % (i // 2)).encode() for i in range(n)]
    quals = [b"I" * 101] * n
    cuts = [(n * k // a.batches) & ~1 for k in range(a.batches)] + [n]
    for k in range(a.batches):
        lo, hi = cuts[k], cuts[k + 1]
        so, rl, flat = host.pack_reads(reads[lo:hi])
        gpu.map_batch(so, rl, flat)
        gpu.format_bam(ids[lo:hi], quals[lo:hi], hi - lo, raw=True)
        gpu.accumulate_bam(k)
    t = {k: [] for k in ("sort_finish_device_ms", "bgzf_device_ms", "markdup_record_pass_ms", "pileup_count_ms", "qc_device_ms", "qc_wall_ms") + tuple("qc_%s_ms" % s for s in STAGES)}
    for r in range(a.warmup + a.runs):
        n_rec, nb = gpu.bam_sort_finish()
        z_ms = 0.0
        for off in range(0, nb, 4096 * BLOCK):
            gpu.bam_sort_compress(off, min(4096 * BLOCK, nb - off))
            z_ms += gpu.bam_device_ms
        gpu.bam_markdup_finish(count_only=True)               # (decides and counts, writes no flag: the array stays as it is)
        md_rec = gpu.bam_markdup_device_ms_split[0]
        gpu.bam_pileup_finish(entries_only=True)
        pu_count = gpu.bam_pileup_device_ms_split[0]
        w0 = time.perf_counter()
        v = gpu.bam_qc_finish()                               # (the wall time holds the download too)
        w1 = time.perf_counter()
        if r >= a.warmup:
            t["sort_finish_device_ms"].append(gpu.bam_sort_device_ms); t["bgzf_device_ms"].append(z_ms); t["markdup_record_pass_ms"].append(md_rec); t["pileup_count_ms"].append(pu_count)
            t["qc_device_ms"].append(gpu.bam_qc_device_ms); t["qc_wall_ms"].append((w1 - w0) * 1e3)
            for s, x in zip(STAGES, gpu.bam_qc_device_ms_split):
                t["qc_%s_ms" % s].append(x)
    stat = lambda x: dict(median=round(statistics.median(x), 4), min=round(min(x), 4), max=round(max(x), 4))
    med = {k: statistics.median(x) for k, x in t.items()}
    sn = [int(x) for x in v["SN"][:16]]
    gbs = lambda ms: round(nb / (ms * 1e-3) / 1e9, 2) if ms else None
    res = dict(reads=n, batches=a.batches, runs=a.runs, warmup=a.warmup, records=n_rec, raw_bytes=nb, words=len(v["words"]), text_bytes=len(gpu.bam_qc_text(v)), granules=gpu.bam_qc_granules(),
               sn=dict(zip(("records", "malformed", "profiled", "left_out", "bases", "profiled_bases", "aligned", "mismatches", "inserted_bases", "deleted_bases", "clipped", "n_ops",
                            "skipped_bases", "bases_without_quality", "quality_sum", "pairs"), sn)),
               **{k: stat(x) for k, x in t.items()},
               array_gb_per_s=dict(qc_cycle_pass_quarter_wave_per_record=gbs(med["qc_cycle_pass_ms"]), qc_record_tables_lane_per_record=gbs(med["qc_record_tables_ms"]),
                                   markdup_record_pass_lane_per_record=gbs(med["markdup_record_pass_ms"]), pileup_counting_walk_lane_per_record=gbs(med["pileup_count_ms"])),
               cycle_pass_over_markdup_record_pass=round(med["qc_cycle_pass_ms"] / med["markdup_record_pass_ms"], 4) if med["markdup_record_pass_ms"] else None,
               qc_over_bgzf_device=round(med["qc_device_ms"] / med["bgzf_device_ms"], 4) if med["bgzf_device_ms"] else None,
               profiled_bases_per_s=round(sn[5] / (med["qc_cycle_pass_ms"] * 1e-3)) if med["qc_cycle_pass_ms"] else None)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
