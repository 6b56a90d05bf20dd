"""Device and wall time of the allele counts (dg_bam_pileup_finish: the counting and emitting walks over the bases and the 2-bit text, the event sort, the plane and
tail scans with the compaction, sites and text) beside the coverage track (dg_bam_coverage_finish) and the BGZF kernels (dg_bam_sort_compress) over the same
sorted array: 1 M pairs of 2x101 on the chr20-sized planted genome at -mis 5, the reads and batches of bam_sort_rate.py.  A tool, not a test.  Device time from
events; prints median, min and max of --runs runs behind --warmup.

    python profiles/probes/pileup_rate.py [--runs 10] [--warmup 2] [--pairs 1000000] [--batches 4] [--cache DIR] [--out profiles/pileup/pileup_rate.json]
    python profiles/probes/pileup_rate.py --resources profiles/pileup/resource_usage.txt      (cross-compiles dg_pileup.h; needs no device)
"""
import argparse, json, os, re, statistics, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BLOCK = 0xFF00
STAGES = ("count", "emit", "sort", "scans", "sites_text")


def resource_table(path):
    """registers, scratch, occupancy and LDS of every kernel of dg_pileup.h, as the compiler reports them for gfx950"""
    import __graft_entry__ as ge
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "pu.hip")
        open(src, "w").write('#include "%s"\n' % os.path.join(ROOT, "dart_amd", "csrc", "dg_pileup.h"))
        r = subprocess.run([ge.HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(d, "pu.o")],
                           capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            m = re.match(r"_Z(\d+)", v)                       # _Z<length><name><parameters>
            name = v[len(m.group(0)):len(m.group(0)) + int(m.group(1))] if m else v
            cur = dict(name=name) if name.startswith("k_pu_") else None      # (the header includes the coverage track's, the sorter's and the formatter's kernels)
            if cur is not None:
                rows.append(cur)
        elif cur is not None:
            cur[k] = v
    cols = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch/B"), ("SGPRs Spill", "SGPRsp"), ("VGPRs Spill", "VGPRsp"),
            ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "LDS/B"), ("Dynamic Stack", "dyn.stack"))
    out = ["# hipcc -O3 --offload-arch=gfx950 -std=c++17 -Rpass-analysis=kernel-resource-usage over dart_amd/csrc/dg_pileup.h (cross-compiled; no device needed)",
           "%-18s" % "kernel" + "".join("%10s" % c for _, c in cols)]
    out += ["%-18s" % r_["name"] + "".join("%10s" % r_.get(k, "?") for k, _ in cols) for r_ in rows]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(out) + "\n")
    assert rows and all(r_.get("ScratchSize [bytes/lane]") == "0" and r_.get("VGPRs Spill") == "0" and r_.get("SGPRs Spill") == "0" for r_ in rows), "a kernel of dg_pileup.h uses scratch or spills"


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
    t = {k: [] for k in ("sort_finish_device_ms", "bgzf_device_ms", "coverage_device_ms", "pileup_device_ms", "pileup_wall_ms", "pileup_entries_only_wall_ms") + tuple("pileup_%s_ms" % s for s in STAGES)}
    for r in range(a.warmup + a.runs):
        n_rec, nb = gpu.bam_sort_finish()
        z_ms = 0.0
        for off in range(0, nb, 4096 * BLOCK):
            gpu.bam_sort_compress(off, min(4096 * BLOCK, nb - off))
            z_ms += gpu.bam_device_ms
        gpu.bam_coverage_finish()
        cov_ms = gpu.bam_coverage_device_ms
        w0 = time.perf_counter()
        ent, text = gpu.bam_pileup_finish()                   # (the wall times hold the downloads too)
        w1 = time.perf_counter()
        split, dev, st, passes = gpu.bam_pileup_device_ms_split, gpu.bam_pileup_device_ms, gpu.bam_pileup_stats, gpu.bam_pileup_passes
        gpu.bam_pileup_finish(entries_only=True)
        w2 = time.perf_counter()
        if r >= a.warmup:
            t["sort_finish_device_ms"].append(gpu.bam_sort_device_ms); t["bgzf_device_ms"].append(z_ms); t["coverage_device_ms"].append(cov_ms)
            t["pileup_device_ms"].append(dev); t["pileup_wall_ms"].append((w1 - w0) * 1e3); t["pileup_entries_only_wall_ms"].append((w2 - w1) * 1e3)
            for s, v in zip(STAGES, split):
                t["pileup_%s_ms" % s].append(v)
    stat = lambda v: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    med = {k: statistics.median(v) for k, v in t.items()}
    events = 2 * st[1] + st[3] + st[4] + st[5]
    res = dict(reads=n, batches=a.batches, runs=a.runs, warmup=a.warmup, records=n_rec, raw_bytes=nb, sites_kept=len(ent), text_bytes=len(text), sort_passes=passes,
               pileup_stats=dict(counted=st[0], blocks=st[1], aligned_bases=st[2], mismatches=st[3], deleted_bases=st[4], insertions=st[5], sites=st[6], kept=st[7], left_out=st[8],
                                 largest_depth=st[9], events=events),
               **{k: stat(v) for k, v in t.items()},
               dominant_stage=max(STAGES, key=lambda s: med["pileup_%s_ms" % s]),
               pileup_over_coverage_device=round(med["pileup_device_ms"] / med["coverage_device_ms"], 4),
               pileup_over_bgzf_device=round(med["pileup_device_ms"] / med["bgzf_device_ms"], 4) if med["bgzf_device_ms"] else None,
               aligned_bases_per_s_pileup=round(st[2] / (med["pileup_device_ms"] * 1e-3)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
