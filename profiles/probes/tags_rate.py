"""Device time of the MD / NM / ts stage (dg_bam_tags_finish: the length pass, lane = record, and the write pass: k_tg_tail, lane = record, and k_tg_copy, sixteen lanes = record) beside the sort's gather
(k_bs_gather, a wave = record: it moves the same record bytes without looking at them -- the yardstick of the write pass) and the BGZF kernels, all over the same
sorted array in the same run: 1 M pairs of 2x101 on the chr20-sized planted genome at -mis 5, the reads and batches of bam_sort_rate.py.  A tool, not a test.
Device time from events; prints median, min and max of --runs runs behind --warmup.

    python profiles/probes/tags_rate.py [--runs 10] [--warmup 2] [--pairs 1000000] [--batches 4] [--cache DIR] [--out profiles/tags/tags_rate.json]
    python profiles/probes/tags_rate.py --resources profiles/tags/resource_usage.txt      (cross-compiles dg_tags.h; needs no device)
"""
import argparse, json, os, re, statistics, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BLOCK = 0xFF00
STATS = ("rewritten", "not_eligible", "aux_unreadable", "old_tags_removed", "mismatches", "inserted_plus_deleted_bases", "ts_written", "introns_without_ts")


def resource_table(path):
    """registers, scratch, occupancy and LDS of every kernel of dg_tags.h, as the compiler reports them for gfx950"""
    import __graft_entry__ as ge
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "tags.hip")
        open(src, "w").write('#include "%s"\n' % os.path.join(ROOT, "dart_amd", "csrc", "dg_tags.h"))
        r = subprocess.run([ge.HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-c", "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", src,
                            "-o", os.path.join(d, "tags.o")], capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            m = re.match(r"_Z(\d+)", v)                       # _Z<length><name><parameters>
            name = v[len(m.group(0)):len(m.group(0)) + int(m.group(1))] if m else v
            cur = dict(name=name) if name.startswith("k_tg_") else None      # (the header includes the allele counts', the coverage track's, the sorter's and the formatter's kernels)
            if cur is not None:
                rows.append(cur)
        elif cur is not None:
            cur[k] = v
    cols = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch/B"), ("SGPRs Spill", "SGPRsp"), ("VGPRs Spill", "VGPRsp"),
            ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "LDS/B"), ("Dynamic Stack", "dyn.stack"))
    out = ["# hipcc -O3 --offload-arch=gfx950 -std=c++17 -Rpass-analysis=kernel-resource-usage over dart_amd/csrc/dg_tags.h (cross-compiled; no device needed)",
           "%-18s" % "kernel" + "".join("%10s" % c for _, c in cols)]
    out += ["%-18s" % r_["name"] + "".join("%10s" % r_.get(k, "?") for k, _ in cols) for r_ in rows]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(out) + "\n")
    assert len(rows) == 3 and all(r_.get("ScratchSize [bytes/lane]") == "0" and r_.get("VGPRs Spill") == "0" and r_.get("SGPRs Spill") == "0" for r_ in rows), "a kernel of dg_tags.h uses scratch or spills"


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
    import ctypes
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
    t = {k: [] for k in ("sort_finish_device_ms", "gather_ms", "bgzf_device_ms", "tags_device_ms", "tags_wall_ms", "tags_length_pass_ms", "tags_write_pass_ms", "tags_write_tail_ms", "tags_write_copy_ms", "tags_md_only_write_pass_ms")}
    for r in range(a.warmup + a.runs):
        n_rec, nb = gpu.bam_sort_finish()
        gather = gpu.bam_sort_device_ms_split[3]
        gpu.bam_tags_finish(md=True, nm=False, ts=False)
        md_only = gpu.bam_tags_device_ms_split[1]
        gpu.bam_sort_finish()                                 # (the untagged array again: every run tags the same bytes)
        w0 = time.perf_counter()
        nb_out, st = gpu.bam_tags_finish()
        w1 = time.perf_counter()
        wr = (ctypes.c_float * 2)()
        assert gpu.lib.dg_bam_tags_write_ms(gpu.ctx, wr) == 0
        z_ms = 0.0
        for off in range(0, nb_out, 4096 * BLOCK):            # the BGZF kernels over the tagged array: what the file is made of
            gpu.bam_sort_compress(off, min(4096 * BLOCK, nb_out - off))
            z_ms += gpu.bam_device_ms
        if r >= a.warmup:
            t["sort_finish_device_ms"].append(gpu.bam_sort_device_ms); t["gather_ms"].append(gather); t["bgzf_device_ms"].append(z_ms)
            t["tags_device_ms"].append(gpu.bam_tags_device_ms); t["tags_wall_ms"].append((w1 - w0) * 1e3)
            t["tags_length_pass_ms"].append(gpu.bam_tags_device_ms_split[0]); t["tags_write_pass_ms"].append(gpu.bam_tags_device_ms_split[1]); t["tags_md_only_write_pass_ms"].append(md_only)
            t["tags_write_tail_ms"].append(float(wr[0])); t["tags_write_copy_ms"].append(float(wr[1]))
    stat = lambda x: dict(median=round(statistics.median(x), 4), min=round(min(x), 4), max=round(max(x), 4))
    med = {k: statistics.median(x) for k, x in t.items()}
    gbs = lambda ms, b: round(b / (ms * 1e-3) / 1e9, 2) if ms else None
    ratio = lambda x, y: round(x / y, 4) if y else None
    res = dict(reads=n, batches=a.batches, runs=a.runs, warmup=a.warmup, records=n_rec, bytes_in=nb, bytes_out=nb_out, granules=gpu.bam_tags_granules(), stats=dict(zip(STATS, st)),
               **{k: stat(x) for k, x in t.items()},
               array_gb_per_s=dict(gather_wave_per_record=gbs(med["gather_ms"], nb), tags_length_pass_lane_per_record=gbs(med["tags_length_pass_ms"], nb),
                                   tags_write_tail_lane_per_record=gbs(med["tags_write_tail_ms"], nb),
                                   tags_write_copy_sixteen_lanes_per_record_in_plus_out=gbs(med["tags_write_copy_ms"], nb + nb_out), gather_in_plus_out=gbs(med["gather_ms"], 2 * nb)),
               write_pass_over_gather=ratio(med["tags_write_pass_ms"], med["gather_ms"]), write_copy_over_gather=ratio(med["tags_write_copy_ms"], med["gather_ms"]),
               write_pass_over_gather_plus_length_pass=ratio(med["tags_write_pass_ms"], med["gather_ms"] + med["tags_length_pass_ms"]),
               tags_over_bgzf_device=ratio(med["tags_device_ms"], med["bgzf_device_ms"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
