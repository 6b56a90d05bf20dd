"""Device and wall time of duplicate marking (dg_bam_markdup_finish: the record pass, the mate sort and search, the pair sorts, the end sorts, the family scan
and the flag writes) beside the coordinate sort's finish (dg_bam_sort_finish) and the BGZF kernels (dg_bam_sort_compress) from the same runs: 1 M pairs of 2x101
on the chr20-sized planted genome at -mis 5 in 4 batches, the store of bam_sort_rate.py, plus 10 % of the pairs a second time under new names (qualities one
lower).  A tool, not a test.  Every run finishes the sort, marks, and compresses the array in pieces of 4096 blocks; prints median, min and max of --runs runs
behind --warmup.

    python profiles/probes/markdup_rate.py [--runs 10] [--warmup 2] [--pairs 1000000] [--batches 4] [--cache DIR] [--out profiles/markdup/markdup_rate.json]
    python profiles/probes/markdup_rate.py --end-to-end profiles/markdup/dart_end_to_end.json      (dart itself, with and without DART_MARK_DUPLICATES=1)
    python profiles/probes/markdup_rate.py --resources profiles/markdup/resource_usage.txt        (cross-compiles dg_markdup.h; needs no device)
"""
import argparse, json, os, re, shutil, statistics, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BLOCK = 0xFF00
STAGES = ("record_pass", "mate_sort_search", "pair_sorts", "end_sorts", "flag_writes", "count_emit")
STATS = ("examined", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "crowded_candidates", "flagged_records", "largest_family")


def resource_table(path):
    """registers, scratch, occupancy and LDS of every kernel of dg_markdup.h, as the compiler reports them for gfx950"""
    import __graft_entry__ as ge
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "md.hip")
        open(src, "w").write('#include "%s"\n' % os.path.join(ROOT, "dart_amd", "csrc", "dg_markdup.h"))
        r = subprocess.run([ge.HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(d, "md.o")],
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
            cur = dict(name=name) if name.startswith("k_md_") or name in ("k_cv_top", "k_cv_tails_top") else None      # (its own kernels and the two of dg_coverage.h it launches)
            if cur is not None:
                rows.append(cur)
        elif cur is not None:
            cur[k] = v
    cols = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch/B"), ("SGPRs Spill", "SGPRsp"), ("VGPRs Spill", "VGPRsp"),
            ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "LDS/B"), ("Dynamic Stack", "dyn.stack"))
    out = ["# hipcc -O3 --offload-arch=gfx950 -std=c++17 -Rpass-analysis=kernel-resource-usage over dart_amd/csrc/dg_markdup.h (cross-compiled; no device needed)",
           "%-18s" % "kernel" + "".join("%10s" % c for _, c in cols)]
    out += ["%-18s" % r_["name"] + "".join("%10s" % r_.get(k, "?") for k, _ in cols) for r_ in rows]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(out) + "\n")
    assert rows and all(r_.get("ScratchSize [bytes/lane]") == "0" and r_.get("SGPRs Spill") == "0" and r_.get("VGPRs Spill") == "0" for r_ in rows), "a kernel of dg_markdup.h uses scratch or spills"


def the_reads(a):
    """the index's prefix, and the interleaved reads: the pairs, then the first tenth of them again"""
    import numpy as np
    import bench
    from dart_amd import host, synth
    prefix, g = bench.prepare_index(a.cache, bench.CHR20_LEN, 0, lambda: None)
    m1, m2 = synth.make_reads(g, a.pairs, rlen=101, seed=1000, sub_rate=0.01, indel_frac=0.02, n_frac=0.002)
    extra = a.pairs // 10
    return prefix, np.concatenate([m1, m1[:extra]]), np.concatenate([m2, m2[:extra]]), extra


def end_to_end(a):
    """dart, process start to exit: a warm-up run, three runs without the switch (the baseline's own spread), one with it"""
    prefix, m1, m2, extra = the_reads(a)
    d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        n = len(m1)
        for mate, m in ((1, m1), (2, m2)):
            with open(os.path.join(d, "%d.fq" % mate), "wb") as f:
                for i in range(n):
                    copy = i >= a.pairs
                    f.write(b"@%s%09d/%d\n" % (b"c" if copy else b"r", i - a.pairs if copy else i, mate) + m[i].tobytes() + b"\n+\n" + (b"H" if copy else b"I") * 101 + b"\n")
        args = [os.path.join(ROOT, "dart_amd", "dart"), "-i", prefix, "-f", "1.fq", "-f2", "2.fq", "-j", "out.j", "-t", "16", "-mis", "5", "-bo", "out.bam"]
        base = dict(os.environ, DART_DEVICE_BAM="1", DART_SORT_BAM="1", DART_BAM_INDEX="1", DART_TIMING="1")
        base.pop("DART_MARK_DUPLICATES", None)

        def run(env):
            t0 = time.perf_counter()
            r = subprocess.run(args, cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
            return time.perf_counter() - t0, r.stderr.decode("latin1")
        warm, _ = run(base)
        without = [round(run(base)[0], 3) for _ in range(3)]
        plain_size = os.path.getsize(os.path.join(d, "out.bam"))
        with_s, err = run(dict(base, DART_MARK_DUPLICATES="1"))
        note = [l for l in err.splitlines() if l.startswith("[dart timing] markdup:")]
        res = dict(what="dart end to end, process start to exit: %d pairs 2x101 (the probe's reads, seed 1000, the first tenth twice) as two FASTQ files on tmpfs against the chr20-sized "
                        "planted genome's index, -bo out.bam -j out.j -t 16 -mis 5 with DART_DEVICE_BAM=1 DART_SORT_BAM=1 DART_BAM_INDEX=1, one MI355X; in this order: a warm-up run, "
                        "three runs without, one with DART_MARK_DUPLICATES=1" % n,
                   warm_up_wall_s=round(warm, 3), without_wall_s=without, with_wall_s=round(with_s, 3), bam_bytes_without=plain_size, bam_bytes_with=os.path.getsize(os.path.join(d, "out.bam")),
                   markdup_txt=open(os.path.join(d, "out.bam.markdup.txt")).read(), markdup_note=note[0] if note else "")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.end_to_end)), exist_ok=True)
    open(a.end_to_end, "w").write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1000000); ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "dart_bench_cache")); ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None); ap.add_argument("--end-to-end", default=None)
    a = ap.parse_args()
    if a.resources:
        resource_table(a.resources)
        return
    if a.end_to_end:
        end_to_end(a)
        return
    from dart_amd import host
    prefix, m1, m2, extra = the_reads(a)
    reads = host.interleave_pairs(m1, m2)
    n = len(reads)
    gpu = host.DartGPU(host.Index(prefix), host.default_params(paired=1, max_mismatch=5))
    ids = [(("r%09d" % (i // 2)) if i < 2 * a.pairs else ("c%09d" % (i // 2 - a.pairs))).encode() for i in range(n)]
    quals = [b"I" * 101] * (2 * a.pairs) + [b"H" * 101] * (2 * extra)
    cuts = [(n * k // a.batches) & ~1 for k in range(a.batches)] + [n]
    for k in range(a.batches):
        lo, hi = cuts[k], cuts[k + 1]
        so, rl, flat = host.pack_reads(reads[lo:hi])
        gpu.map_batch(so, rl, flat)
        gpu.format_bam(ids[lo:hi], quals[lo:hi], hi - lo, raw=True)
        gpu.accumulate_bam(k)
    t = {k: [] for k in ("sort_finish_device_ms", "sort_finish_wall_ms", "markdup_device_ms", "markdup_wall_ms", "markdup_count_only_wall_ms", "bgzf_device_ms", "compress_wall_ms") +
         tuple("markdup_%s_ms" % s for s in STAGES)}
    for r in range(a.warmup + a.runs):
        w0 = time.perf_counter()
        n_rec, nb = gpu.bam_sort_finish()
        w1 = time.perf_counter()
        gpu.bam_markdup_finish(count_only=True)
        w2 = time.perf_counter()
        st = gpu.bam_markdup_finish()
        w3 = time.perf_counter()
        split, dev, passes = gpu.bam_markdup_device_ms_split, gpu.bam_markdup_device_ms, gpu.bam_markdup_passes
        z_ms, z_bytes = 0.0, 0
        for off in range(0, nb, 4096 * BLOCK):
            z_bytes += len(gpu.bam_sort_compress(off, min(4096 * BLOCK, nb - off))); z_ms += gpu.bam_device_ms
        w4 = time.perf_counter()
        if r >= a.warmup:
            t["sort_finish_device_ms"].append(gpu.bam_sort_device_ms); t["sort_finish_wall_ms"].append((w1 - w0) * 1e3)
            t["markdup_device_ms"].append(dev); t["markdup_wall_ms"].append((w3 - w2) * 1e3); t["markdup_count_only_wall_ms"].append((w2 - w1) * 1e3)
            t["bgzf_device_ms"].append(z_ms); t["compress_wall_ms"].append((w4 - w3) * 1e3)
            for s, v in zip(STAGES, split):
                t["markdup_%s_ms" % s].append(v)
    stat = lambda v: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = dict(reads=n, batches=a.batches, runs=a.runs, warmup=a.warmup, records=n_rec, raw_bytes=nb, bgzf_bytes=z_bytes, sort_passes=passes, launches_per_pass=5,
               markdup_stats=dict(zip(STATS, st)), **{k: stat(v) for k, v in t.items()},
               dominant_stage=max(STAGES, key=lambda s: med["markdup_%s_ms" % s]),
               markdup_over_sort_finish_device=round(med["markdup_device_ms"] / med["sort_finish_device_ms"], 4),
               markdup_over_bgzf_device=round(med["markdup_device_ms"] / med["bgzf_device_ms"], 4),
               records_per_s_markdup=round(n_rec / (med["markdup_device_ms"] * 1e-3)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
