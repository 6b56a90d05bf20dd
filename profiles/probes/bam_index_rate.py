"""Device and wall time of the BAM index (dg_bam_index_finish: the per-record pass, the chunk sort, the merge, the serialisation) beside the coordinate sort's
finish (dg_bam_sort_finish) on the same store: 1 M pairs of 2x101 on the chr20-sized planted genome at -mis 5, the reads and batches of bam_sort_rate.py.
A tool, not a test.  Every run finishes the sort, compresses the array in pieces of 4096 blocks (which records the blocks' sizes) and builds the index; prints
median, min and max of --runs runs behind --warmup.

    python profiles/probes/bam_index_rate.py [--runs 10] [--warmup 2] [--pairs 1000000] [--batches 4] [--cache DIR] [--out profiles/bamidx/bam_index_rate.json]
"""
import argparse, json, os, statistics, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from dart_amd import host, synth

BLOCK = 0xFF00


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1000000); ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "dart_bench_cache")); ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
    t = {k: [] for k in ("sort_finish_device_ms", "sort_finish_wall_ms", "index_device_ms", "index_wall_ms")}
    for r in range(a.warmup + a.runs):
        w0 = time.perf_counter()
        n_rec, nb = gpu.bam_sort_finish()
        w1 = time.perf_counter()
        for off in range(0, nb, 4096 * BLOCK):
            gpu.bam_sort_compress(off, min(4096 * BLOCK, nb - off))
        w2 = time.perf_counter()
        bai = gpu.bam_index_finish(0)                          # (the wall time holds the download of the index too)
        w3 = time.perf_counter()
        if r >= a.warmup:
            t["sort_finish_device_ms"].append(gpu.bam_sort_device_ms); t["sort_finish_wall_ms"].append((w1 - w0) * 1e3)
            t["index_device_ms"].append(gpu.bam_index_device_ms); t["index_wall_ms"].append((w3 - w2) * 1e3)
    stat = lambda v: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    med = {k: statistics.median(v) for k, v in t.items()}
    st = gpu.bam_index_stats
    res = dict(reads=n, batches=a.batches, runs=a.runs, warmup=a.warmup, records=n_rec, raw_bytes=nb, index_bytes=len(bai),
               index_stats=dict(placed=st[0], n_no_coor=st[1], bins=st[2], chunks_before_merge=st[3], chunks=st[4], linear_entries=st[5]),
               **{k: stat(v) for k, v in t.items()},
               index_over_sort_finish_device=round(med["index_device_ms"] / med["sort_finish_device_ms"], 4),
               index_over_sort_finish_wall=round(med["index_wall_ms"] / med["sort_finish_wall_ms"], 4),
               records_per_s_index=round(n_rec / (med["index_device_ms"] * 1e-3)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
