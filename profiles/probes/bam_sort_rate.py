"""Device time of the coordinate sort (dg_batch_accumulate_bam per batch; dg_bam_sort_finish: segment ordering, the radix sort, the length pass, the gather;
dg_bam_sort_compress: the BGZF kernels) on the headline workload's shape: 1 M pairs of 2x101 on the chr20-sized planted genome at -mis 5, the reads of
sam_format_rate.py, in --batches batches.  A tool, not a test.  Prints device ms of the key kernels per batch, of every phase of the finish (median, min
and max of --runs runs behind --warmup), bytes moved, and the share of the HBM peak the gather reaches.

    python profiles/probes/bam_sort_rate.py [--runs 10] [--warmup 2] [--pairs 1000000] [--batches 4] [--cache DIR] [--out profiles/bamsort/bam_sort_rate.json]
"""
import argparse, json, os, statistics, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from dart_amd import host, synth

HBM_PEAK_GBS = 8000.0       # MI355X: 8 TB/s nominal
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
    acc_ms, per_batch = [], []
    for k in range(a.batches):
        lo, hi = cuts[k], cuts[k + 1]
        so, rl, flat = host.pack_reads(reads[lo:hi])
        gpu.map_batch(so, rl, flat)
        raw, ct = gpu.format_bam(ids[lo:hi], quals[lo:hi], hi - lo, raw=True)
        records = gpu.accumulate_bam(k)
        acc_ms.append(gpu.bam_sort_accumulate_ms); per_batch.append(dict(reads=hi - lo, records=records, raw_bytes=len(raw), key_kernels_and_copy_ms=round(gpu.bam_sort_accumulate_ms, 4)))
    phases = {k: [] for k in ("segments", "sort", "lengths", "gather", "bgzf")}
    for r in range(a.warmup + a.runs):
        n_rec, nb = gpu.bam_sort_finish()
        z_ms, z_bytes = 0.0, 0
        for off in range(0, nb, 4096 * BLOCK):                # pieces of 4096 blocks (255 MB)
            z = gpu.bam_sort_compress(off, min(4096 * BLOCK, nb - off))
            z_ms += gpu.bam_device_ms; z_bytes += len(z)
        if r >= a.warmup:
            for name, ms in zip(("segments", "sort", "lengths", "gather"), gpu.bam_sort_device_ms_split):
                phases[name].append(ms)
            phases["bgzf"].append(z_ms)
    passes = gpu.bam_sort_passes
    stat = lambda v: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    med = {k: statistics.median(v) for k, v in phases.items()}
    gbps = lambda b, ms: round(b / (ms * 1e-3) / 1e9, 1) if ms > 0 else None
    # bytes moved: segments: 16 B per record in and out; a sort pass: keys read twice, values once, both written; lengths: offset + 4 bytes of the record in,
    # 8 out; gather: offset and place in, the record in and out
    moved = dict(segments=32 * n_rec, sort=passes * 40 * n_rec, lengths=20 * n_rec, gather=16 * n_rec + 2 * nb, bgzf_in=nb, bgzf_out=z_bytes)
    res = dict(reads=n, batches=a.batches, runs=a.runs, warmup=a.warmup, records=n_rec, raw_bytes=nb, bgzf_bytes=z_bytes, per_batch=per_batch,
               accumulate_ms_per_batch=stat(acc_ms), finish_ms={k: stat(v) for k, v in phases.items() if k != "bgzf"}, sort_passes=passes,
               sort_ms_per_pass_median=round(med["sort"] / max(passes, 1), 4), bgzf_ms=stat(phases["bgzf"]), bytes_moved=moved,
               gather_GBps=gbps(moved["gather"], med["gather"]), gather_fraction_of_hbm_peak=round(moved["gather"] / (med["gather"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if med["gather"] > 0 else None,
               sort_GBps=gbps(moved["sort"], med["sort"]), records_per_s_finish=round(n_rec / (sum(med[k] for k in ("segments", "sort", "lengths", "gather")) * 1e-3)),
               hbm_peak_GBps_assumed=HBM_PEAK_GBS)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
