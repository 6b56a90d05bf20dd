"""Device time of the SAM formatter (dg_batch_format_sam: k_sam_len + k_tiles_top + k_sam_write) on the headline workload's shape: 1 M pairs of 2x101 on the
chr20-sized planted genome at -mis 5.  A tool, not a test.  Prints reads/s and the achieved fraction of the HBM peak for bytes in + bytes out.

    python profiles/probes/sam_format_rate.py [--runs 20] [--warmup 3] [--pairs 1000000] [--cache DIR] [--out FILE]
"""
import argparse, ctypes as C, json, os, statistics, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from dart_amd import host, synth

HBM_PEAK_GBS = 8000.0       # MI355X: 8 TB/s nominal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1000000); ap.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "dart_bench_cache"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    prefix, g = bench.prepare_index(a.cache, bench.CHR20_LEN, 0, lambda: None)
    m1, m2 = synth.make_reads(g, a.pairs, rlen=101, seed=1000, sub_rate=0.01, indel_frac=0.02, n_frac=0.002)
    so, rl, flat = host.pack_reads(host.interleave_pairs(m1, m2))
    n = 2 * a.pairs
    gpu = host.DartGPU(host.Index(prefix), host.default_params(paired=1, max_mismatch=5))
    gpu.upload(so, rl, flat)
    used = gpu.run()
    ids = np.char.add("r", np.char.zfill(np.repeat(np.arange(a.pairs), 2).astype(str), 9))
    ho, hb = host.flatten_strings([s.encode() for s in ids.tolist()])
    qo = (np.arange(n + 1, dtype=np.uint64) * 101).astype(np.uint32); qb = np.full(n * 101 + 1, ord("I"), np.uint8)
    t = host.SamText(); t.hdr_off, t.hdr, t.qual_off, t.qual, t.n_pair_mode = ho.ctypes.data, hb.ctypes.data, qo.ctypes.data, qb.ctypes.data, n
    nb = C.c_size_t(0); ct = (C.c_uint64 * 3)(); ms = C.c_float(0)
    times = []
    for k in range(a.warmup + a.runs):
        rc = gpu.lib.dg_batch_format_sam(gpu.ctx, C.byref(t), 0, C.byref(nb), ct, C.byref(ms))
        if rc:
            raise RuntimeError((gpu.lib.dg_last_error(gpu.ctx) or b"").decode())
        if k >= a.warmup:
            times.append(float(ms.value))
    med = statistics.median(times)
    bytes_in = n * 36 + used[0] * 40 + used[1] * 4 + flat.size + n * (4 + 2) + int(ho[n]) + int(qo[n]) + 2 * 4 * (n + 1)
    # pass 1 leaves 8 + 4 bytes per read for pass 2, which reads them back
    bytes_scan = 2 * n * 12
    bytes_out = int(nb.value)
    res = {"reads": n, "runs": a.runs, "device_ms_median": round(med, 4), "device_ms_min": round(min(times), 4), "device_ms_max": round(max(times), 4),
           "reads_per_s": round(n / (med * 1e-3)), "bytes_in": bytes_in, "bytes_out": bytes_out, "bytes_scan_state": bytes_scan,
           "achieved_GBps": round((bytes_in + bytes_out) / (med * 1e-3) / 1e9, 1),
           "fraction_of_hbm_peak": round((bytes_in + bytes_out) / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "hbm_peak_GBps_assumed": HBM_PEAK_GBS}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
