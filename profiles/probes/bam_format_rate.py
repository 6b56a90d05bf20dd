"""Device time of the BAM writer (dg_batch_format_bam: k_bam_len + k_tiles_top + k_bam_write, then k_bgzf_deflate + k_tiles_top + k_bgzf_copy) on the headline
workload's shape: 1 M pairs of 2x101 on the chr20-sized planted genome at -mis 5, the batch of sam_format_rate.py.  A tool, not a test.  Prints the device time
split into record kernels and BGZF kernels, bytes read and written, raw and compressed sizes, and the share of the HBM peak.
--dynamic adds a second arm in the same process, its runs alternating with the first arm's: DG_BAM_DYNAMIC (k_bgzf_deflate_dyn in place of k_bgzf_deflate).  The
result then holds both arms ("fixed", "dynamic"), the quotient of their BGZF times, and where the dynamic kernel's time goes (dg_probe_bgzf_phases on the same
records: lane 0's clocks per phase, as shares of their sum).  The fixed arm's BGZF time is the yardstick: its kernel is the one without the flag.

    python profiles/probes/bam_format_rate.py [--dynamic] [--runs 20] [--warmup 3] [--pairs 1000000] [--cache DIR] [--out profiles/bam/bam_format_rate.json]
"""
import argparse, ctypes as C, json, os, statistics, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from dart_amd import host, synth

HBM_PEAK_GBS = 8000.0       # MI355X: 8 TB/s nominal
BLOCK, SLOT = 0xFF00, 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1000000); ap.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "dart_bench_cache"))
    ap.add_argument("--out", default=None); ap.add_argument("--dynamic", action="store_true")
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
    nb = C.c_size_t(0); n_raw = C.c_size_t(0); ct = (C.c_uint64 * 5)(); ms = C.c_float(0); split = (C.c_float * 2)()
    arms = [("fixed", 0)] + ([("dynamic", host.BAM_DYNAMIC)] if a.dynamic else [])
    rec_ms, z_ms, sizes = {k: [] for k, _ in arms}, {k: [] for k, _ in arms}, {}
    for k in range(a.warmup + a.runs):
        for arm, flags in arms:
            rc = gpu.lib.dg_batch_format_bam(gpu.ctx, C.byref(t), flags, C.byref(nb), C.byref(n_raw), ct, C.byref(ms))
            if rc:
                raise RuntimeError((gpu.lib.dg_last_error(gpu.ctx) or b"").decode())
            gpu.lib.dg_batch_bam_device_ms(gpu.ctx, split)
            sizes[arm] = (int(n_raw.value), int(nb.value), int(ct[3]), int(ct[4]))
            if k >= a.warmup:
                rec_ms[arm].append(float(split[0])); z_ms[arm].append(float(split[1]))
    # records: the batch's records, bases, names and qualities in; 8 + 4 bytes of scan state per read written and read back; the records out
    rec_in = n * 36 + used[0] * 40 + used[1] * 4 + flat.size + n * (4 + 2) + int(ho[n]) + int(qo[n]) + 2 * 4 * (n + 1) + 2 * n * 12
    gbps = lambda b, m: round(b / (m * 1e-3) / 1e9, 1) if m > 0 else None

    def result(arm):
        raw, z, records, refused = sizes[arm]
        blocks = (raw + BLOCK - 1) // BLOCK
        # BGZF: the records in; every block written to its slot and read back by the copy; the stream out; 12 bytes of sizes per block
        z_in, z_out = raw + z, 2 * z + 12 * blocks
        med_r, med_z = statistics.median(rec_ms[arm]), statistics.median(z_ms[arm])
        return {"reads": n, "runs": a.runs, "records": records, "refused": refused, "raw_bytes": raw, "bgzf_bytes": z, "bgzf_blocks": blocks, "ratio_raw_over_bgzf": round(raw / max(z, 1), 3),
                "records_ms_median": round(med_r, 4), "records_ms_min": round(min(rec_ms[arm]), 4), "records_ms_max": round(max(rec_ms[arm]), 4),
                "bgzf_ms_median": round(med_z, 4), "bgzf_ms_min": round(min(z_ms[arm]), 4), "bgzf_ms_max": round(max(z_ms[arm]), 4),
                "reads_per_s": round(n / ((med_r + med_z) * 1e-3)),
                "records_bytes_in": rec_in, "records_bytes_out": raw, "bgzf_bytes_in": z_in, "bgzf_bytes_out": z_out,
                "records_GBps": gbps(rec_in + raw, med_r), "bgzf_GBps": gbps(z_in + z_out, med_z),
                "fraction_of_hbm_peak": round((rec_in + raw + z_in + z_out) / ((med_r + med_z) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "hbm_peak_GBps_assumed": HBM_PEAK_GBS}

    res = result("fixed")
    if a.dynamic:
        dyn = result("dynamic")
        if gpu.lib.dg_batch_format_bam(gpu.ctx, C.byref(t), host.BAM_RAW, C.byref(nb), C.byref(n_raw), ct, C.byref(ms)):      # the same records, on the host
            raise RuntimeError((gpu.lib.dg_last_error(gpu.ctx) or b"").decode())
        raw_bytes = np.zeros(int(nb.value) + 1, np.uint8)
        if gpu.lib.dg_batch_download_bam(gpu.ctx, raw_bytes.ctypes.data, int(nb.value)):
            raise RuntimeError((gpu.lib.dg_last_error(gpu.ctx) or b"").decode())
        cyc, z_probe = gpu.probe_bgzf_phases(raw_bytes[:-1])
        assert len(z_probe) == dyn["bgzf_bytes"]
        tot = max(sum(cyc.values()), 1)
        res = {"fixed": res, "dynamic": dyn, "bgzf_ms_dynamic_over_fixed": round(dyn["bgzf_ms_median"] / res["bgzf_ms_median"], 3),
               "bgzf_bytes_dynamic_over_fixed": round(dyn["bgzf_bytes"] / res["bgzf_bytes"], 4),
               "dynamic_kernel_phase_share": {k: round(v / tot, 4) for k, v in cyc.items()}, "dynamic_kernel_phase_probe_ms": round(gpu.bam_device_ms, 4),
               "dynamic_kernel_phase_probe_bytes": len(raw_bytes) - 1}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
