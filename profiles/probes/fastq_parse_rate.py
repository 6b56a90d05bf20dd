"""Device time of the FASTQ parser (dg_batch_upload_fastq: k_fq_count, k_fq_top, k_fq_lines, k_fq_len, k_fq_top3, k_fq_write) on the headline workload's
shape: the FASTQ text of 1 M pairs of 2x101 of the chr20-sized planted genome, as two files.  A tool, not a test.  Prints reads/s and the achieved fraction
of the HBM peak for bytes read + bytes written by the six kernels (the host-to-device copy of the text is outside the timed events).

    python profiles/probes/fastq_parse_rate.py [--runs 20] [--warmup 3] [--pairs 1000000] [--cache DIR] [--out FILE]
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
    d = tempfile.mkdtemp()
    synth.write_fastq_fast(os.path.join(d, "1.fq"), m1, 1); synth.write_fastq_fast(os.path.join(d, "2.fq"), m2, 2)
    t1 = np.fromfile(os.path.join(d, "1.fq"), np.uint8); t2 = np.fromfile(os.path.join(d, "2.fq"), np.uint8)
    n = 2 * a.pairs
    gpu = host.DartGPU(host.Index(prefix), host.default_params(paired=1, max_mismatch=5))
    t = host.FastqText(); t.text1, t.n1, t.text2, t.n2, t.rc_odd_reads, t.max_reads = t1.ctypes.data, t1.size, t2.ctypes.data, t2.size, 1, n
    got = C.c_int(0); ms = C.c_float(0)
    times = []
    for k in range(a.warmup + a.runs):
        rc = gpu.lib.dg_batch_upload_fastq(gpu.ctx, C.byref(t), C.byref(got))
        if rc or got.value != n:
            raise RuntimeError("%d reads: %s" % (got.value, (gpu.lib.dg_last_error(gpu.ctx) or b"").decode()))
        gpu.lib.dg_batch_fastq_device_ms(gpu.ctx, C.byref(ms))
        if k >= a.warmup:
            times.append(float(ms.value))
    gpu._n = n
    so, rl, flat, names, quals = gpu.download_reads()
    want_so, want_rl, want_flat = host.pack_reads(host.interleave_pairs(m1, m2))
    same = bool(np.array_equal(so, want_so) and np.array_equal(rl, want_rl) and np.array_equal(flat, want_flat))
    med = statistics.median(times)
    text = int(t1.size + t2.size); lines = 4 * n
    out_bytes = int(flat.size) + sum(len(x) for x in names) + sum(len(x) for x in quals)
    # the text is read three times (count, line starts, copy -- the copy reads what it writes), line starts written once and read by two kernels,
    # per read 2 + 4 + 4 + 3 x 4 bytes of lengths and local offsets written and read back, 3 x 4 bytes of final offsets written
    bytes_in = 2 * text + out_bytes + 2 * 4 * lines + n * 22
    bytes_out = 4 * lines + n * 22 + out_bytes + n * 12
    res = {"reads": n, "runs": a.runs, "text_bytes": text, "device_ms_median": round(med, 4), "device_ms_min": round(min(times), 4), "device_ms_max": round(max(times), 4),
           "reads_per_s": round(n / (med * 1e-3)), "text_GBps": round(text / (med * 1e-3) / 1e9, 1), "bytes_in": bytes_in, "bytes_out": bytes_out,
           "achieved_GBps": round((bytes_in + bytes_out) / (med * 1e-3) / 1e9, 1),
           "fraction_of_hbm_peak": round((bytes_in + bytes_out) / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "hbm_peak_GBps_assumed": HBM_PEAK_GBS,
           "batch_equals_host_packer": same}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
