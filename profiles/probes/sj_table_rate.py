"""The junction table on the device against the host's map, on the spliced 2x151 shape of the README.  A tool, not a test.
  library   one batch of --pairs spliced pairs on the chr20-sized planted genome: time of dg_batch_accumulate_sj on a fresh table (host wall clock around
            the call: one launch, one wait, growth included) and on a table that already holds the keys, and of dg_sj_finish (device time and wall clock)
  dart      the same reads as FASTQ files through `dart` with and without DART_DEVICE_SJ=1: the two `[dart sj]` lines and the job's wall time

    python profiles/probes/sj_table_rate.py [--runs 10] [--pairs 500000] [--cache DIR] [--out profiles/sj/sj_table_rate.json]
"""
import argparse, json, os, statistics, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from dart_amd import host, synth

DART = os.path.join(ROOT, "dart_amd", "dart")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10); ap.add_argument("--pairs", type=int, default=500000)
    ap.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "dart_bench_cache")); ap.add_argument("--out", default=None)
    ap.add_argument("--no-dart", action="store_true")
    a = ap.parse_args()
    prefix, g = bench.prepare_index(a.cache, bench.CHR20_LEN, 0, lambda: None)
    m1, m2 = synth.make_reads(g, a.pairs, rlen=151, seed=1000, spliced_frac=0.35, sub_rate=0.01, indel_frac=0.02, n_frac=0.002)
    so, rl, flat = host.pack_reads(host.interleave_pairs(m1, m2))
    gpu = host.DartGPU(host.Index(prefix), host.default_params(paired=1, max_mismatch=5))
    gpu.upload(so, rl, flat)
    fresh_ms, warm_ms, fin_ms, fin_wall_ms = [], [], [], []
    tuples = entries = 0
    for k in range(a.runs + 1):
        gpu.sj_reset()
        gpu.run()                                                  # (a batch is counted once: every timing gets a batch of its own)
        t = time.perf_counter(); tuples = gpu.accumulate_sj(); d_fresh = (time.perf_counter() - t) * 1e3
        gpu.run()
        t = time.perf_counter(); gpu.accumulate_sj(); d_warm = (time.perf_counter() - t) * 1e3
        t = time.perf_counter(); ent, text = gpu.sj_finish(); d_fin = (time.perf_counter() - t) * 1e3
        entries = len(ent)
        if k:                                                      # the first round grows the table from its first size
            fresh_ms.append(d_fresh); warm_ms.append(d_warm); fin_ms.append(gpu.sj_device_ms); fin_wall_ms.append(d_fin)
    med = lambda v: round(statistics.median(v), 4)
    res = {"pairs": a.pairs, "rlen": 151, "tuples": tuples, "entries": entries, "text_bytes": len(text), "runs": a.runs,
           "accumulate_ms_fresh_table_median": med(fresh_ms), "accumulate_ms_warm_table_median": med(warm_ms), "accumulate_ms_warm_table_min": round(min(warm_ms), 4),
           "tuples_per_s_warm": round(tuples / (statistics.median(warm_ms) * 1e-3)) if tuples else 0,
           "tuple_download_bytes_avoided": tuples * 24, "finish_device_ms_median": med(fin_ms), "finish_wall_ms_median": med(fin_wall_ms)}
    gpu.close()
    if not a.no_dart:
        d = tempfile.mkdtemp()
        synth.write_fastq(os.path.join(d, "1.fq"), m1, 1); synth.write_fastq(os.path.join(d, "2.fq"), m2, 2)
        for tag, extra in (("host", {}), ("device", {"DART_DEVICE_SJ": "1"})):
            best = None
            for _ in range(3):
                t = time.perf_counter()
                r = subprocess.run([DART, "-i", prefix, "-f", "1.fq", "-f2", "2.fq", "-mis", "5", "-o", "o.sam", "-j", tag + ".j", "-t", "16"], cwd=d,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, DART_TIMING="1", **extra), check=True)
                wall = time.perf_counter() - t
                line = [l for l in r.stderr.decode("latin1").splitlines() if l.startswith("[dart sj]")][-1]
                if best is None or wall < best[0]:
                    best = (wall, line)
            res["dart_%s_wall_s_best_of_3" % tag] = round(best[0], 3); res["dart_%s_line" % tag] = best[1]
        res["junction_files_equal"] = open(os.path.join(d, "host.j")).read() == open(os.path.join(d, "device.j")).read()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
