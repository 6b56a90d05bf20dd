"""Device time of the trimming stage inside the FASTQ upload (dg_set_trim: k_trim_cut, k_trim_len, k_trim_top3, k_trim_write) beside the plain parser's, on the
FASTQ text of 1 M pairs of 2x101 as two files: random reads, a third of them with adapter read-through from a random insert size on under low qualities, a few
with a poly-G tail.  A tool, not a test.

    python profiles/probes/trim_rate.py --mode trim  [--runs 20] [--warmup 3] [--pairs 1000000] [--cache DIR] [--out FILE]
        all steps on: per upload dg_batch_trim_stats' device_ms and dg_batch_fastq_device_ms; then the same text untrimmed on the same context
    python profiles/probes/trim_rate.py --mode plain ...
        untrimmed uploads only (dg_batch_fastq_device_ms): runs with any build of the library (DARTGPU_LIB), for A/B series against the parent commit

The index is a small one (the upload does not look at it); text and index are cached under --cache.  --out appends one JSON line.
"""
import argparse, ctypes as C, json, os, statistics, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from dart_amd import host, synth, index_build

ADAPTER = np.frombuffer(b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC", np.uint8)


def make_text(pairs, seed, tag):
    """fixed-width records, built as one array: '@r%09d/t\\n' + 101 bases + '\\n+\\n' + 101 qualities + '\\n'"""
    rng = np.random.default_rng(seed)
    L = 101
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(pairs, L))].copy()
    qual = (33 + 30 + rng.integers(0, 11, size=(pairs, L))).astype(np.uint8)
    third = np.arange(pairs) % 3 == 0
    ins = rng.integers(0, L - 4, size=pairs)
    col = np.arange(L)[None, :]
    rel = col - ins[:, None]
    ad = third[:, None] & (rel >= 0) & (rel < ADAPTER.size)
    seq[ad] = ADAPTER[rel[ad]]
    qual[third[:, None] & (col >= np.maximum(ins, L - 15)[:, None])] = 35
    tail = (np.arange(pairs) % 17 == 1) & ~third
    n_g = rng.integers(12, 30, size=pairs)
    seq[tail[:, None] & (col >= (L - n_g)[:, None])] = ord("G")
    name = np.frombuffer(b"".join(b"@r%09d/%d\n" % (i, tag) for i in range(pairs)), np.uint8).reshape(pairs, 14)
    rec = np.empty((pairs, 14 + L + 3 + L + 1), np.uint8)
    rec[:, :14] = name; rec[:, 14:14 + L] = seq; rec[:, 14 + L:14 + L + 3] = np.frombuffer(b"\n+\n", np.uint8); rec[:, 17 + L:17 + 2 * L] = qual; rec[:, -1] = 10
    return rec.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["trim", "plain"], default="trim")
    ap.add_argument("--runs", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1000000); ap.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "dart_trim_cache"))
    ap.add_argument("--out", default=None); ap.add_argument("--label", default="")
    a = ap.parse_args()
    os.makedirs(a.cache, exist_ok=True)
    prefix = os.path.join(a.cache, "idx")
    if not os.path.exists(prefix + ".ann"):
        index_build.build_index_from_genome(synth.make_genome([200000], seed=3, repeat_scale=20.0, n_introns=10), prefix)
    texts = []
    for tag in (1, 2):
        p = os.path.join(a.cache, "t%d_%d.npy" % (tag, a.pairs))
        if not os.path.exists(p):
            np.save(p, make_text(a.pairs, 100 + tag, tag))
        texts.append(np.load(p))
    t1, t2 = texts
    n = 2 * a.pairs
    gpu = host.DartGPU(host.Index(prefix), host.default_params(paired=1, max_mismatch=5))
    t = host.FastqText(); t.text1, t.n1, t.text2, t.n2, t.rc_odd_reads, t.max_reads = t1.ctypes.data, t1.size, t2.ctypes.data, t2.size, 1, n
    got = C.c_int(0); ms = C.c_float(0)

    def series(trimmed):
        fq, tr, stats = [], [], None
        for k in range(a.warmup + a.runs):
            rc = gpu.lib.dg_batch_upload_fastq(gpu.ctx, C.byref(t), C.byref(got))
            if rc or (not trimmed and got.value != n):
                raise RuntimeError("%d reads: %s" % (got.value, (gpu.lib.dg_last_error(gpu.ctx) or b"").decode()))
            gpu.lib.dg_batch_fastq_device_ms(gpu.ctx, C.byref(ms))
            if k >= a.warmup:
                fq.append(float(ms.value))
                if trimmed:
                    stats = gpu.trim_stats(); tr.append(gpu.trim_device_ms)
        return fq, tr, stats

    summ = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    res = {"mode": a.mode, "label": a.label, "reads": n, "runs": a.runs, "warmup": a.warmup, "text_bytes": int(t1.size + t2.size)}
    if a.mode == "trim":
        gpu.set_trim(adapter=b"AGATCGGAAGAGC", qual3=20, qual5=20, poly="GA", min_len=20, pairs=True)
        fq, tr, stats = series(True)
        res["trimmed_upload_fastq_device_ms"] = summ(fq); res["trim_kernels_device_ms"] = summ(tr)
        res["line_kernels_device_ms_median"] = round(statistics.median(fq) - statistics.median(tr), 4)
        res["trim_stats"] = dict(zip(host.TRIM_STAT_KEYS, stats))
        res["reads_per_s_through_trim_kernels"] = round(n / (statistics.median(tr) * 1e-3))
        gpu.set_trim(off=True)
    fq, _, _ = series(False)
    res["plain_upload_fastq_device_ms"] = summ(fq)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "a").write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
