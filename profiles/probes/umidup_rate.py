"""Device time of the UMI-aware duplicate marking (dg_bam_markdup_umi_finish) by stage, for max_edit 0 and 1, beside dg_bam_markdup_finish over the same sorted
array: the workload of markdup_rate.py (1 M pairs of 2x101 on the chr20-sized planted genome at -mis 5 in 4 batches, the first tenth of the pairs a second time,
qualities one lower) with an 8-letter UMI appended to every name; a copy carries its original's UMI.  A tool, not a test.  The three calls alternate inside every
run (plain, exact, edit1, the order rotating from run to run), so a drift of the clock meets all three alike; prints median, min and max of --runs runs behind
--warmup.  The plain call over the un-suffixed names is markdup_rate.py's own figure.

    python profiles/probes/umidup_rate.py [--runs 10] [--warmup 2] [--pairs 1000000] [--batches 4] [--cache DIR] [--out profiles/umidup/umidup_rate.json]
"""
import argparse, json, os, random, statistics, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STAGES = ("record_pass", "mate_sort_search", "pair_sorts", "end_sorts", "heads_groups_families", "clustering", "flag_writes", "count_emit")
STATS = ("examined", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "crowded_candidates", "flagged_records", "largest_cluster", "records_with_umi",
         "pair_families_of_several_groups", "absorbed_groups", "crowded_families")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1000000); ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "dart_bench_cache")); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import markdup_rate
    from dart_amd import host
    prefix, m1, m2, extra = markdup_rate.the_reads(a)
    reads = host.interleave_pairs(m1, m2)
    n = len(reads)
    rng = random.Random(8)
    umi = [bytes(rng.choice(b"ACGT") for _ in range(8)) for _ in range(a.pairs)]
    gpu = host.DartGPU(host.Index(prefix), host.default_params(paired=1, max_mismatch=5))
    ids = [(b"r%09d_" % (i // 2) + umi[i // 2]) if i < 2 * a.pairs else (b"c%09d_" % (i // 2 - a.pairs) + umi[i // 2 - a.pairs]) for i in range(n)]
    quals = [b"I" * 101] * (2 * a.pairs) + [b"H" * 101] * (2 * extra)
    cuts = [(n * k // a.batches) & ~1 for k in range(a.batches)] + [n]
    for k in range(a.batches):
        lo, hi = cuts[k], cuts[k + 1]
        so, rl, flat = host.pack_reads(reads[lo:hi])
        gpu.map_batch(so, rl, flat)
        gpu.format_bam(ids[lo:hi], quals[lo:hi], hi - lo, raw=True)
        gpu.accumulate_bam(k)
    n_rec, nb = gpu.bam_sort_finish()
    kinds = ("plain", "exact", "edit1")
    t = {"%s_device_ms" % k: [] for k in kinds}
    t.update({"%s_wall_ms" % k: [] for k in kinds})
    t.update({"%s_%s_ms" % (k, s): [] for k in kinds[1:] for s in STAGES})
    stats, passes = {}, {}
    for r in range(a.warmup + a.runs):
        for j in range(3):
            kind = kinds[(r + j) % 3]
            w0 = time.perf_counter()
            if kind == "plain":
                stats[kind] = gpu.bam_markdup_finish(); dev, passes[kind], split = gpu.bam_markdup_device_ms, gpu.bam_markdup_passes, ()
            else:
                stats[kind] = gpu.bam_markdup_umi_finish(max_edit=1 if kind == "edit1" else 0)
                dev, passes[kind], split = gpu.bam_markdup_umi_device_ms, gpu.bam_markdup_umi_passes, gpu.bam_markdup_umi_device_ms_split
            w1 = time.perf_counter()
            if r >= a.warmup:
                t["%s_device_ms" % kind].append(dev); t["%s_wall_ms" % kind].append((w1 - w0) * 1e3)
                for s, v in zip(STAGES, split):
                    t["%s_%s_ms" % (kind, s)].append(v)
    stat = lambda v: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = dict(reads=n, batches=a.batches, runs=a.runs, warmup=a.warmup, records=n_rec, raw_bytes=nb, umi_letters=8, sort_passes=passes,
               plain_stats=dict(zip(STATS[:8], stats["plain"])), exact_stats=dict(zip(STATS, stats["exact"])), edit1_stats=dict(zip(STATS, stats["edit1"])),
               **{k: stat(v) for k, v in t.items()},
               exact_over_plain_device=round(med["exact_device_ms"] / med["plain_device_ms"], 4), edit1_over_plain_device=round(med["edit1_device_ms"] / med["plain_device_ms"], 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
