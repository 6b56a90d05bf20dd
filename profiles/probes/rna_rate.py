"""Device and wall time of the RNA-seq metrics (dg_bam_rna_finish: the class pass, lane = record; the event path of the coverage track under the stage's filter;
the body pass, a wave = transcript) beside the coverage track's counting walk (k_cv_count, lane = record over the same heads and CIGARs without the look-up: the
yardstick), the whole coverage track, the QC's per-record tables and the BGZF kernels, all over the same sorted array in the same run: 1 M pairs of 2x101 on the
chr20-sized planted genome at -mis 5, the reads and batches of bam_sort_rate.py, against a seeded random annotation of GRCh38's density (about 20 genes and 80
transcripts a megabase, seven exons a transcript, spans that cover two fifths of the sequence).  A tool, not a test.  Device time from events; prints median, min and
max of --runs runs behind --warmup.

    python profiles/probes/rna_rate.py [--runs 10] [--warmup 2] [--pairs 1000000] [--batches 4] [--cache DIR] [--out profiles/rnametrics/rna_rate.json]
    python profiles/probes/rna_rate.py --resources profiles/rnametrics/resource_usage.txt      (cross-compiles dg_rnametrics.h; needs no device)
"""
import argparse, json, os, random, re, statistics, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BLOCK = 0xFF00
PARTS = ("class_pass", "events_and_sort", "body_pass")


def resource_table(path):
    """registers, scratch, occupancy and LDS of every kernel of dg_rnametrics.h, as the compiler reports them for gfx950"""
    import __graft_entry__ as ge
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "rm.hip")
        open(src, "w").write('#include "%s"\n' % os.path.join(ROOT, "dart_amd", "csrc", "dg_rnametrics.h"))
        r = subprocess.run([ge.HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-c", "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", src,
                            "-o", os.path.join(d, "rm.o")], capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            m = re.match(r"_Z(\d+)", v)                       # _Z<length><name><parameters>
            name = v[len(m.group(0)):len(m.group(0)) + int(m.group(1))] if m else v
            cur = dict(name=name) if name.startswith("k_rm_") else None      # (the header includes the coverage track's, the sorter's and the formatter's kernels)
            if cur is not None:
                rows.append(cur)
        elif cur is not None:
            cur[k] = v
    cols = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch/B"), ("SGPRs Spill", "SGPRsp"), ("VGPRs Spill", "VGPRsp"),
            ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "LDS/B"), ("Dynamic Stack", "dyn.stack"))
    out = ["# hipcc -O3 --offload-arch=gfx950 -std=c++17 -Rpass-analysis=kernel-resource-usage over dart_amd/csrc/dg_rnametrics.h (cross-compiled; no device needed)",
           "%-18s" % "kernel" + "".join("%10s" % c for _, c in cols)]
    out += ["%-18s" % r_["name"] + "".join("%10s" % r_.get(k, "?") for k, _ in cols) for r_ in rows]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(out) + "\n")
    assert len(rows) == 4 and all(r_.get("ScratchSize [bytes/lane]") == "0" and r_.get("VGPRs Spill") == "0" and r_.get("SGPRs Spill") == "0" for r_ in rows), "a kernel of dg_rnametrics.h uses scratch or spills"


def annotation(lengths, seed=17, genes_per_mb=20.0, tx_per_gene=4):
    """-> (RNA_TX array, RNA_EXON array): genes of 4 .. 20 exons of 50 .. 400 bases over spans of 5 .. 100 kb, either strand, neighbours overlapping now and then;
    a gene's transcripts are subsets of its exons with a CDS that leaves the outer exons' halves as UTR; one gene in fifty is ribosomal"""
    import numpy as np
    from dart_amd import host
    rng = random.Random(seed)
    tx, ex = [], []
    for c, L in enumerate(lengths):
        L = int(L)
        at = rng.randrange(1000, 20000)
        step = 1e6 / genes_per_mb
        while at < L - 120000:
            span = int(min(100000, max(5000, rng.lognormvariate(10.1, 0.8))))
            n_ex = rng.randrange(4, 21)
            starts = sorted(rng.randrange(at, at + span) for _ in range(n_ex))
            exons = [(s, s + rng.randrange(50, 401)) for s in starts]
            strand, ribo = rng.randrange(2), rng.random() < 0.02
            for _ in range(tx_per_gene):
                mine = sorted(rng.sample(exons, rng.randrange(2, n_ex + 1)))
                lo, hi = mine[0][0], max(e for s, e in mine)
                cds = (0, 0) if rng.random() < 0.2 else (lo + (mine[0][1] - lo) // 2, hi - 25)
                tx.append((c, strand, 1 if ribo else 0, cds[0], cds[1], len(mine), len(ex)))
                ex += mine
            at += int(rng.expovariate(1.0 / step)) + (0 if rng.random() < 0.2 else span // 3)
    return np.array(tx, host.RNA_TX), np.array(ex, host.RNA_EXON)


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
    import bench
    from dart_amd import host, synth
    prefix, g = bench.prepare_index(a.cache, bench.CHR20_LEN, 0, lambda: None)
    m1, m2 = synth.make_reads(g, a.pairs, rlen=101, seed=1000, sub_rate=0.01, indel_frac=0.02, n_frac=0.002)
    reads = host.interleave_pairs(m1, m2)
    n = 2 * a.pairs
    ix = host.Index(prefix)
    gpu = host.DartGPU(ix, host.default_params(paired=1, max_mismatch=5))
    tx, ex = annotation(ix.chr_len)
    n_seg, n_elig = gpu.rna_set_annotation(tx, ex)
    ids = [("r%09d" % (i // 2)).encode() for i in range(n)]
    quals = [b"I" * 101] * n
    cuts = [(n * k // a.batches) & ~1 for k in range(a.batches)] + [n]
    for k in range(a.batches):
        lo, hi = cuts[k], cuts[k + 1]
        so, rl, flat = host.pack_reads(reads[lo:hi])
        gpu.map_batch(so, rl, flat)
        gpu.format_bam(ids[lo:hi], quals[lo:hi], hi - lo, raw=True)
        gpu.accumulate_bam(k)
    names = ("sort_finish_device_ms", "bgzf_device_ms", "coverage_device_ms", "coverage_count_walk_ms", "coverage_emit_ms", "coverage_sort_ms", "qc_record_tables_ms", "rna_device_ms", "rna_wall_ms")
    t = {k: [] for k in names + tuple("rna_%s_ms" % s for s in PARTS)}
    for r in range(a.warmup + a.runs):
        n_rec, nb = gpu.bam_sort_finish()
        z_ms = 0.0
        for off in range(0, nb, 4096 * BLOCK):
            gpu.bam_sort_compress(off, min(4096 * BLOCK, nb - off))
            z_ms += gpu.bam_device_ms
        gpu.bam_coverage_finish(0x904, 0, entries_only=True)  # (the stage's own default filter, so both walk the same records)
        cov, cov_split = gpu.bam_coverage_device_ms, gpu.bam_coverage_device_ms_split
        gpu.bam_qc_finish()
        qc_flag = gpu.bam_qc_device_ms_split[0]
        w0 = time.perf_counter()
        v = gpu.bam_rna_finish()                              # (the wall time holds the download too)
        w1 = time.perf_counter()
        if r >= a.warmup:
            for k, x in zip(names, (gpu.bam_sort_device_ms, z_ms, cov, cov_split[0], cov_split[1], cov_split[2], qc_flag, gpu.bam_rna_device_ms, (w1 - w0) * 1e3)):
                t[k].append(x)
            for s, x in zip(PARTS, gpu.bam_rna_device_ms_split):
                t["rna_%s_ms" % s].append(x)
    stat = lambda x: dict(median=round(statistics.median(x), 4), min=round(min(x), 4), max=round(max(x), 4))
    med = {k: statistics.median(x) for k, x in t.items()}
    ratio = lambda p, q: round(med[p] / med[q], 4) if med[q] else None
    gbs = lambda ms: round(nb / (ms * 1e-3) / 1e9, 2) if ms else None
    res = dict(reads=n, batches=a.batches, runs=a.runs, warmup=a.warmup, records=n_rec, raw_bytes=nb, words=len(v["words"]), text_bytes=len(gpu.bam_rna_text(v)), granules=gpu.bam_rna_granules(),
               annotation=dict(transcripts=len(tx), exons=len(ex), segments=n_seg, eligible=n_elig, chromosome_bases=int(sum(int(x) for x in ix.chr_len))),
               sn=dict(zip(("records", "counted", "blocks", "aligned_bases", "transcripts", "eligible_transcripts", "contributing_transcripts", "segments"), [int(x) for x in v["SN"][:8]])),
               ba=[int(x) for x in v["BA"]], rc=[int(x) for x in v["RC"]], st=[int(x) for x in v["ST"]],
               **{k: stat(x) for k, x in t.items()},
               array_gb_per_s=dict(rna_class_pass_lane_per_record=gbs(med["rna_class_pass_ms"]), coverage_counting_walk_lane_per_record=gbs(med["coverage_count_walk_ms"]),
                                   qc_record_tables_lane_per_record=gbs(med["qc_record_tables_ms"])),
               class_pass_over_coverage_counting_walk=ratio("rna_class_pass_ms", "coverage_count_walk_ms"),
               rna_events_and_sort_over_coverage_count_emit_sort=round(med["rna_events_and_sort_ms"] / (med["coverage_count_walk_ms"] + med["coverage_emit_ms"] + med["coverage_sort_ms"]), 4),
               rna_over_bgzf_device=ratio("rna_device_ms", "bgzf_device_ms"))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
