"""Device time of the gene counts (dg_batch_accumulate_genes: k_gc_count + k_gc_top) beside the kernels of the batch they count (the sum of dg_last_timings,
unchanged code: the yardstick): 1 M pairs of 2x101 on the chr20-sized planted genome at -mis 5, the reads of the other rate probes, one batch, with a generated
annotation (tests/genecount_inputs.py::random_annotation, about half the genome covered) and with a skewed one (one gene over the first half of the chromosome,
so about half the units fall on one row).  Every run maps the batch again (a batch is counted once) and counts it; prints median, min and max of --runs runs
behind --warmup.  With --dart the host program runs end to end with and without DART_GENE_COUNTS.  A tool, not a test.

    python profiles/probes/gene_count_rate.py [--runs 10] [--warmup 2] [--pairs 1000000] [--cache DIR] [--out profiles/genecount/gene_count_rate.json]
    python profiles/probes/gene_count_rate.py --dart [--out profiles/genecount/dart_end_to_end.json]
    python profiles/probes/gene_count_rate.py --resources profiles/genecount/resource_usage.txt      (cross-compiles dg_genecount.h; needs no device)
"""
import argparse, json, os, random, re, shutil, statistics, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def resource_table(path):
    """registers, scratch, occupancy and LDS of every kernel of dg_genecount.h, as the compiler reports them for gfx950"""
    import __graft_entry__ as ge
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "gc.hip")
        open(src, "w").write('#include "%s"\n' % os.path.join(ROOT, "dart_amd", "csrc", "dg_genecount.h"))
        r = subprocess.run([ge.HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(d, "gc.o")],
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
            cur = dict(name=name) if name.startswith("k_gc_") else None
            if cur is not None:
                rows.append(cur)
        elif cur is not None:
            cur[k] = v
    cols = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch/B"), ("SGPRs Spill", "SGPRsp"), ("VGPRs Spill", "VGPRsp"),
            ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "LDS/B"), ("Dynamic Stack", "dyn.stack"))
    out = ["# hipcc -O3 --offload-arch=gfx950 -std=c++17 -Rpass-analysis=kernel-resource-usage over dart_amd/csrc/dg_genecount.h (cross-compiled; no device needed)",
           "%-18s" % "kernel" + "".join("%10s" % c for _, c in cols)]
    out += ["%-18s" % r_["name"] + "".join("%10s" % r_.get(k, "?") for k, _ in cols) for r_ in rows]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(out) + "\n")
    assert rows and all(r_.get("ScratchSize [bytes/lane]") == "0" for r_ in rows), "a kernel of dg_genecount.h uses scratch"


def annotations(g):
    """-> {name: (n_genes, exons)}: the generated one, and the skewed one (its genes of the chromosome's second half, and one gene over the first half)"""
    import genecount_inputs as gci
    lengths = [int(x) for x in g.lengths]
    n_genes, exons = gci.random_annotation(random.Random(1), lengths)
    half = lengths[0] // 2
    keep = [e for e in exons if not (e[0] == 0 and e[1] < half)]
    skew = keep + [(0, 0, half, 0, n_genes)]
    return {"generated": (n_genes, exons), "skewed": (n_genes + 1, skew)}


def stat(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def rate(a):
    import bench
    from dart_amd import host, synth
    prefix, g = bench.prepare_index(a.cache, bench.CHR20_LEN, 0, lambda: None)
    m1, m2 = synth.make_reads(g, a.pairs, rlen=101, seed=1000, sub_rate=0.01, indel_frac=0.02, n_frac=0.002)
    reads = host.interleave_pairs(m1, m2)
    n = 2 * a.pairs
    gpu = host.DartGPU(host.Index(prefix), host.default_params(paired=1, max_mismatch=5))
    gpu.upload(*host.pack_reads(reads))
    res = dict(what="device time of dg_batch_accumulate_genes beside the kernels of the batch it counts (sum of dg_last_timings), one batch, one MI355X", reads=n, units=a.pairs,
               runs=a.runs, warmup=a.warmup, min_mapq=4)
    for name, (n_genes, exons) in annotations(g).items():
        n_seg = gpu.gene_set_annotation(n_genes, exons)
        gpu.gene_reset()
        acc, batch, wall = [], [], []
        for r in range(a.warmup + a.runs):
            gpu.run()
            w0 = time.perf_counter()
            units = gpu.accumulate_genes(n, 4)
            counts = gpu.gene_counts()                      # (waits for the stream: the device time is read behind it)
            w1 = time.perf_counter()
            if r >= a.warmup:
                acc.append(gpu.gene_device_ms); batch.append(sum(ms for _, ms in gpu.timings())); wall.append((w1 - w0) * 1e3)
        assert units == a.pairs and int(counts[:, 0].sum()) == (a.warmup + a.runs) * a.pairs
        one = counts // (a.warmup + a.runs)
        top = int(one[4:, 0].max())
        res[name] = dict(genes=n_genes, exons=len(exons), segments=n_seg, accumulate_device_ms=stat(acc), batch_kernels_ms=stat(batch), accumulate_and_download_wall_ms=stat(wall),
                         accumulate_over_batch=round(statistics.median(acc) / statistics.median(batch), 5), units_per_s=round(a.pairs / (statistics.median(acc) * 1e-3)),
                         per_batch=dict(unmapped=int(one[0, 0]), multimapping=int(one[1, 0]), nofeature=int(one[2, 0]), ambiguous=int(one[3, 0]), counted=int(one[4:, 0].sum()), largest_gene_row=top,
                                        genes_with_counts=int((one[4:, 0] > 0).sum())))
    gpu.close()
    return res


def dart(a):
    """`dart` end to end, process start to exit, with and without DART_GENE_COUNTS: a warm-up run, two runs without (their difference is the run-to-run spread), one with"""
    import bench
    import genecount_inputs as gci
    from dart_amd import synth
    prefix, g = bench.prepare_index(a.cache, bench.CHR20_LEN, 0, lambda: None)
    m1, m2 = synth.make_reads(g, a.pairs, rlen=101, seed=1000, sub_rate=0.01, indel_frac=0.02, n_frac=0.002)
    d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    synth.write_fastq_fast(os.path.join(d, "1.fq"), m1, 1); synth.write_fastq_fast(os.path.join(d, "2.fq"), m2, 2)
    n_genes, exons = annotations(g)["generated"]
    gci.write_gtf(os.path.join(d, "ann.gtf"), exons, g.names)
    exe = os.path.join(ROOT, "dart_amd", "dart")
    def run(tag, extra):
        env = dict(os.environ, DART_TIMING="1", **extra)
        t0 = time.perf_counter()
        r = subprocess.run([exe, "-i", prefix, "-f", "1.fq", "-f2", "2.fq", "-o", tag + ".sam", "-j", tag + ".j", "-t", "16", "-mis", "5"], cwd=d, env=env, capture_output=True, text=True)
        wall = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-500:]
        if tag not in ("a", "c"):
            os.remove(os.path.join(d, tag + ".sam"))
        return wall, [l for l in r.stderr.splitlines() if l.startswith("[dart genes]")]
    warm, _ = run("w", {})
    b1, _ = run("a", {})
    b2, _ = run("b", {})
    with_s, note = run("c", {"DART_GENE_COUNTS": "ann.gtf"})
    same = open(os.path.join(d, "a.sam"), "rb").read() == open(os.path.join(d, "c.sam"), "rb").read()
    res = dict(what="dart end to end, process start to exit: 1 M pairs 2x101 (the probe's reads, seed 1000) as two FASTQ files on tmpfs against the chr20-sized planted genome's index, "
                     "-o out.sam -j out.j -t 16 -mis 5, one MI355X; one run each, in this order: a warm-up run, without, without again (the baseline's run-to-run spread), with DART_GENE_COUNTS",
                pairs=a.pairs, genes=n_genes, exons=len(exons), gtf_bytes=os.path.getsize(os.path.join(d, "ann.gtf")), warm_up_wall_s=round(warm, 3), without_wall_s=[round(b1, 3), round(b2, 3)],
                with_wall_s=round(with_s, 3), sam_identical=same, table_bytes=os.path.getsize(os.path.join(d, "c.sam.genes.tab")), genes_note=note[0] if note else None)
    shutil.rmtree(d, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "dart_bench_cache")); ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None); ap.add_argument("--dart", action="store_true")
    a = ap.parse_args()
    if a.resources:
        resource_table(a.resources)
        return
    line = json.dumps(dart(a) if a.dart else rate(a))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
