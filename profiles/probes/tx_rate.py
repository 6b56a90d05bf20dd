"""Device time of the expression stage (dg_batch_accumulate_tx: the compatibility passes k_tx_count + k_tx_top + k_tx_write, and the class building; dg_tx_finish:
the EM) beside its yardsticks, every figure over the same batch in the same run: 1 M pairs of 2x101 on the chr20-sized planted genome at -mis 5, the reads of the
other rate probes, one batch; a generated annotation (tests/genecount_inputs.py::random_annotation's genes, each as a locus of three isoforms: full, one exon
skipped, one intron retained).
  compatibility passes   against dg_batch_accumulate_genes over the same batch, with the same transcripts' exons as genes: the same heads, reports and CIGARs with
                         one look-up
  class building         against one rs_sort_passes (dg_probe_sort_passes: 64 key bits, histograms allocated beforehand) over as many pairs as the build sorts
                         (the counted units; the table is empty: every run begins behind dg_tx_reset); beside it one dg_sort_pairs, the call the index builder
                         makes, which allocates and frees its histograms inside the figure
  EM                     one round (the time of a 16-round call over 16) and the rounds to convergence
Device time from events; every run maps the batch again (a batch is counted once); prints median, min and max of --runs runs behind --warmup.  A tool, not a test.

    python profiles/probes/tx_rate.py [--runs 10] [--warmup 2] [--pairs 1000000] [--cache DIR] [--out profiles/txquant/tx_rate.json]
    python profiles/probes/tx_rate.py --resources profiles/txquant/resource_usage.txt      (cross-compiles dg_txquant.h; needs no device)
"""
import argparse, json, os, random, re, statistics, subprocess, sys, tempfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def resource_table(path):
    """registers, scratch, occupancy and LDS of every kernel of dg_txquant.h, as the compiler reports them for gfx950"""
    import __graft_entry__ as ge
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "tx.hip")
        open(src, "w").write('#include "%s"\n' % os.path.join(ROOT, "dart_amd", "csrc", "dg_txquant.h"))
        r = subprocess.run([ge.HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(d, "tx.o")],
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
            cur = dict(name=name) if name.startswith("k_tx_") else None
            if cur is not None:
                rows.append(cur)
        elif cur is not None:
            cur[k] = v
    cols = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch/B"), ("SGPRs Spill", "SGPRsp"), ("VGPRs Spill", "VGPRsp"),
            ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "LDS/B"), ("Dynamic Stack", "dyn.stack"))
    out = ["# hipcc -O3 --offload-arch=gfx950 -std=c++17 -Rpass-analysis=kernel-resource-usage over dart_amd/csrc/dg_txquant.h (cross-compiled; no device needed)",
           "# SGPRsp: scalar registers kept in lanes of a vector register, not in memory; scratch/B is what would be memory",
           "%-18s" % "kernel" + "".join("%10s" % c for _, c in cols)]
    out += ["%-18s" % r_["name"] + "".join("%10s" % r_.get(k, "?") for k, _ in cols) for r_ in rows]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(out) + "\n")
    assert rows and all(r_.get("ScratchSize [bytes/lane]") == "0" for r_ in rows), "a kernel of dg_txquant.h uses scratch"


def annotation(g):
    """-> (transcripts, gene exons): every gene of the generated annotation as a locus of up to three isoforms; the same exons with the transcript as their gene"""
    import genecount_inputs as gci
    import txquant_inputs as txi
    rng = random.Random(1)
    n_genes, exons = gci.random_annotation(rng, [int(x) for x in g.lengths])
    by_gene = {}
    for c, s, e, st, gene in exons:
        by_gene.setdefault(gene, (c, st, set()))[2].add((s, e))
    tr = []
    for gene in sorted(by_gene):
        c, st, ex = by_gene[gene]
        tr += txi.locus_isoforms(c, st, txi.merged(ex), rng)
    gene_exons = [(c, s, e, st, t) for t, (c, st, ex) in enumerate(tr) for s, e in ex]
    return tr, gene_exons


def stat(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def rate(a):
    import torch
    import bench
    import txquant_inputs as txi
    from dart_amd import host, synth
    prefix, g = bench.prepare_index(a.cache, bench.CHR20_LEN, 0, lambda: None)
    m1, m2 = synth.make_reads(g, a.pairs, rlen=101, seed=1000, sub_rate=0.01, indel_frac=0.02, n_frac=0.002)
    reads = host.interleave_pairs(m1, m2)
    n = 2 * a.pairs
    gpu = host.DartGPU(host.Index(prefix), host.default_params(paired=1, max_mismatch=5))
    gpu.upload(*host.pack_reads(reads))
    tr, gene_exons = annotation(g)
    tx, ex = txi.annot_arrays(tr)
    n_merged, n_seg = gpu.tx_set_annotation(tx, ex)
    gpu.gene_set_annotation(len(tr), gene_exons)
    compat, build, genes, batch = [], [], [], []
    for r in range(a.warmup + a.runs):
        gpu.run()
        gpu.gene_reset(); gpu.tx_reset()
        gpu.accumulate_genes(n, 4); gpu.gene_counts()
        units = gpu.accumulate_tx(n, 4, 0)
        off, ids, cnt, words = gpu.tx_classes()
        if r >= a.warmup:
            compat.append(gpu.tx_device_ms_split[0]); build.append(gpu.tx_device_ms_split[1]); genes.append(gpu.gene_device_ms); batch.append(sum(ms for _, ms in gpu.timings()))
    assert units == a.pairs and int(words[0]) == a.pairs
    counted = int(words[4])
    # the yardstick of the class building: one sort of as many pairs, 64 key bits
    k = torch.randint(0, 2 ** 62, (counted,), dtype=torch.int64, device="cuda"); v = torch.arange(counted, dtype=torch.int64, device="cuda")
    kt, vt = torch.empty_like(k), torch.empty_like(v)
    sort, passes = [], []
    import ctypes as C
    gpu.lib.dg_sort_pairs.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]      # (without them ctypes passes the pointers as 32-bit ints)
    gpu.lib.dg_sort_pairs.restype = C.c_int
    gpu.lib.dg_probe_sort_passes.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    gpu.lib.dg_probe_sort_passes.restype = C.c_int
    for r in range(a.warmup + a.runs):
        kk = k.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = gpu.lib.dg_sort_pairs(0, kk.data_ptr(), v.data_ptr(), kt.data_ptr(), vt.data_ptr(), counted, 64)
        e1.record(); e1.synchronize()
        assert rc == 0
        # rs_sort_passes alone: the histograms allocated in front of the first event, nothing copied back
        kk = k.clone(); torch.cuda.synchronize()
        ms = C.c_float(0)
        assert gpu.lib.dg_probe_sort_passes(0, kk.data_ptr(), v.data_ptr(), kt.data_ptr(), vt.data_ptr(), counted, 64, C.byref(ms), None) == 0
        if r >= a.warmup:
            sort.append(e0.elapsed_time(e1)); passes.append(float(ms.value))
    em16, emfull, rounds = [], [], 0
    for r in range(a.warmup + a.runs):
        gpu.tx_finish(200, 16); t16 = gpu.tx_em_device_ms
        fin = gpu.tx_finish(200, 1000); tf = gpu.tx_em_device_ms
        rounds = int(fin[len(tr) + 8])
        if r >= a.warmup:
            em16.append(t16 / 16); emfull.append(tf)
    res = dict(what="device time of the expression stage beside its yardsticks, one batch, one MI355X", reads=n, units=a.pairs, runs=a.runs, warmup=a.warmup, min_mapq=4,
               transcripts=len(tr), merged_exons=n_merged, segments=n_seg, words=[int(x) for x in words], classes=len(cnt), members=len(ids), largest_class=int(cnt.max()) if len(cnt) else 0,
               compatibility_ms=stat(compat), gene_count_ms=stat(genes), compatibility_over_gene_count=round(statistics.median(compat) / statistics.median(genes), 3),
               class_building_ms=stat(build), sort_of_as_many_pairs_ms=stat(sort), sorted_pairs=counted, class_building_over_sort=round(statistics.median(build) / statistics.median(sort), 3),
               sort_passes_alone_ms=stat(passes), class_building_over_sort_passes=round(statistics.median(build) / statistics.median(passes), 3),
               sort_yardstick="sort_passes_alone_ms is rs_sort_passes between two events with its histograms allocated beforehand (dg_probe_sort_passes): the yardstick. "
                              "sort_of_as_many_pairs_ms is one dg_sort_pairs call, which also allocates and frees its histograms and copies back when the passes end in the other buffer",
               longest_list=int(np.diff(off.astype(np.int64)).max()) if len(cnt) else 0,
               batch_kernels_ms=stat(batch), em_round_ms=stat(em16), em_to_convergence_ms=stat(emfull), em_rounds_to_convergence=rounds, em_converged=int(fin[len(tr) + 9]))
    gpu.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "dart_bench_cache")); ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    if a.resources:
        resource_table(a.resources)
        return
    line = json.dumps(rate(a))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
