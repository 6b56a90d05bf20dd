"""GPU suite (-m gpu): genomes of 32 b to 130 kb (tests/small_genome_inputs.py), the sizes a phage, plasmid, mitochondrion or amplicon job has and
no other GPU test maps against.  The index builder against the bytes the reference's indexer wrote (tests/golden/small_genomes.json); every record,
CIGAR op, junction tuple and reference-equivalent counter of every run against the oracle, which tests/test_small_genomes_oracle.py pins on the
reference at these sizes; the prefix table's K at the seams 4^8 and 4^9; the index aids switched off or sampled and the three seeding kernels; the
start-up paths; FASTQ text in and SAM text out on the device."""
import json, os, re
import numpy as np
import pytest
import common, oracle_py
import small_genome_inputs as sgi
import sam_device_inputs as sdi
from test_gpu_index import _select
from dart_amd import host, index_build

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(common.GOLDEN, "small_genomes.json")))
AID_GENOMES = ("g32", "g129", "g32768", "c5")
TEXT_GENOMES = ("c5", "g5386")
# the GPU's counter -> the oracle's (occ_blocks is a lower bound by design and stays out)
COUNTERS = (("steps", "n_2occ4"), ("lf_steps", "n_lf"), ("sa_lookups", "n_sa"), ("nw_calls", "n_nw"), ("nw_cells", "nw_cells"),
            ("reseed_calls", "n_reseed"), ("reseed_window", "reseed_window"))


def _index_is_recorded(name, prefix, what):
    for ext, want in GOLD["genomes"][name]["index_sha256"].items():
        assert common.sha(prefix + "." + ext) == want, "GPU-built .%s differs from the reference bwt_index output (%s, %s)" % (ext, name, what)


@pytest.fixture(scope="module")
def small(workdir):
    """name -> dict(prefix, ix, orc, want): the genome's index built by the default builder (and checked against the reference's bytes, so no test
    here compares two consumers of a wrong index), the oracle on it, and the oracle's records and counters of every run, computed once"""
    made = {}

    def get(name):
        if name not in made:
            assert sgi.codes_sha256(name) == GOLD["genomes"][name]["codes_sha256"], "the genome generator drifted from the recorded inputs"
            prefix = os.path.join(workdir, "smallgpu_" + name)
            index_build.build_index_from_genome(sgi.make_genome(name), prefix)
            _index_is_recorded(name, prefix, "default builder")
            orc = oracle_py.Oracle(prefix)
            want = {}
            for key, paired, flags in sgi.runs(name):
                p, h = common.parse_flags(flags)
                b = sgi.batch(name, paired)
                rec = orc.map_batch(orc.params(paired=int(paired), **p), *b)
                want[key] = dict(paired=paired, p=p, h=h, batch=b, rec=rec, ctr=dict(orc.counters))
                assert int((rec[0]["score"] > 0).sum()) == GOLD["runs"][key]["n_mapped"] and len(rec[3]) == GOLD["runs"][key]["n_junction_tuples"], key
            made[name] = dict(prefix=prefix, ix=host.Index(prefix), orc=orc, want=want)
        return made[name]
    yield get
    for v in made.values():
        v["orc"].close()


def _packed(name, paired):
    """the run's ragged reads as dg_map_batch_packed takes them: 2 bits per base in words of the longest read's width, N listed, the lengths beside them"""
    seqs = sgi.stored_pairs(*sgi.paired_reads(name)) if paired else sgi.single_reads(name)
    lens = np.asarray([len(s) for s in seqs], np.uint16)
    arr = np.full((len(seqs), int(lens.max())), ord("A"), np.uint8)
    for i, s in enumerate(seqs):
        arr[i, :len(s)] = np.frombuffer(s, np.uint8)
    words, nlist = host.pack_reads_2bit(arr)
    return words, nlist, lens


@pytest.mark.parametrize("sorter", ["hip", "hip-python", "plain", "bucketed"])
@pytest.mark.parametrize("name", sgi.NAMES)
def test_gpu_index_builder_writes_the_reference_indexers_files_for_small_genomes(name, sorter, workdir, monkeypatch):
    """di_build_files (hip), the same kernels driven from index_build.py (hip-python) and the two torch-orchestrated sorters: one tile, empty two-symbol
    buckets, N = 4095 / 4097, a text of one Occ block -- none of them refuses a size from 32 bases on, and all write the reference's five files"""
    _select(sorter, monkeypatch)
    prefix = os.path.join(workdir, "smallidx_%s_%s" % (name, sorter))
    index_build.build_index_from_genome(sgi.make_genome(name), prefix, device="cuda")
    _index_is_recorded(name, prefix, sorter + " sorter")


@pytest.mark.parametrize("name", sgi.NAMES)
def test_gpu_records_and_counters_match_oracle_on_small_genome(name, small):
    s = small(name)
    gpu = host.DartGPU(s["ix"])
    try:
        gpu.wait_index()
        K = int(re.search(r"K=(\d+) table", gpu.init_report()).group(1))
        assert K == sgi.expected_k(name) == GOLD["genomes"][name]["K"], gpu.init_report()
        for key, w in s["want"].items():
            gpu.set_params(host.default_params(paired=int(w["paired"]), **w["p"]))
            common.assert_same(gpu.map_batch(*w["batch"]), w["rec"])
            c = gpu.counters()
            for mine, theirs in COUNTERS:
                assert c[mine] == w["ctr"][theirs], (key, mine, c[mine], w["ctr"][theirs])
            assert c["reruns_scan_total"] == 0, key
            if sgi.l_pac(name) >= sgi.LONG_GAP_MIN:
                assert c["reseed_calls"] > 0 and len(w["rec"][3]) > 0, key
            # the reads hold A, C, G, T and N only: the packed entry and both compact forms too
            words, nlist, lens = _packed(name, w["paired"])
            common.assert_same(gpu.map_batch_packed(words, nlist, 0, rlen=lens), w["rec"])
            common.assert_same(gpu.download_compact(), w["rec"])
            common.assert_same(gpu.map_batch_compact(words, nlist, 0, rlen=lens), w["rec"])
    finally:
        gpu.close()


def _runs_for_switches(s, name):
    return [k for k in s["want"] if k.endswith("e: -mis 5")]


@pytest.mark.parametrize("name", AID_GENOMES)
def test_gpu_index_aids_and_seeding_kernels_on_small_genome(name, small, monkeypatch):
    """no prefix table, no dense suffix array, every 4th row of it -- each with the lane-per-read kernel, the phased queue kernel and the queue kernel
    without few-row comparisons: the oracle's records, and the reference-equivalent seeding counters of the default configuration"""
    s = small(name)
    keys = _runs_for_switches(s, name)
    base = {}
    gpu = host.DartGPU(s["ix"])
    for key in keys:
        w = s["want"][key]
        gpu.set_params(host.default_params(paired=int(w["paired"]), **w["p"]))
        common.assert_same(gpu.map_batch(*w["batch"]), w["rec"])
        base[key] = gpu.counters()
    gpu.close()
    for aid, aid_value in (("DG_KTAB_K", "0"), ("DG_SA_DENSE", "0"), ("DG_SA_DENSE", "4")):
        for kernel, kernel_value in (("DG_SEED_LEGACY", "1"), ("DG_SEED_PHASES", "1"), ("DG_SEED_MULTI", "0")):
            monkeypatch.setenv(aid, aid_value); monkeypatch.setenv(kernel, kernel_value)
            gpu = host.DartGPU(s["ix"])                  # (the aids are chosen when the index is loaded, the kernels at dg_set_params)
            try:
                for key in keys:
                    w = s["want"][key]
                    gpu.set_params(host.default_params(paired=int(w["paired"]), **w["p"]))
                    common.assert_same(gpu.map_batch(*w["batch"]), w["rec"])
                    c = gpu.counters()
                    for k in ("steps", "lf_steps", "sa_lookups", "seeds"):
                        assert c[k] == base[key][k], (key, k, aid, aid_value, kernel)
            finally:
                gpu.close()
                monkeypatch.delenv(aid); monkeypatch.delenv(kernel)


@pytest.mark.parametrize("name", AID_GENOMES)
def test_gpu_start_up_paths_on_small_genome(name, small):
    """the index as host arrays, the index files straight to HBM, and the aids built beside the first batches: the same records and seeding counters"""
    s = small(name)
    keys = _runs_for_switches(s, name)
    base = None
    for kw in (dict(from_files=False), dict(from_files=True), dict(from_files=True, async_aids=True)):
        gpu = host.DartGPU(s["ix"], **kw)
        try:
            for waited in (False, True):                 # (with async_aids the first batches may run without the aids)
                got = {}
                for key in keys:
                    w = s["want"][key]
                    gpu.set_params(host.default_params(paired=int(w["paired"]), **w["p"]))
                    common.assert_same(gpu.map_batch(*w["batch"]), w["rec"])
                    c = gpu.counters()
                    got[key] = {k: c[k] for k in ("steps", "lf_steps", "sa_lookups", "seeds")}
                if base is None: base = got
                assert got == base, (kw, waited)
                gpu.wait_index()
            assert ("host arrays" in gpu.init_report()) == (not kw["from_files"]), gpu.init_report()
        finally:
            gpu.close()


@pytest.mark.parametrize("name", TEXT_GENOMES)
def test_gpu_fastq_in_and_sam_out_on_small_genome(name, small, workdir):
    """upload_fastq of the reads written as FASTQ is the host packer's batch; format_sam and format_sam_resident are sam.format_records of the
    oracle's records: 1-based positions on 33-base contigs, mate fields across contigs, '*' records"""
    s = small(name)
    d = os.path.join(workdir, "smalltext_" + name)
    sgi.write_inputs(name, d)
    gpu = host.DartGPU(s["ix"])
    try:
        for key, w in s["want"].items():
            paired = w["paired"]
            seqs = sgi.stored_pairs(*sgi.paired_reads(name)) if paired else sgi.single_reads(name)
            n = len(seqs)
            headers = [b"r%d" % (i // 2 if paired else i) for i in range(n)]
            quals = [b"I" * len(x) for x in seqs]
            t1 = open(os.path.join(d, "p1.fq" if paired else "a.fq"), "rb").read()
            t2 = open(os.path.join(d, "p2.fq"), "rb").read() if paired else None
            gpu.set_params(host.default_params(paired=int(paired), **w["p"]))
            assert gpu.upload_fastq(t1, t2, rc_odd_reads=paired) == n
            so, rl, flat = w["batch"]
            gso, grl, gflat, names, gquals = gpu.download_reads()
            assert np.array_equal(gso, so) and np.array_equal(grl, rl) and np.array_equal(gflat, flat.reshape(-1))
            assert names == headers and gquals == quals
            gpu.run()
            common.assert_same(gpu.download(), w["rec"])
            reads, rep, cig, sj = w["rec"]
            npm = n if paired else 0
            twin, st = sdi.twin_text(headers, seqs, quals, reads, rep, cig, s["ix"].names, npm, multi=bool(w["p"]["multi_hit"]), unique=w["h"]["unique"])
            assert b"\t*\t0\t0\t*\t" in twin                 # (the all-N reads at least are '*' records)
            text, ct = gpu.format_sam_resident(npm, unique_only=w["h"]["unique"])
            assert text == twin, common.first_diff(text.decode("latin1"), twin.decode("latin1"))
            assert ct == dict(unmapped=st.unmapped, unique=st.unique, paired=st.paired)
            text2, ct2 = gpu.format_sam(headers, quals, npm, unique_only=w["h"]["unique"])
            assert text2 == twin and ct2 == ct
            gpu.map_batch(so, rl, flat)                  # and the host-array formatter behind a plain upload
            text3, ct3 = gpu.format_sam(headers, quals, npm, unique_only=w["h"]["unique"])
            assert text3 == twin and ct3 == ct
    finally:
        gpu.close()
