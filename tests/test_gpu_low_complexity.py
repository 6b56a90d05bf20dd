"""GPU suite (-m gpu): low-complexity genomes of at most 64 kb (tests/low_complexity_inputs.py) -- homopolymers, microsatellites, a text that is its own
reverse complement, one contig three times, a ladder of copy counts around max_dup, the 128-row floor of k_seed_heavy_walk and 16 seeds per unit.  They
reach in seconds what only the GRCh38-sized run reached before: searches that restart base by base, intervals above max_dup, k_seed_heavy_walk +
k_seed_heavy, k_chain_heavy, the general report path, alignments and splice boundaries with many equally good answers, equal scores on several contigs;
and for the index builder texts whose ties run to their end.  The index builder against the bytes the reference's indexer wrote
(tests/golden/low_complexity.json); every record, CIGAR op, junction tuple and reference-equivalent counter of every run against the oracle, which
tests/test_low_complexity_oracle.py pins on the reference for these runs; the index aids off or sampled and the three seeding kernels; SAM text on the
device; `dart index` and `dart`.  The counters of the named paths are asserted, so a read set that stops reaching them fails here."""
import json, os, subprocess
import numpy as np
import pytest
import common, oracle_py
import low_complexity_inputs as lci
import sam_device_inputs as sdi
import test_low_complexity_oracle as tl
from test_gpu_index import _select
from dart_amd import host, index_build

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(common.GOLDEN, "low_complexity.json")))
DART = os.path.join(common.ROOT, "dart_amd", "dart")
AID_GENOMES = ("ladder", "dinuc")
TEXT_GENOMES = ("twins", "micro")
HEAVY_GENOMES = ("homopolymer", "dinuc", "micro", "ladder")          # where reads must be handed from k_seed_qf to k_seed_heavy
# the GPU's counter -> the oracle's (occ_blocks is a lower bound by design and stays out)
COUNTERS = (("steps", "n_2occ4"), ("lf_steps", "n_lf"), ("sa_lookups", "n_sa"), ("nw_calls", "n_nw"), ("nw_cells", "nw_cells"),
            ("reseed_calls", "n_reseed"), ("reseed_window", "reseed_window"))
# counters that must be positive, summed over the genome's runs in one context under default switches: the paths the genome is there for
# (wave_ticks_k_seed_heavy counts the ticks of an empty launch too: what shows the hand-over is test_gpu_reads_go_through_k_seed_heavy_...)
PATHS = {"wave_chained_units": ("ladder", "dinuc", "micro"), "general_path_units": ("twins", "dinuc"),
         "wave_ticks_k_seed_heavy": ("homopolymer", "dinuc", "micro"), "ktab_lookups": lci.NAMES}


def _index_is_recorded(name, prefix, what):
    for ext, want in GOLD["genomes"][name]["index_sha256"].items():
        assert common.sha(prefix + "." + ext) == want, "GPU-built .%s differs from the reference bwt_index output (%s, %s)" % (ext, name, what)


@pytest.fixture(scope="module")
def lowc(workdir):
    """name -> dict(prefix, ix, orc, want): the genome's index built by the default builder (and checked against the reference's bytes, so no test
    here compares two consumers of a wrong index), the oracle on it, and the oracle's records and counters of every run, computed once; the counts
    of those records are the recorded ones, which are the reference's"""
    made = {}

    def get(name):
        if name not in made:
            assert lci.codes_sha256(name) == GOLD["genomes"][name]["codes_sha256"], "the genome generator drifted from the recorded inputs"
            prefix = os.path.join(workdir, "lowcgpu_" + name)
            index_build.build_index_from_genome(lci.make_genome(name), prefix)
            _index_is_recorded(name, prefix, "default builder")
            orc = oracle_py.Oracle(prefix)
            want, figs = {}, {}
            for key, paired, flags in lci.runs(name):
                p, h = common.parse_flags(flags)
                rec = tl.oracle_records(orc, name, paired, flags)
                want[key] = dict(paired=paired, p=p, h=h, batch=lci.batch(name, paired), rec=rec, ctr=dict(orc.counters))
                figs[key] = tl.figures_of(rec)
                assert figs[key] == {k: GOLD["runs"][key][k] for k in figs[key]}, key
            tl.check_not_vacuous(name, figs)
            made[name] = dict(prefix=prefix, ix=host.Index(prefix), orc=orc, want=want)
        return made[name]
    yield get
    for v in made.values():
        v["orc"].close()


def _seqs(name, paired):
    return lci.stored_pairs(*lci.paired_reads(name)) if paired else lci.single_reads(name)


def _packed(name, paired):
    """the run's ragged reads as dg_map_batch_packed takes them: 2 bits per base in words of the longest read's width, N listed, the lengths beside them"""
    seqs = _seqs(name, paired)
    lens = np.asarray([len(s) for s in seqs], np.uint16)
    arr = np.full((len(seqs), int(lens.max())), ord("A"), np.uint8)
    for i, s in enumerate(seqs):
        arr[i, :len(s)] = np.frombuffer(s, np.uint8)
    words, nlist = host.pack_reads_2bit(arr)
    return words, nlist, lens


@pytest.mark.parametrize("sorter", ["hip", "hip-python", "plain", "bucketed"])
@pytest.mark.parametrize("name", lci.NAMES)
def test_gpu_index_builder_writes_the_reference_indexers_files_for_low_complexity_genomes(name, sorter, workdir, monkeypatch):
    """di_build_files (hip), the same kernels driven from index_build.py (hip-python) and the two torch-orchestrated sorters on texts where 13 or 14 of
    the 16 two-symbol buckets are empty, one bucket spans more than one 4096-pair tile, ties run to the end of the text (homopolymer_long) and every
    suffix ties with its partner on the other strand until the sentinel (self_rc, palindrome): the reference's five files"""
    _select(sorter, monkeypatch)
    prefix = os.path.join(workdir, "lowcidx_%s_%s" % (name, sorter))
    index_build.build_index_from_genome(lci.make_genome(name), prefix, device="cuda")
    _index_is_recorded(name, prefix, sorter + " sorter")


@pytest.mark.parametrize("name", ["self_rc", "homopolymer_long"])
def test_dart_index_writes_the_reference_indexers_files_for_low_complexity_fasta(name, workdir):
    d = os.path.join(workdir, "lowccli_" + name)
    lci.write_inputs(name, d)
    r = subprocess.run([DART, "index", "g.fa", "g"], cwd=d, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    _index_is_recorded(name, os.path.join(d, "g"), "dart index")


def test_dart_maps_twins_with_all_places_like_the_oracle(workdir):
    """`dart index`, then `dart -m` on the genome that holds one contig three times: the oracle command line's SAM (three lines per read), junctions and
    statistics, which are the ones the reference wrote"""
    import hashlib
    oracle_py.build()
    d = os.path.join(workdir, "lowccli_twins")
    se, pe = lci.write_inputs("twins", d)
    subprocess.run([DART, "index", "g.fa", "g"], cwd=d, check=True, stdout=subprocess.DEVNULL)
    _index_is_recorded("twins", os.path.join(d, "g"), "dart index")
    for key, files, extra in (("twins " + lci.MULTI_RUN, se, ["-mis", "5", "-m", "-max_dup", "1000"]), ("twins pe: -mis 5", pe, ["-mis", "5"])):
        flags = files + extra
        rg = subprocess.run([DART, "-i", "g"] + flags + ["-o", "gpu.sam", "-j", "gpu.j", "-t", "3"], cwd=d, stdout=subprocess.PIPE, check=True)
        ro = subprocess.run([oracle_py.ORACLE_CLI, "-i", "g"] + flags + ["-o", "orc.sam", "-j", "orc.j"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        a, b = open(os.path.join(d, "orc.sam")).read(), open(os.path.join(d, "gpu.sam")).read()
        assert a == b, (key, common.first_diff(b, a))
        junc = open(os.path.join(d, "gpu.j")).read()
        assert open(os.path.join(d, "orc.j")).read() == junc, key
        assert common.stats_block(rg.stdout) == common.stats_block(ro.stdout) == GOLD["runs"][key]["stats"] != "", (key, rg.stdout[-600:])
        assert hashlib.sha256(b.encode()).hexdigest() == GOLD["runs"][key]["sam_sha256"] and hashlib.sha256(junc.encode()).hexdigest() == GOLD["runs"][key]["junctions_sha256"], key


@pytest.mark.parametrize("name", lci.NAMES)
def test_gpu_records_and_counters_match_oracle_on_low_complexity_genome(name, lowc):
    s = lowc(name)
    gpu = host.DartGPU(s["ix"])
    total = {k: 0 for k in PATHS}
    try:
        gpu.wait_index()
        for key, w in s["want"].items():
            gpu.set_params(host.default_params(paired=int(w["paired"]), **w["p"]))
            common.assert_same(gpu.map_batch(*w["batch"]), w["rec"])      # (after any growth of the data-dependent buffers: reruns_capacity_total may be positive)
            c = gpu.counters()
            for mine, theirs in COUNTERS:
                assert c[mine] == w["ctr"][theirs], (key, mine, c[mine], w["ctr"][theirs])
            assert c["reruns_scan_total"] == 0, key
            for k in total:
                total[k] += c[k]
            fig = tl.figures_of(w["rec"])
            print("FIGURES %-46s mapped %3d of %3d, %3d with several places; %s" % (key, fig["n_mapped"], fig["n_reads"], fig["n_multi"],
                  " ".join("%s=%d" % (k, c[k]) for k in ("wave_chained_units", "general_path_units", "wave_ticks_k_seed_heavy", "wave_ticks_k_chain_heavy", "ktab_lookups", "reruns_capacity_total"))))
            # the packed entry and both compact forms: the reads hold A, C, G, T and N only
            words, nlist, lens = _packed(name, w["paired"])
            common.assert_same(gpu.map_batch_packed(words, nlist, 0, rlen=lens), w["rec"])
            common.assert_same(gpu.download_compact(), w["rec"])
            common.assert_same(gpu.map_batch_compact(words, nlist, 0, rlen=lens), w["rec"])
        for k, names in PATHS.items():
            if name in names:
                assert total[k] > 0, "%s stayed 0 over the runs of %s: its reads no longer reach that path" % (k, name)
    finally:
        gpu.close()


@pytest.mark.parametrize("name", AID_GENOMES)
def test_gpu_index_aids_and_seeding_kernels_on_low_complexity_genome(name, lowc, monkeypatch):
    """no prefix table, no dense suffix array, every 4th row of it -- each with the lane-per-read kernel, the phased queue kernel and the queue kernel
    without few-row comparisons -- and the queue kernel handing reads to k_seed_heavy after 6 trips or never: the oracle's records, and the
    reference-equivalent seeding counters of the default configuration"""
    s = lowc(name)
    keys = [k for k in s["want"] if k.endswith("e: -mis 5") or k.endswith(lci.MULTI_RUN)]
    base = {}
    gpu = host.DartGPU(s["ix"])
    try:
        for key in keys:
            w = s["want"][key]
            gpu.set_params(host.default_params(paired=int(w["paired"]), **w["p"]))
            common.assert_same(gpu.map_batch(*w["batch"]), w["rec"])
            base[key] = gpu.counters()
    finally:
        gpu.close()
    combos = [((aid, av), (kernel, kv)) for aid, av in (("DG_KTAB_K", "0"), ("DG_SA_DENSE", "0"), ("DG_SA_DENSE", "4"))
              for kernel, kv in (("DG_SEED_LEGACY", "1"), ("DG_SEED_PHASES", "1"), ("DG_SEED_MULTI", "0"))]
    combos += [(("DG_SEED_BAIL_TRIPS", "6"),), (("DG_SEED_BAIL_TRIPS", "1000"),)]
    for combo in combos:
        for k, v in combo:
            monkeypatch.setenv(k, v)
        gpu = host.DartGPU(s["ix"])                      # (the aids are chosen when the index is loaded, the kernels at dg_set_params)
        try:
            for key in keys:
                w = s["want"][key]
                gpu.set_params(host.default_params(paired=int(w["paired"]), **w["p"]))
                common.assert_same(gpu.map_batch(*w["batch"]), w["rec"])
                c = gpu.counters()
                for k in ("steps", "lf_steps", "sa_lookups", "seeds"):
                    assert c[k] == base[key][k], (key, k, combo)
        finally:
            gpu.close()
            for k, _ in combo:
                monkeypatch.delenv(k)


def _steps_executed(s, keys):
    """a fresh context under the switches of the moment -> run -> Occ steps the seeding kernels really made (the records are checked on the way)"""
    gpu = host.DartGPU(s["ix"])
    try:
        out = {}
        for key in keys:
            w = s["want"][key]
            gpu.set_params(host.default_params(paired=int(w["paired"]), **w["p"]))
            common.assert_same(gpu.map_batch(*w["batch"]), w["rec"])
            out[key] = gpu.counters()["steps_executed"]
        return out
    finally:
        gpu.close()


@pytest.mark.parametrize("name", HEAVY_GENOMES)
def test_gpu_reads_go_through_k_seed_heavy_on_low_complexity_genome(name, lowc, monkeypatch):
    """wave_ticks_k_seed_heavy is positive even for an empty list of heavy reads (the ticks of an empty launch), so it proves nothing.  What does: with
    DG_SEED_BAIL_TRIPS=1000 no read reaches 1000 trips and every search runs in k_seed_qf, while k_seed_heavy_walk spares a handed-over read the
    searches it proves to fail.  The steps really made are the same in two contexts under the same switches; so a different number under the
    default switches, for the same reference-equivalent steps, says that there reads were handed to k_seed_heavy_walk and k_seed_heavy."""
    s = lowc(name)
    keys = list(s["want"])
    first, again = _steps_executed(s, keys), _steps_executed(s, keys)
    monkeypatch.setenv("DG_SEED_BAIL_TRIPS", "1000")
    try:
        never = _steps_executed(s, keys)
    finally:
        monkeypatch.delenv("DG_SEED_BAIL_TRIPS")
    print("FIGURES steps_executed", name, {k: (first[k], again[k], never[k]) for k in keys})
    assert first == again, "steps_executed differs between two contexts under the same switches: it cannot show a hand-over"
    assert any(first[k] != never[k] for k in keys), "no run of %s hands a read to k_seed_heavy under the default switches" % name


@pytest.mark.parametrize("name", TEXT_GENOMES)
def test_gpu_sam_text_on_low_complexity_genome(name, lowc, workdir):
    """format_sam_resident and format_sam are sam.format_records of the oracle's records: -m secondaries of reads with three equally good places, mates on
    different contigs, spliced reads whose boundary could lie anywhere in a run"""
    s = lowc(name)
    d = os.path.join(workdir, "lowctext_" + name)
    lci.write_inputs(name, d)
    gpu = host.DartGPU(s["ix"])
    try:
        for key, w in s["want"].items():
            paired = w["paired"]
            seqs = _seqs(name, paired)
            n = len(seqs)
            headers = [b"r%d" % (i // 2 if paired else i) for i in range(n)]
            quals = [b"I" * len(x) for x in seqs]
            t1 = open(os.path.join(d, "p1.fq" if paired else "a.fq"), "rb").read()
            t2 = open(os.path.join(d, "p2.fq"), "rb").read() if paired else None
            gpu.set_params(host.default_params(paired=int(paired), **w["p"]))
            assert gpu.upload_fastq(t1, t2, rc_odd_reads=paired) == n
            gpu.run()
            common.assert_same(gpu.download(), w["rec"])
            reads, rep, cig, sj = w["rec"]
            npm = n if paired else 0
            twin, st = sdi.twin_text(headers, seqs, quals, reads, rep, cig, s["ix"].names, npm, multi=bool(w["p"]["multi_hit"]), unique=w["h"]["unique"])
            if w["p"]["multi_hit"]:
                assert twin.count(b"\n") > n                 # (secondary lines are there to be compared)
            text, ct = gpu.format_sam_resident(npm, unique_only=w["h"]["unique"])
            assert text == twin, common.first_diff(text.decode("latin1"), twin.decode("latin1"))
            assert ct == dict(unmapped=st.unmapped, unique=st.unique, paired=st.paired)
            text2, ct2 = gpu.format_sam(headers, quals, npm, unique_only=w["h"]["unique"])
            assert text2 == twin and ct2 == ct
    finally:
        gpu.close()
