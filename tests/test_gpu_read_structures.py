"""GPU suite (-m gpu): the read and pair structures of tests/read_structures.py -- what synth.make_reads never makes -- through the HIP path, every record
against the oracle: per class and flag set (the 250-base set also at -mis 100, under which its insertions of 31-80 bases map), paired and with every mate as its own read, through the ASCII, the packed and the compact entry points; all
classes shuffled into one batch; the reference-equivalent counters; and the reference's own SAM and junctions of the -mis 12 -m run (tests/golden/
read_structures.mis12m.*) through the records and through `dart`.  tests/test_read_structures_oracle.py states what path each class reaches."""
import os, subprocess
import numpy as np
import pytest
import common, oracle_py, read_structures as rs, read_structure_inputs as rsi
from dart_amd import host, sam

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")


def _class_ids():
    """(set, class) of every class of both sets, without building them: the names depend on the read length alone"""
    return [(name, cls) for name, (case, rlen) in rsi.SETS.items() for cls in rs.class_names(rlen)]


@pytest.fixture(scope="module")
def ctxs(workdir):
    """one context per genome"""
    out = {}
    for name in rsi.SETS:
        c, classes, info = rsi.read_set(name, workdir)
        ix = host.Index(c["prefix"])
        out[name] = (c, classes, ix, host.DartGPU(ix), oracle_py.Oracle(c["prefix"]))
    yield out
    for c, classes, ix, gpu, orc in out.values():
        gpu.close(); orc.close()


def _assert_counters(c, oc):
    """the reference-equivalent counters of a run against the oracle's (as test_gpu_reference_equivalent_counters)"""
    assert c["steps"] == oc["n_2occ4"]
    assert c["lf_steps"] == oc["n_lf"]
    assert c["sa_lookups"] == oc["n_sa"]
    assert c["nw_calls"] == oc["n_nw"] and c["nw_cells"] == oc["nw_cells"]
    assert c["reseed_calls"] == oc["n_reseed"] and c["reseed_window"] == oc["reseed_window"]
    assert 0 <= oc["n_occ_blocks"] - (c["occ_blocks"] + c["lf_steps"]) <= 1e-2 * oc["n_occ_blocks"]


def _map_and_compare(gpu, orc, reads, flags, paired, every_entry_point=True):
    """-> (the oracle's records, the GPU's counters, the oracle's counters)"""
    p, _ = common.parse_flags(flags)
    so, rl, flat = host.pack_reads(reads)
    want = orc.map_batch(orc.params(paired=paired, **p), so, rl, flat, threads=4)
    oc = dict(orc.counters)
    gpu.set_params(host.default_params(paired=paired, **p))
    common.assert_same(gpu.map_batch(so, rl, flat), want)
    ctr = gpu.counters()
    if every_entry_point:                            # (the classes hold A/C/G/T only: 2-bit words in, and compact records out)
        words, nlist, longest, lens = rsi.padded_2bit(reads)
        common.assert_same(gpu.map_batch_packed(words, nlist, longest, lens), want)
        common.assert_same(gpu.download_compact(), want)
        common.assert_same(gpu.map_batch_compact(words, nlist, longest, lens), want)
    return want, ctr, oc


@pytest.mark.parametrize("name,cls", _class_ids(), ids=["%s-%s" % t for t in _class_ids()])
def test_gpu_class_matches_oracle(name, cls, ctxs):
    c, classes, ix, gpu, orc = ctxs[name]
    reads = rs.as_reads(classes[cls])
    for flags in rsi.GPU_FLAG_SETS[name]:
        for paired in (1, 0):
            try:
                want, ctr, oc = _map_and_compare(gpu, orc, reads, flags, paired)
                _assert_counters(ctr, oc)
            except AssertionError as e:
                raise AssertionError("%s %s %s paired=%d: %s" % (name, cls, " ".join(flags), paired, str(e)[:600]))


def _per_read(reads, rep, cig, sj):
    """per read: its record, its reports with their CIGARs, its junction tuples -- without the places they have in the batch's arrays"""
    ops = rsi.cigar_lists(rep, cig)
    out = []
    for r in reads:
        lo, n = int(r["rep_off"]), int(r["n_rep"])
        head = tuple(int(r[f]) for f in ("score", "sub_score", "mis_num", "mapq", "n_rep", "best", "n_sj"))
        reps = [tuple(int(rep[k][f]) for f in ("aln_score", "sj_type", "flag", "paired_idx", "chr", "bdir", "pos")) + (tuple(ops[k]),) for k in range(lo, lo + n)]
        tuples = [(int(t["g1"]), int(t["g2"]), int(t["type"])) for t in sj[int(r["sj_off"]):int(r["sj_off"]) + int(r["n_sj"])]] if int(r["n_sj"]) else []
        out.append((head, reps, tuples))
    return out


@pytest.mark.parametrize("name", sorted(rsi.SETS))
def test_gpu_all_classes_in_one_shuffled_batch(name, ctxs):
    """every class in one batch, shuffled by pairs (k_pair's workgroups, k_report's item order and the shared re-seeding windows see mixed neighbours): the batch against
    the oracle, every read's records equal to those of its class mapped alone, and the counters of the whole set"""
    c, classes, ix, gpu, orc = ctxs[name]
    pairs, names = rs.all_pairs(classes)
    order = np.random.default_rng(77).permutation(len(pairs))
    reads = rs.as_reads([pairs[i] for i in order])
    nw = reseed = 0
    for flags in rsi.GPU_FLAG_SETS[name]:
        p, _ = common.parse_flags(flags)
        for paired in (1, 0):
            want, ctr, oc = _map_and_compare(gpu, orc, reads, flags, paired, every_entry_point=paired == 1)
            _assert_counters(ctr, oc)
            nw += ctr["nw_calls"]; reseed += ctr["reseed_calls"]
            alone = []
            for cl_pairs in classes.values():
                so, rl, flat = host.pack_reads(rs.as_reads(cl_pairs))
                alone += _per_read(*orc.map_batch(orc.params(paired=paired, **p), so, rl, flat, threads=4))
            mixed = _per_read(*want)
            for k, i in enumerate(order.tolist()):
                for m in (0, 1):
                    assert mixed[2 * k + m] == alone[2 * i + m], (names[i], flags, paired, i, m)
    assert nw > 0 and reseed > 0


def _fixture_inputs(ctxs):
    c, classes, ix, gpu, orc = ctxs["rs101"]
    pairs, _ = rs.all_pairs(classes)
    reads = rs.as_reads(pairs)
    headers = ["p%d" % (i // 2) for i in range(len(reads))]
    quals = ["I" * len(r) for r in reads]
    return c, ix, gpu, pairs, reads, headers, quals


def test_gpu_records_print_the_reference_sam_of_the_read_structures(ctxs):
    """the -mis 12 -m run the reference's object code wrote (multi-N and long-I CIGARs, unpaired and improper flags, mates of different lengths): the GPU's records through
    the Python formatter, line by line, and its junction table"""
    c, ix, gpu, pairs, reads, headers, quals = _fixture_inputs(ctxs)
    p, _ = common.parse_flags(rsi.FIXTURE_FLAGS)
    gpu.set_params(host.default_params(paired=1, **p))
    res = gpu.map_batch(*host.pack_reads(reads))
    body = sam.format_records(headers, [r.decode() for r in reads], quals, res.reads, res.reports, res.cigar, ix.names, paired=True, multi_hit=True)
    text = sam.sam_header(ix.names, ix.chr_len) + body
    want = rsi.fixture_sam()
    assert text == want, common.first_diff(text, want)
    assert sam.junction_table(res.sj, ix.names, ix.chr_off, ix.chr_len, ix.l_pac) == rsi.fixture_junctions()


def test_dart_cli_read_structures_reproduce_the_reference_sam(ctxs, workdir):
    """the same run through `dart`, on both host pipelines, in several batches"""
    c, ix, gpu, pairs, reads, headers, quals = _fixture_inputs(ctxs)
    d = os.path.join(workdir, "read_structures_cli"); os.makedirs(d, exist_ok=True)
    rs.write_fastq(os.path.join(d, "a.fq"), os.path.join(d, "b.fq"), pairs)
    want = rsi.fixture_sam()
    for env in (dict(os.environ, DART_BATCH="1000"), dict(os.environ, DART_BATCH="1000", DART_STREAMING="1")):
        r = subprocess.run([DART, "-i", c["prefix"], "-f", "a.fq", "-f2", "b.fq"] + rsi.FIXTURE_FLAGS + ["-o", "o.sam", "-j", "o.j", "-t", "4"], cwd=d, stdout=subprocess.PIPE, check=True, env=env)
        got = open(os.path.join(d, "o.sam")).read()
        assert got == want, common.first_diff(got, want)
        assert open(os.path.join(d, "o.j")).read() == rsi.fixture_junctions()
        assert common.stats_block(r.stdout) == rsi.gold()["runs"][rsi.run_key("rs101", rsi.FIXTURE_FLAGS)]["stats"]
