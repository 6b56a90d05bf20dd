"""GPU suite (-m gpu): the device's text holds both strands (k_pac_both builds the reverse complement once, when the index is loaded), and no kernel computes a
reverse complement per access.  Four two-chromosome genomes of L = 2000, 2002, 3003 and 4097 bases (every L % 4, so the byte that holds symbols around L is
composed in three of them); about 600 pairs of 2x101 and 200 of 2x36 each, a quarter of them from the first and last 150 bases of a chromosome so that seeds and
gap windows touch 0, L and 2L; 1 % substitutions, 5 % of the pairs with a 1-3 base indel, a few N.  Every record, CIGAR op, junction tuple and
reference-equivalent counter against the oracle, through the ASCII, packed and compact entry points, at -mis 5 and at the default; and the text as the kernels
read it (dg_probe_refseq) against the text's definition over the whole of [0, 2L) and 70 positions either side."""
import os
import numpy as np
import pytest
import common, oracle_py
from dart_amd import host, index_build, synth

pytestmark = pytest.mark.gpu
GENOMES = {"L2000": [1200, 800], "L2002": [1201, 801], "L3003": [1800, 1203], "L4097": [2500, 1597]}
FLAG_SETS = (["-mis", "5"], [])
EDGE = 150
# the GPU's counter -> the oracle's (occ_blocks is a lower bound by design and stays out)
COUNTERS = (("steps", "n_2occ4"), ("lf_steps", "n_lf"), ("sa_lookups", "n_sa"), ("nw_calls", "n_nw"), ("nw_cells", "nw_cells"),
            ("reseed_calls", "n_reseed"), ("reseed_window", "reseed_window"))
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = np.full(256, ord("N"), np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def _revcomp(a):
    return _COMP[a[::-1]]


def _genome(name):
    lens = GENOMES[name]
    rng = np.random.default_rng(9100 + sum(lens))
    return synth.Genome(["c1", "c2"], lens, rng.integers(0, 4, size=sum(lens), dtype=np.uint8), np.zeros((0, 3), np.int64))


def _edit(rng, src, rlen, indel):
    """a mate of rlen bases from src (rlen + 3 bases of the fragment's direction): 1 % substitutions, with `indel` a 1-3 base insertion or deletion, rarely an N"""
    s = src.copy()
    if indel:
        n = int(rng.integers(1, 4)); q = int(rng.integers(rlen // 3, 2 * rlen // 3))
        s = np.concatenate([s[:q], s[q + n:]]) if rng.random() < 0.5 else np.concatenate([s[:q], _ACGT[rng.integers(0, 4, n)], s[q:]])
    s = s[:rlen].copy()
    for q in np.nonzero(rng.random(rlen) < 0.01)[0]:
        s[q] = _ACGT[(int(np.nonzero(_ACGT == s[q])[0][0]) + int(rng.integers(1, 4))) & 3]
    if rng.random() < 0.02:
        s[int(rng.integers(0, rlen))] = ord("N")
    return s


def _reads(g, name):
    """the batch as the loader stores it (mate 1, then mate 2 reverse-complemented): list of bytes"""
    rng = np.random.default_rng(9200 + g.total)
    text = g.ascii()
    out = []
    n_edge = n_indel = 0
    for rlen, n_pairs in ((101, 600), (36, 200)):
        for k in range(n_pairs):
            ci = k % 2
            off, ln = int(g.offsets[ci]), int(g.lengths[ci])
            flen = int(rng.integers(rlen + 8, min(ln, rlen + 300) + 1))
            where = k % 8
            if where == 0:   s = int(rng.integers(0, EDGE - 100 if rlen == 101 else EDGE - 36))      # mate 1 inside the chromosome's first 150 bases
            elif where == 1: s = ln - flen - int(rng.integers(0, EDGE - 100 if rlen == 101 else EDGE - 36))      # mate 2 inside its last 150
            else:            s = int(rng.integers(0, ln - flen + 1))
            if where == 0 and k % 16 == 0: s = 0
            if where == 1 and k % 16 == 1: s = ln - flen
            n_edge += where < 2
            frag = text[off + s: off + s + flen]
            indel = rng.random() < 0.05
            n_indel += indel
            which = int(rng.integers(0, 2))
            a = _edit(rng, frag[:rlen + 3], rlen, indel and which == 0)                     # mate 1: the fragment's first bases
            b = _edit(rng, _revcomp(frag)[:rlen + 3], rlen, indel and which == 1)           # mate 2 as sequenced: the other strand's first bases
            if k % 4 >= 2:                                                                  # every second pair of fragments from the reverse strand
                a, b = b, a
            out.append(a.tobytes()); out.append(_revcomp(b).tobytes())
    assert n_edge >= 190 and n_indel >= 20, (name, n_edge, n_indel)
    return out


def _packed(seqs):
    lens = np.asarray([len(s) for s in seqs], np.uint16)
    arr = np.full((len(seqs), int(lens.max())), ord("A"), np.uint8)
    for i, s in enumerate(seqs):
        arr[i, :len(s)] = np.frombuffer(s, np.uint8)
    words, nlist = host.pack_reads_2bit(arr)
    return words, nlist, lens


@pytest.fixture(scope="module")
def cases(workdir):
    """genome name -> dict(g, ix, seqs, batch, want): the index, the reads, and the oracle's records and counters under both flag sets, computed once"""
    made = {}

    def get(name):
        if name not in made:
            g = _genome(name)
            prefix = os.path.join(workdir, "pacboth_" + name)
            index_build.build_index_from_genome(g, prefix)
            seqs = _reads(g, name)
            b = host.pack_reads(seqs)
            orc = oracle_py.Oracle(prefix)
            want = []
            for flags in FLAG_SETS:
                p, _ = common.parse_flags(flags)
                rec = orc.map_batch(orc.params(paired=1, **p), *b)
                want.append(dict(p=p, rec=rec, ctr=dict(orc.counters)))
            orc.close()
            assert int((want[0]["rec"][0]["score"] > 0).sum()) > len(seqs) // 2, name      # (most reads map: the comparison below is not one of empty records)
            made[name] = dict(g=g, ix=host.Index(prefix), seqs=seqs, batch=b, want=want)
        return made[name]
    return get


@pytest.mark.parametrize("flag_set", range(len(FLAG_SETS)), ids=["mis5", "default"])
@pytest.mark.parametrize("name", sorted(GENOMES))
def test_gpu_records_and_counters_match_oracle_with_both_strands_stored(name, flag_set, cases):
    c = cases(name)
    w = c["want"][flag_set]
    gpu = host.DartGPU(c["ix"])
    try:
        gpu.wait_index()
        assert "k_pac_both" in gpu.init_report(), gpu.init_report()
        gpu.set_params(host.default_params(paired=1, **w["p"]))
        common.assert_same(gpu.map_batch(*c["batch"]), w["rec"])
        ctr = gpu.counters()
        for mine, theirs in COUNTERS:
            assert ctr[mine] == w["ctr"][theirs], (name, mine, ctr[mine], w["ctr"][theirs])
        words, nlist, lens = _packed(c["seqs"])
        common.assert_same(gpu.map_batch_packed(words, nlist, 0, rlen=lens), w["rec"])
        ctr = gpu.counters()
        for mine, theirs in COUNTERS:
            assert ctr[mine] == w["ctr"][theirs], (name, "packed", mine, ctr[mine], w["ctr"][theirs])
        common.assert_same(gpu.download_compact(), w["rec"])
        common.assert_same(gpu.map_batch_compact(words, nlist, 0, rlen=lens), w["rec"])
    finally:
        gpu.close()


@pytest.mark.parametrize("name", sorted(GENOMES))
def test_gpu_text_as_the_kernels_read_it_is_forward_then_reverse_complement(name, cases):
    c = cases(name)
    fwd = c["g"].ascii()
    L = len(fwd)
    want = np.concatenate([np.zeros(70, np.uint8), fwd, _revcomp(fwd), np.zeros(70, np.uint8)]).tobytes()
    for kw in (dict(from_files=False), dict(from_files=True)):
        gpu = host.DartGPU(c["ix"], **kw)
        try:
            got = gpu.probe_refseq(-70, 2 * L + 140)
            assert got == want, (name, kw, common.first_diff(got.decode("latin1"), want.decode("latin1")))
            assert gpu.probe_refseq(L - 3, 6) == want[70 + L - 3:70 + L + 3] and gpu.probe_refseq(0, 0) == b""
        finally:
            gpu.close()
