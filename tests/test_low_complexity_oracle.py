"""CPU suite: the checker pinned on low-complexity genomes (tests/low_complexity_inputs.py: homopolymers, microsatellites, a text equal to its own
reverse complement, contigs present three times, a ladder of copy counts around max_dup / 128 rows / 16 seeds) before the GPU tests rely on it
there (tests/test_gpu_low_complexity.py).  Per genome: the CPU index builder's five files are the bytes the reference's indexer wrote; the oracle's
command line writes the SAM, the junctions and the statistics the reference's object code wrote for every run (tests/golden/low_complexity.json,
made by tests/golden/make_low_complexity.py; where oracle/_ref exists the reference also runs live beside it); the library entry agrees with the
command line's counts; and the runs are worth comparing: reads map where they should and nowhere on the long homopolymer, most mapped reads of
the -m runs have several places, junctions are written, and every rung of the ladder is met from the side its copy count says."""
import json, os
import numpy as np
import pytest
import common, oracle_py
import low_complexity_inputs as lci
import test_oracle_vs_ref as t
from dart_amd import index_build

GOLD_PATH = os.path.join(common.GOLDEN, "low_complexity.json")
MAPS_NOTHING = "homopolymer_long"
MULTI_GENOMES = ("dinuc", "twins", "ladder")
INSIDE_KINDS = ("inside", "pure17")                  # unmodified windows of the rung


def gold():
    return json.load(open(GOLD_PATH))


def oracle_records(orc, name, paired, flags):
    p, _ = common.parse_flags(flags)
    return orc.map_batch(orc.params(paired=int(paired), **p), *lci.batch(name, paired), cap_scale=16)        # (-m: hundreds of places per read)


def figures_of(rec):
    """the counts of one run from the oracle's records: reads, mapped reads, mapped reads with more than one place, junction tuples"""
    reads, rep, cig, sj = rec
    mapped = reads["score"] > 0
    return {"n_reads": len(reads), "n_mapped": int(mapped.sum()), "n_multi": int((mapped & (reads["n_rep"] > 1)).sum()), "n_junction_tuples": len(sj)}


def oracle_figures(orc, name, paired, flags):
    return figures_of(oracle_records(orc, name, paired, flags))


def ladder_figures(mapped_dup100, mapped_dup1000):
    """per rung of the ladder, from the mapped flags of the single-end runs with max_dup 100 and 1000: the 17-mer's copies in the text, the distinct reads wholly
    inside the rung (windows of it, unmodified), and how many of its probe reads -- whose first seed's interval is exactly the copy count -- mapped under either limit"""
    g = lci.make_genome("ladder")
    tags = lci.tagged_single_reads("ladder")
    out = []
    for k, ((unit, want), copies) in enumerate(zip(lci.LADDER, lci.rung_copies())):
        ri = g.rungs[k]
        inside = [i for i, (kind, r, _) in enumerate(tags) if r == ri and kind in INSIDE_KINDS]
        pr = [i for i, (kind, r, _) in enumerate(tags) if r == ri and kind == "probe"]
        assert all(s in lci.tile(unit, len(s) + len(unit)) for _, _, s in (tags[i] for i in inside))
        out.append({"unit": unit.decode(), "copies": copies, "n_inside": len({tags[i][2] for i in inside}), "n_probe": len(pr),
                    "probe_mapped_max_dup_100": int(mapped_dup100[pr].sum()), "probe_mapped_max_dup_1000": int(mapped_dup1000[pr].sum()),
                    "inside_mapped_max_dup_100": int(mapped_dup100[inside].sum()), "inside_mapped_max_dup_1000": int(mapped_dup1000[inside].sum())})
    return out


def check_ladder(rungs):
    """every rung has its planned copy count and at least 10 different reads wholly inside; its probe reads map under a limit exactly when the copy count is
    within it, so the two runs differ exactly on the rungs of 101 .. 1000 copies -> the number of those rungs"""
    assert [r["copies"] for r in rungs] == [c for _, c in lci.LADDER], rungs
    differ = 0
    for r in rungs:
        assert r["n_inside"] >= 10 and r["n_probe"] >= 4, r
        assert r["probe_mapped_max_dup_100"] == (r["n_probe"] if r["copies"] <= 100 else 0), r
        assert r["probe_mapped_max_dup_1000"] == (r["n_probe"] if r["copies"] <= 1000 else 0), r
        differ += r["probe_mapped_max_dup_100"] != r["probe_mapped_max_dup_1000"]
    assert differ == sum(100 < c <= 1000 for _, c in lci.LADDER)
    return differ


def check_not_vacuous(name, figs):
    """figs: run key -> figures of every run of the genome"""
    if name == MAPS_NOTHING:
        assert all(f["n_mapped"] == 0 and f["n_reads"] > 50 for f in figs.values()), figs
        return
    assert any(4 * f["n_mapped"] >= f["n_reads"] for f in figs.values()), (name, figs)
    if name in MULTI_GENOMES:
        f = figs["%s %s" % (name, lci.MULTI_RUN)]
        assert f["n_mapped"] > 0 and 10 * f["n_multi"] >= 3 * f["n_mapped"], (name, f)
    if name == "micro":
        assert max(f["n_junction_tuples"] for f in figs.values()) >= 20, figs


def prepare(name, workdir):
    """the genome's FASTA, reads and CPU-built index under workdir -> (directory, prefix, single-end files, paired files)"""
    d = os.path.join(workdir, "lowc_" + name)
    se, pe = lci.write_inputs(name, d)
    prefix = os.path.join(d, "g")
    if not os.path.exists(prefix + ".sa"):
        index_build.build_index_from_genome(lci.make_genome(name), prefix, device="cpu")
    return d, prefix, se, pe


@pytest.mark.parametrize("name", lci.NAMES)
def test_low_complexity_inputs_and_cpu_index_are_the_recorded_ones(name, workdir):
    g = gold()["genomes"][name]
    assert lci.codes_sha256(name) == g["codes_sha256"], "the genome generator drifted from the recorded inputs"
    pe = lci.paired_reads(name)
    assert lci.reads_sha256(lci.single_reads(name)) == g["reads_sha256"]["se"] and lci.reads_sha256(pe[0] + pe[1]) == g["reads_sha256"]["pe"]
    assert lci.make_genome(name).total <= 65536 and len(lci.single_reads(name)) + len(pe[0]) <= 700
    d, prefix, se, pe_files = prepare(name, workdir)
    for ext, want in g["index_sha256"].items():
        assert common.sha(prefix + "." + ext) == want, "CPU-built .%s differs from the reference indexer's (%s)" % (ext, name)


def test_low_complexity_texts_are_what_their_names_say():
    """the properties the genomes are there for, from the texts themselves"""
    both = lci.both_strands
    for name in ("self_rc", "palindrome"):               # the text of both strands is the forward text twice: every suffix ties with its partner
        f = lci.make_genome(name).ascii().tobytes()
        if name == "self_rc": f = f[:900]
        assert lci.revcomp(f) == f, name
    t3 = lci.make_genome("twins").ascii().tobytes()
    assert t3[:3000] == t3[3000:6000] == lci.revcomp(t3[6000:])
    hl = both("homopolymer_long")
    assert hl == b"A" * 4200 + b"T" * 4200                # 14 of the 16 two-symbol buckets are empty; AA holds 4199 suffixes, more than one 4096-pair tile
    run = lci.make_genome("homopolymer").ascii().tobytes()[500:]
    pairs = {(run + lci.revcomp(run))[i:i + 2] for i in range(1199)}
    assert len(pairs) == 3                                # AA, AT, TT: 13 of the 16 buckets of the run's contig are empty
    assert lci.count_occurrences(run + lci.revcomp(run), b"A" * 16) == 585          # (a 115-base run would hold 100 of them, a 116-base run 101)
    assert lci.rung_copies() == [c for _, c in lci.LADDER] == gold()["ladder"]["copies"]
    for name in ("ladder", "micro"):                     # every planted run is in the text as listed, and no longer than listed
        g = lci.make_genome(name)
        text = g.ascii().tobytes()
        ends = set(np.cumsum(g.lengths).tolist())
        for a, r, u in g.runs:
            assert text[a:a + r] == lci.tile(u, r), (name, a)
            assert a in ends or a == 0 or text[a - 1:a + r] != lci.tile(u, r + 1, len(u) - 1), (name, a)
            assert a + r in ends or text[a:a + r + 1] != lci.tile(u, r + 1), (name, a)
    g = lci.make_genome("micro")
    text = g.ascii().tobytes()
    assert {u for _, _, u in g.runs} == set(lci.MICRO_UNITS) and all(24 <= r <= 400 for _, r, _ in g.runs)
    for (d, sk, motif), in zip(g.introns.tolist()):      # both ends of every skip lie in the middle of 24-base runs of one unit, but for a motif's two bases
        w1, w2 = text[d - 12:d + 12], text[d + sk - 12:d + sk + 12]
        same = [w1 == lci.tile(u, 24) and w2 == lci.tile(u, 24) for u in lci.MICRO_UNITS]
        if motif:
            same = [w1[:12] + w1[14:] == lci.tile(u, 24)[:12] + lci.tile(u, 24)[14:] and w2[:10] + w2[12:] == lci.tile(u, 24)[:10] + lci.tile(u, 24)[12:] for u in lci.MICRO_UNITS]
        assert any(same), (d, sk, motif)


@pytest.mark.parametrize("name", lci.NAMES)
def test_oracle_matches_reference_on_low_complexity_genome(name, workdir):
    oracle_py.build()
    d, prefix, se, pe_files = prepare(name, workdir)
    runs = gold()["runs"]
    orc = oracle_py.Oracle(prefix)
    try:
        figs, mapped = {}, {}
        for key, paired, flags in lci.runs(name):
            t.run_both(d, prefix, (pe_files if paired else se) + flags, key, want=runs[key])
            rec = oracle_records(orc, name, paired, flags)
            figs[key] = figures_of(rec)
            mapped[key] = rec[0]["score"] > 0
            assert figs[key] == {k: runs[key][k] for k in figs[key]}, (key, figs[key])
            assert figs[key]["n_mapped"] == runs[key]["n_mapped_reference"]
        check_not_vacuous(name, figs)
        if name == "ladder":
            rungs = ladder_figures(mapped["ladder se: -mis 5"], mapped["ladder " + lci.MULTI_RUN])
            assert rungs == gold()["ladder"]["rungs"]
            assert check_ladder(rungs) == gold()["ladder"]["n_rungs_that_differ_between_max_dup_100_and_1000"]
    finally:
        orc.close()
