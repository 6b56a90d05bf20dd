"""CPU suite: the per-read code of the device's SAM formatter (dart_amd/csrc/dg_samfmt.h: decimal widths, a line's length, a line's fields into a byte
buffer) compiled for the host (tests/native/sam_checks.hip) and run read by read over the oracle's records of every golden case: the text must be the
reference's own SAM body byte for byte, the per-read lengths of pass 1 must add up to it, and the counters must be those of sam.Stats."""
import gzip, os
import numpy as np
import pytest
import common, oracle_py
import sam_device_inputs as sdi
from dart_amd import host, sam

CASES = sorted(common.MANIFEST["cases"])


def _check(workdir, tag, res, so, rl, flat, headers, quals, names, n_pair_mode, unique, multi, want_body=None, seqs=None):
    reads, rep, cig, _ = res
    exe = sdi.build_lane_program(workdir)
    path = os.path.join(workdir, "sam_batch_%s.bin" % tag)
    sdi.write_batch(path, reads, rep, cig, so, rl, flat, headers, quals, names, n_pair_mode, unique, multi)
    lens, ct, text = sdi.run_lane_program(exe, path)
    assert int(lens.sum()) == len(text)
    twin, st = sdi.twin_text(headers, seqs, quals, reads, rep, cig, names, n_pair_mode, multi=multi, unique=unique)
    assert text == twin, common.first_diff(text.decode("latin1"), twin.decode("latin1"))
    assert ct == [st.unmapped, st.unique, st.paired], (ct, st.unmapped, st.unique, st.paired)
    if want_body is not None:
        assert text == want_body, common.first_diff(text.decode("latin1"), want_body.decode("latin1"))
    return text


@pytest.mark.parametrize("name", CASES)
def test_lane_code_prints_the_reference_sam_of_every_golden_run(name, workdir):
    c = common.build_case(name, workdir)
    orc, ix = oracle_py.Oracle(c["prefix"]), host.Index(c["prefix"])
    so, rl, flat = host.pack_reads(c["reads"])
    paired = bool(c["spec"]["paired"])
    for run in c["runs"]:
        p, h = common.parse_flags(run["flags"])
        res = orc.map_batch(orc.params(paired=int(paired), **p), so, rl, flat, threads=4)
        text = _check(workdir, run["base"], res, so, rl, flat, c["headers"], c["quals"], ix.names, len(c["reads"]) if paired else 0, h["unique"], bool(p["multi_hit"]),
                      want_body=sdi.body_of(common.golden_sam(run["base"])), seqs=c["seqs"])
        if paired and c["spec"]["spliced"] > 0:         # the rules this exercises occur (asserted, not assumed)
            lines = text.decode("latin1").split("\n")
            assert any(l.split("\t")[6:7] == ["="] for l in lines), "no mate line"
            assert any(l.endswith(" XS:A:-") for l in lines) and any(l.endswith(" XS:A:+") for l in lines)
            assert any(l.split("\t")[2:3] == ["*"] for l in lines), "no unmapped line"
            stored = {hd: [] for hd in set(c["headers"])}
            for k, hd in enumerate(c["headers"]):
                stored[hd].append(c["seqs"][k])
            assert any(len(f) > 9 and f[2] != "*" and f[9] not in stored[f[0]] for f in (l.split("\t") for l in lines if l)), "no line printed the reverse complement of the stored read"


def test_lane_code_prints_the_reference_sam_of_the_odd_character_reads(workdir):
    c = common.build_case("pe101_spliced", workdir)
    orc, ix = oracle_py.Oracle(c["prefix"]), host.Index(c["prefix"])
    seqs = common.odd_character_reads(c["genome"])
    so, rl, flat = host.pack_reads(seqs)
    res = orc.map_batch(orc.params(paired=0, max_mismatch=12), so, rl, flat, threads=4)
    headers = ["r%d" % i for i in range(len(seqs))]
    quals = ["I" * len(s) for s in seqs]
    want = sdi.body_of(gzip.open(os.path.join(common.GOLDEN, "odd_characters.mis12.sam.gz"), "rt").read())
    _check(workdir, "odd", res, so, rl, flat, headers, quals, ix.names, 0, False, False, want_body=want, seqs=seqs)


def test_lane_code_prints_the_reference_sam_of_the_read_structures(workdir):
    """tests/read_structures.py's classes, paired, -mis 12 -m: several N in a CIGAR, long insertions, chains of one-base operations, improper and unpaired flags,
    mates of 14 to 101 bases"""
    import read_structures as rs, read_structure_inputs as rsi
    c, classes, _ = rsi.read_set("rs101", workdir)
    orc, ix = oracle_py.Oracle(c["prefix"]), host.Index(c["prefix"])
    seqs = rs.as_reads(rs.all_pairs(classes)[0])
    so, rl, flat = host.pack_reads(seqs)
    p, _ = common.parse_flags(rsi.FIXTURE_FLAGS)
    res = orc.map_batch(orc.params(paired=1, **p), so, rl, flat, threads=4)
    headers = ["p%d" % (i // 2) for i in range(len(seqs))]
    quals = ["I" * len(s) for s in seqs]
    _check(workdir, "read_structures", res, so, rl, flat, headers, quals, ix.names, len(seqs), False, True, want_body=sdi.body_of(rsi.fixture_sam()), seqs=seqs)


def _edge_records():
    """hand-made records for the edge batch (6 pairs + a single tail): several reports per read, both strands, a negative POS and negative distances,
    an unmapped mate, a low MAPQ for -unique, a long CIGAR that outgrows the writer's staging area"""
    R = np.zeros(13, host.READ_OUT); P = []; cig = []
    def report(aln, sj, flag, pidx, ch, bdir, pos, ops):
        P.append((aln, sj, flag, pidx, ch, bdir, pos, len(cig), len(ops))); cig.extend(ops)
    def read(k, score, sub, mis, mapq, best, reps):
        R[k]["score"], R[k]["sub_score"], R[k]["mis_num"], R[k]["mapq"], R[k]["best"] = score, sub, mis, mapq, best
        R[k]["rep_off"], R[k]["n_rep"] = len(P), len(reps)
        for r in reps:
            report(*r)
    M = lambda l: (l << 4)
    read(0, 101, 0, 0, 50, 0, [(101, -1, 99, 0, 0, 1, 1000, [M(101)]), (90, 0, 355, -1, 1, 0, 77, [M(50), (1200 << 4) | 3, M(51)])])
    read(1, 101, 0, 1, 50, 0, [(101, -1, 147, 0, 0, 0, 1200, [M(101)])])
    read(2, 1000, 10, 2, 50, 1, [(0, -1, 0, -1, 0, 1, 5, [M(1000)]), (1000, 1, 97, 0, 1, 1, -3, [M(400), (2 << 4) | 1, (7 << 4) | 2, M(598)])])
    read(3, 101, 0, 0, 50, 0, [(101, 2, 145, 1, 1, 1, 250, [(5 << 4) | 4, M(96)])])
    read(4, 80, 80, 3, 0, 0, [(80, 3, 65, 0, 0, 0, 500, [M(1)] * 150), (80, -1, 321, -1, 0, 1, 900, [M(101)])])
    read(5, 1, 0, 0, 2, 0, [(1, -1, 129, 0, 0, 0, 90000, [M(1)])])
    read(6, 0, 0, 0, 0, 0, [(0, -1, 77, -1, -1, 0, 0, [])])
    read(7, 0, 0, 0, 0, 0, [(0, -1, 141, -1, -1, 0, 0, [])])
    read(8, 101, 90, 0, 3, 0, [(101, -1, 73, 0, 0, 1, 10, [M(101)])])
    read(9, 0, 0, 0, 0, 0, [(0, -1, 133, -1, -1, 0, 0, [])])
    read(10, 60, 60, 1, 1, 0, [(0, -1, 0, -1, 0, 1, 1, [M(101)]), (60, 1, 99, 0, 1, 0, 4000000000, [M(101)])])
    read(11, 60, 0, 0, 50, 0, [(60, 0, 147, 1, 1, 0, 3999999000, [M(101)])])
    read(12, 101, 101, 0, 0, 0, [(50, -1, 0, -1, 0, 1, 3, [M(101)]), (101, 0, 16, -1, 1, 0, 20001, [M(101)]), (101, 1, 256, -1, 0, 1, 5, [M(101)])])
    return R, np.asarray(P, host.REPORT_OUT), np.asarray(cig, np.uint32)


@pytest.mark.parametrize("unique,multi,fasta", [(False, False, False), (True, False, False), (False, True, False), (True, True, True), (False, False, True)])
def test_lane_code_on_an_input_the_fixtures_do_not_hold(unique, multi, fasta, workdir):
    """a quality with a NUL in the middle, one longer than its read, FASTA, -unique, -m, a negative POS and negative distances, a POS beyond 32 bits, a 1-base and a 1000-base read, a 5000-byte name, a CIGAR of 150 ops, the last read of a paired batch left single -- against sam.format_records"""
    c = common.build_case("pe101_spliced", workdir)
    seqs, headers, quals = sdi.edge_reads(c["genome"])
    so, rl, flat = host.pack_reads(seqs)
    R, P, cig = _edge_records()
    text = _check(workdir, "edge_%d%d%d" % (unique, multi, fasta), (R, P, cig, None), so, rl, flat, headers, None if fasta else quals, ["chrA", "c" * 300], 12, unique, multi, seqs=seqs)
    lines = text.decode("latin1").split("\n")
    assert any(l.split("\t")[3:4] == ["-3"] for l in lines) and any(len(l.split("\t")) > 8 and l.split("\t")[8].startswith("-") for l in lines)
    assert lines[0].split("\t")[10] == ("*" if fasta else sdi.c_string(quals[0])) and (fasta or len(lines[0].split("\t")[10]) == 40)
    assert ("\tp4\t73\t" not in "\t" + text.decode("latin1").replace("\n", "\t")) == unique      # MAPQ 3 and below is hidden by -unique
