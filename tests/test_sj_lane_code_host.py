"""CPU suite: the host-callable code of the device's junction table (dart_amd/csrc/dg_sjtab.h: key words and their order, the hash and the probe
sequence, the chromosome look-up, a line's length and bytes) compiled for the host (tests/native/sj_checks.hip) and fed the oracle's tuples of every
golden run: its sorted entries and text must be the reference's junctions.tab byte for byte and equal the Python twin (sam.junction_twin)."""
import os
import numpy as np
import pytest
import common, oracle_py
import sj_device_inputs as sji
from dart_amd import host

CASES = sorted(common.MANIFEST["cases"])


def _check(workdir, tag, tuples, ix, slots=256, want_text=None):
    exe = sji.build_lane_program(workdir)
    path = os.path.join(workdir, "sj_in_%s.bin" % tag)
    sji.write_input(path, tuples, ix, slots)
    ent, text, lines, grown = sji.run_lane_program(exe, path)
    t_ent, t_text, t_lines = sji.twin(tuples, ix)
    assert text == t_text, common.first_diff(text.decode("latin1"), t_text.decode("latin1"))
    assert lines == t_lines and len(ent) == len(t_ent)
    for f in host.SJ_ENTRY.names:
        assert np.array_equal(ent[f], t_ent[f]), f
    if want_text is not None:
        assert text == want_text, common.first_diff(text.decode("latin1"), want_text.decode("latin1"))
    return ent, text, lines, grown


@pytest.mark.parametrize("name", CASES)
def test_lane_code_prints_the_reference_junction_table_of_every_golden_run(name, workdir):
    c = common.build_case(name, workdir)
    orc, ix = oracle_py.Oracle(c["prefix"]), host.Index(c["prefix"])
    so, rl, flat = host.pack_reads(c["reads"])
    paired = bool(c["spec"]["paired"])
    for run in c["runs"]:
        p, _ = common.parse_flags(run["flags"])
        sj = orc.map_batch(orc.params(paired=int(paired), **p), so, rl, flat, threads=4)[3]
        tuples = list(zip(sj["g1"].tolist(), sj["g2"].tolist()))
        ent, text, lines, grown = _check(workdir, run["base"], tuples, ix, want_text=common.golden_junctions(run["base"]).encode("latin1"))
        if c["spec"]["spliced"] > 0:                      # the case proves something: both strands, repeated keys, a table that grew from its smallest size
            assert lines > 0 and np.isin(sj["type"], (0, 2)).any() and np.isin(sj["type"], (1, 3)).any() and (ent["count"] > 1).any()
            assert grown > 0 or len(ent) <= 128
    orc.close()


def test_lane_code_on_keys_the_mapper_never_emits(workdir):
    c = common.build_case("pe101_spliced", workdir)
    ix = host.Index(c["prefix"])
    rows = sji.synthetic_keys(ix)
    ent, text, lines, _ = _check(workdir, "synthetic", rows, ix)
    keys = sji.boundary_keys(ix)
    by_g1 = {int(e["g1"]): int(e["chr"]) for e in ent}
    assert by_g1[keys[0]] == 0 and by_g1[keys[0] + 1] == 1                       # on a boundary key: its chromosome; one past it: the next
    assert by_g1[keys[-1]] == 0 and by_g1[keys[-1] + 1] == host.SJ_NO_CHR        # the last key, and one past it: no line
    assert by_g1[-1] == 0 and lines == int((ent["chr"] != host.SJ_NO_CHR).sum()) < len(ent)
    assert int(ent["g1"][0]) == -(1 << 62) and int(ent["g1"][-1]) == (1 << 62)   # signed order
    shown = text.decode().split("\n")
    assert any(l.endswith("\t%d" % sji.INT_MAX) for l in shown) and any(l.split("\t")[1:2] == ["0"] for l in shown)      # g1 = -1 prints position 0
    first = [e for e in ent if int(e["g1"]) == keys[0]]
    assert len(first) == 1 and int(first[0]["count"]) == 8                       # two rows with one key added up


def test_lane_code_growth_keeps_every_count(workdir):
    """5000 distinct keys, each twice, into the smallest table: several growths, every count 2"""
    c = common.build_case("se100", workdir)
    ix = host.Index(c["prefix"])
    rng = np.random.default_rng(5)
    g1 = rng.integers(0, 2 * int(ix.l_pac), 5000); g2 = rng.integers(-1000, 1 << 34, 5000)
    rows = list({(int(a), int(b)) for a, b in zip(g1, g2)})
    both = rows + rows
    rng.shuffle(both)
    ent, _, _, grown = _check(workdir, "growth", both, ix)
    assert grown >= 5 and len(ent) == len(rows) and (ent["count"] == 2).all()
