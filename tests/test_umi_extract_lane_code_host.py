"""CPU suite: the host-callable rules of the inline UMI cut (dart_amd/csrc/dg_trim.h) through tests/native/umi_extract_checks.hip -- the slot, the partners, the
cut, the pairwise verdict, the letters and the name's suffix -- against the sequential twin of tests/umi_extract_inputs.py, for one text, an interleaved text and
two texts; and the twin itself: with the rule off it is the trimming twin, and the cut commutes with writing the cut reads back and trimming those."""
import pytest
import trim_inputs as ti
import umi_extract_inputs as uxi


def _reads():
    a = uxi.seam_reads(11, seed=3, n_fill=60, drop_at=(3, 17, 58))
    b = uxi.seam_reads(4, seed=4, n_fill=59, drop_at=(5, 18))[: len(a) - 1]
    inter = [r for pair in zip(a, b) for r in pair]
    return {"one_text": (ti.text_of(a), None, 0), "interleaved": (ti.text_of(inter) + ti.text_of(a[len(b):]), None, uxi.UMI_PAIRS), "two_texts": (ti.text_of(a, "/1"), ti.text_of(b, "/2"), 0)}


RULES = [uxi.umi(8, 4, 3, 0, b"_"), uxi.umi(6, 0, 0, 5, b"#"), uxi.umi(0, 21, 0, 0, b":"), uxi.umi(1, 0, 0, 0, b"_"), uxi.umi(10, 11, 60, 2, b"|")]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_rules_equal_the_twin(sanitize, workdir):
    exe = uxi.build_program(workdir, sanitize)
    for layout, (t1, t2, flags) in _reads().items():
        recs = ti.records(t1, t2)
        two = t2 is not None
        for j, rule in enumerate(RULES):
            u = dict(rule, flags=flags)
            got = uxi.run_program(exe, workdir, "%s_%d" % (layout, j), recs, u, two)
            kept, st, idx = uxi.batch(recs, ti.params(), u, two, False)
            assert len(got) == len(recs)
            assert [k for k, g in enumerate(got) if not g[3]] == idx                       # with every step off and min_len 1 the rule alone decides
            assert sum(g[1] for g in got if not g[2]) == st[14] and sum(g[3] for g in got) == st[15] and st[11] == st[12] == 0
            for (name, _, _), k in zip(kept, idx):
                assert name == recs[k][0] + got[k][5]
            for k, (h, s, q, f) in enumerate(recs):
                m = uxi.slot_of(k, f, two, u)
                assert got[k][:3] == (m, u["len"][m] + u["skip"][m], int(len(s) < u["len"][m] + u["skip"][m] + 1))
                assert got[k][4] == int((two or bool(flags)) and (k ^ 1) < len(recs))


def test_the_twin_without_the_rule_is_the_trimming_twin_and_the_cut_comes_first():
    p = ti.params(qual3=20, qual5=15, min_overlap=5, poly_mask=ti.poly_mask("GA"), poly_min=10, min_len=8, adapter=(ti.ADAPTER, ti.ADAPTER[:20]))
    for layout, (t1, t2, flags) in _reads().items():
        recs = ti.records(t1, t2)
        two, rc = t2 is not None, layout != "one_text"
        pp = dict(p, flags=ti.PAIRS if rc else 0)
        a, b = uxi.batch(recs, pp, None, two, rc), ti.trim_batch(recs, pp, two, rc)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[3] and a[1][14] == a[1][15] == 0
        # cutting first and trimming what is left (reads that pass the rule, their first u bases gone) gives the reads the combined twin gives
        u = uxi.umi(8, 4, 3, 0, b"_", flags)
        kept, st, idx = uxi.batch(recs, pp, u, two, rc)
        alone, _, idx0 = uxi.batch(recs, ti.params(), u, two, False)
        cut = [(h, s, q, recs[k][3]) for (h, s, q), k in zip(alone, idx0)]
        again, st2, _, idx2, _ = ti.trim_batch(cut, pp, two, rc)
        if all((k ^ 1) in idx0 or (k ^ 1) >= len(recs) for k in idx0) and (not rc or len(cut) % 2 == len(recs) % 2):      # (pairs stay side by side after the cut)
            assert again == kept and [idx0[k] for k in idx2] == idx and st2[3] == st[3]
