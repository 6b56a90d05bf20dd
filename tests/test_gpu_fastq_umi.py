"""GPU suite (-m gpu): inline UMIs cut inside the FASTQ upload (dg_set_umi, dart_amd/csrc/dg_trim.h) against the sequential twin of the definition
(tests/umi_extract_inputs.py): one text, an interleaved text and two texts; reads one base either side of the rule, remainders around a wave's 64 lanes, drops on
either side of a workgroup of the length kernel, a last read without a partner, N and lower case inside the UMI, the UMI together with every trimming step, the
two sums, and the error contract.  Every comparison is exact."""
import re
import pytest
import common
import trim_inputs as ti
import umi_extract_inputs as uxi
from dart_amd import host

pytestmark = pytest.mark.gpu
ARG = -3


@pytest.fixture(scope="module")
def ctx(workdir):
    c = common.build_case("se100", workdir)
    g = host.DartGPU(host.Index(c["prefix"]))
    yield g
    g.close()


@pytest.fixture()
def gpu(ctx):
    ctx.set_trim(off=True); ctx.set_umi(off=True)
    yield ctx
    ctx.set_trim(off=True); ctx.set_umi(off=True)


def _batch(g):
    so, rl, flat, names, quals = g.download_reads()
    raw = flat.tobytes()
    return [(names[k], raw[int(so[k]):int(so[k]) + int(rl[k])], quals[k]) for k in range(len(rl))]


def _set_trim(g, p):
    g.set_trim(adapter=p["adapter"][0], adapter2=p["adapter"][1], qual3=p["qual3"], qual5=p["qual5"], qual_base=p["qual_base"], min_overlap=p["min_overlap"],
               max_err_permille=p["max_err_permille"], poly_mask=p["poly_mask"], poly_min=p["poly_min"], min_len=p["min_len"], flags=p["flags"])


def _against_the_twin(g, t1, t2, rc_odd, p, u):
    """p None: dg_set_umi alone (the twin then takes every step off and min_len 1)"""
    if p is not None:
        _set_trim(g, p)
    g.set_umi(u["len"][0], u["len"][1], u["skip"][0], u["skip"][1], u["sep"], flags=u["flags"])
    want, stats, idx = uxi.batch(ti.records(t1, t2), p if p is not None else ti.params(), u, t2 is not None, rc_odd)
    assert g.upload_fastq(t1, t2, rc_odd_reads=rc_odd) == len(want)
    got = _batch(g)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a, b)
    assert g.trim_stats() == stats
    return want, stats, idx


def _layouts(reads1, reads2):
    """(text1, text2, flags of the rule, reads are pairs) for one text, an interleaved text and two texts"""
    inter = [r for pair in zip(reads1, reads2) for r in pair]
    return {"one_text": (ti.text_of(reads1), None, 0), "interleaved": (ti.text_of(inter) + ti.text_of(reads1[len(reads2):]), None, uxi.UMI_PAIRS),
            "two_texts": (ti.text_of(reads1, "/1"), ti.text_of(reads2, "/2"), 0)}


@pytest.mark.parametrize("layout", ["one_text", "interleaved", "two_texts"])
@pytest.mark.parametrize("with_trim", [False, True], ids=["umi_alone", "umi_and_every_step"])
def test_the_cut_the_names_and_the_sums_against_the_twin(layout, with_trim, gpu):
    g0 = gpu.trim_granules()[0]
    n_fill = g0 + 40
    drops = (3, g0 - 9, g0 - 8, g0 - 7, n_fill - 2)               # with the 8 seam reads in front: a drop on each side of the length kernel's workgroup edge
    reads1 = uxi.seam_reads(11, seed=3, n_fill=n_fill, drop_at=drops)
    reads2 = uxi.seam_reads(4, seed=4, n_fill=n_fill - 1, drop_at=(5, g0 - 8))[: len(reads1) - 1]      # one read fewer: the last read of text 1 has no partner
    t1, t2, flags = _layouts(reads1, reads2)[layout]
    u = uxi.umi(8, 4, 3, 0, b"_", flags)
    p = ti.params(qual3=20, qual5=15, min_overlap=5, poly_mask=ti.poly_mask("GA"), poly_min=10, min_len=8, adapter=(ti.ADAPTER, ti.ADAPTER[:20]),
                  flags=ti.PAIRS if layout != "one_text" else 0) if with_trim else None
    want, st, idx = _against_the_twin(gpu, t1, t2, layout != "one_text", p, u)
    assert st[14] > 0 and st[15] >= len(drops) and st[1] == len(want) < st[0]
    names = [n for n, _, _ in want]
    if layout == "one_text":
        assert all(re.fullmatch(rb".*_[ACGTN]{8}", n) for n in names) and b"n_and_lower_ANCGTNNN" in names
        assert (b"len12_" + uxi.letters(reads1[2][1], 8) in names) == (not with_trim) and not any(n.startswith(b"len11_") or n.startswith(b"len10_") for n in names)       # L = u + 1 passes the rule (and then fails min_len 8), u and u - 1 fail it
    else:
        paired = [n for n in names if re.fullmatch(rb".*_[ACGTN]{12}", n)]
        assert len(paired) == len(names) - 1 and len(paired) % 2 == 0
        assert all(names[k][-13:] == names[k + 1][-13:] for k in range(0, len(paired), 2))          # partners are kept or dropped together and carry one suffix
        alone = [n for n in names if not re.fullmatch(rb".*_[ACGTN]{12}", n)]
        assert len(alone) <= 1 and all(re.fullmatch(rb".*_[ACGTN]{8}", n) for n in alone)          # the last read without a partner carries its own letters
        assert (len(ti.records(t1, t2)) - 1) in idx and len(alone) == 1
    # the rule off again: today's bytes, and the two sums are zero
    gpu.set_umi(off=True)
    if p is not None:
        want0, st0, _, _, _ = ti.trim_batch(ti.records(t1, t2), p, t2 is not None, layout != "one_text")
        assert gpu.upload_fastq(t1, t2, rc_odd_reads=layout != "one_text") == len(want0)
        assert _batch(gpu) == want0 and gpu.trim_stats() == st0 and st0[14] == st0[15] == 0
    else:
        n = gpu.upload_fastq(t1, t2, rc_odd_reads=layout != "one_text")
        assert n == len(ti.records(t1, t2)) and gpu.trim_stats() == [0] * 16


def test_slot_one_without_letters_and_a_linker_alone(gpu):
    reads1 = uxi.seam_reads(6, seed=7, n_fill=20)
    reads2 = uxi.seam_reads(5, seed=8, n_fill=20)
    t1, t2 = ti.text_of(reads1, "/1"), ti.text_of(reads2, "/2")
    want, st, _ = _against_the_twin(gpu, t1, t2, True, None, uxi.umi(6, 0, 0, 5, b"#", 0))       # mate 2 gives no letters but loses a linker of 5
    assert all(re.fullmatch(rb".*#[ACGTN]{6}", n) for n, _, _ in want) and st[14] > 0
    want, st, _ = _against_the_twin(gpu, t1, t2, True, None, uxi.umi(0, 21, 0, 0, b":", 0))      # 21 letters from mate 2 alone
    assert all(re.fullmatch(rb".*:[ACGTN]{21}", n) for n, _, _ in want)


def test_argument_errors_leave_the_setting_as_it_was(gpu):
    reads = uxi.seam_reads(8, seed=9, n_fill=10)
    t1 = ti.text_of(reads)
    want, st, _ = _against_the_twin(gpu, t1, None, False, None, uxi.umi(8, 0, 0, 0, b"_", 0))

    def refused(**kw):
        with pytest.raises(RuntimeError) as x:
            gpu.set_umi(**kw)
        m = re.search(r"failed \((-?\d+)\): (.*)", str(x.value), re.S)
        assert int(m.group(1)) == ARG and m.group(2).startswith("dg_set_umi: "), str(x.value)
    refused(len1=8, flags=2); refused(len1=0, len2=0); refused(len1=11, len2=11); refused(len1=8, skip1=100000); refused(len2=8, skip2=100000)
    for sep in (b"\0", b" ", b"\t", b"/", b"A", b"C", b"G", b"T", b"N", b"+", b"-"):
        refused(len1=8, sep=sep)
    assert gpu.upload_fastq(t1, None) == len(want) and _batch(gpu) == want and gpu.trim_stats() == st
