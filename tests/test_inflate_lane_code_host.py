"""CPU suite: the device inflater's code (dart_amd/csrc/dg_inflate.h: the member walker, the bit string, the Huffman tables, the token decode, the lanes'
copies, the CRC) compiled for the host (tests/native/inflate_checks.hip: a stand-alone program that runs a member as one wave of k_bgzf_inflate does, the
lanes of a phase one after the other in two orders) against zlib: the same bytes where zlib inflates, the rule zlib names where it refuses.  Every case runs in
a plain build and in one with the address and undefined-behaviour sanitizers, in which a member's input and output are heap blocks of their exact sizes."""
import zlib
import numpy as np
import pytest
import gz_device_inputs as gz
import fastq_device_inputs as fdi


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, workdir):
    exe = gz.build_program(workdir, sanitize=request.param == "sanitized")
    return lambda cases: gz.run_program(exe, workdir, cases)


def _same(res, want, label):
    assert res[0] == gz.OK, (label, res[0], res[1])
    assert res[2] == want, (label, len(res[2]), len(want))


def test_hand_made_valid_streams_inflate_to_zlibs_bytes(program):
    v = gz.valid_streams()
    names = list(v)
    for name, res in zip(names, program([gz.as_member(*v[n]) for n in names])):
        _same(res, v[name][1], name)
    # all of them as the members of one file
    whole = b"".join(gz.as_member(*v[n]) for n in names)
    _same(program([whole])[0], b"".join(v[n][1] for n in names), "all")


def test_hand_made_invalid_streams_break_the_rule_zlib_names(program):
    iv = gz.invalid_streams()
    names = list(iv)
    for name, res in zip(names, program([gz.as_member(iv[n][0], None) for n in names])):
        assert (res[0], res[1], res[2]) == (iv[name][1], 0, b""), (name, res[0], iv[name][1])
    # behind two good members: the index is the failing member's
    good = gz.bgzf(gz.fastq_like(900, 4), block=500)
    for name, res in zip(names, program([good + gz.as_member(iv[n][0], None) + good for n in names])):
        assert (res[0], res[1]) == (iv[name][1], 2), (name, res)


def test_files_the_walker_or_the_trailer_check_refuses(program):
    f = gz.invalid_files()
    names = list(f)
    for name, res in zip(names, program([f[n][0] for n in names])):
        assert (res[0], res[1]) == (f[name][1], f[name][2]), (name, res[:2], f[name][1:3])


def test_zlib_made_blocks_of_every_level_and_strategy(program):
    t = gz.fastq_like(3 * gz.BLOCK + 17)
    cases = [(gz.bgzf(t, level=lvl), t) for lvl in (0, 1, 6, 9)]
    cases += [(gz.bgzf(t, strategy=st), t) for st in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)]
    big = gz.fastq_like(65536, 5)
    cases.append((gz.member(gz.deflate_raw(big), big), big))
    part = t[:60000]
    cases.append((gz.member(gz.deflate_raw(part, 6, full_flush_at=(100, 100, 5000, 30000)), part), part))
    noise = np.random.default_rng(1).integers(0, 256, 100 * 1024, dtype=np.uint8).tobytes()
    cases += [(gz.bgzf(noise), noise), (gz.bgzf(b"A" * (200 * 1024)), b"A" * (200 * 1024)), (b"", b""), (gz.EOF_MEMBER, b"")]
    cases.append((gz.EOF_MEMBER + gz.bgzf(t[:1000], block=300) + gz.EOF_MEMBER + gz.bgzf(t[1000:2000], eof=True), t[:2000]))
    cases.append((gz.bgzf(t[:5000], block=700, extra_front=b"XY\x03\x00abc"), t[:5000]))
    a1, a2, inter = fdi.awkward_texts(fdi.random_reads(23, seed=5), fdi.random_reads(23, seed=6))
    cases += [(gz.bgzf(a1, block=b), a1) for b in (1, 7, 100)]
    for (blocks, want), res in zip(cases, program([c[0] for c in cases])):
        assert gz.bgzf_reference(blocks) == want
        _same(res, want, len(want))
