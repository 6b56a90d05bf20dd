"""GPU suite (-m gpu): the dynamic-Huffman mode of the device's BGZF coder (k_bgzf_deflate_dyn, dart_amd/csrc/dg_bgzf_dyn.h) through dg_bgzf_compress_flags
and DG_BAM_DYNAMIC.  The kernel's bytes are those of its lane functions run on the host in the kernel's order (tests/native/bgzf_dyn_checks.hip), which
carries the host run's fork counters and its watch over the slot to the device; every stream is inflated by zlib as well (tests/bam_decode.py)."""
import ctypes as C
import gzip, os
import numpy as np
import pytest
import common, bam_decode
import bam_device_inputs as bdi
import bgzf_dyn_inputs as dyn
from dart_amd import host

pytestmark = pytest.mark.gpu
BLOCK = dyn.BLOCK


@pytest.fixture(scope="module")
def case(workdir):
    c = common.build_case("pe101_spliced", workdir)
    ix = host.Index(c["prefix"])
    gpu = host.DartGPU(ix)
    yield c, ix, gpu
    gpu.close()


@pytest.fixture(scope="module")
def gpu(case):
    return case[2]


def _equals_host_lane_code(gpu, workdir, data):
    z = gpu.bgzf_compress(data, dynamic=True)
    want, ct = dyn.host_deflate_dyn(workdir, data)
    assert z == want, "%d bytes against the host lane code's %d" % (len(z), len(want))
    assert b"".join(b for b, _ in bam_decode.bgzf_blocks(z)) == data
    return z, ct


@pytest.mark.parametrize("n", [0, 1, 3, dyn.STRIP + 5, BLOCK, BLOCK + 1, 3 * BLOCK + 7])
def test_kernel_equals_the_host_lane_code_on_text(n, gpu, workdir):
    z, ct = _equals_host_lane_code(gpu, workdir, dyn.text(n))
    assert (z == b"") == (n == 0) and ct["blocks"] == (n + BLOCK - 1) // BLOCK
    if n >= dyn.STRIP:
        assert ct["dynamic"] >= n // dyn.STRIP - 1 and len(z) < 0.8 * len(gpu.bgzf_compress(dyn.text(n)))


def test_kernel_equals_the_host_lane_code_on_the_edge_alphabets(gpu, workdir):
    seen = {}
    for name, data in dyn.edge_alphabets().items():
        z, seen[name] = _equals_host_lane_code(gpu, workdir, data)
    assert seen["one_value"]["onedist"] == 1 and seen["four_values"]["nodist"] == 1 and seen["noise"]["stored"] == 1 and seen["words_then_noise"]["stored"] == 1


def test_dynamic_mode_is_deterministic(gpu):
    data = dyn.text(3 * BLOCK + 7, seed=2)
    first = gpu.bgzf_compress(data, dynamic=True)
    assert gpu.bgzf_compress(data, dynamic=True) == first
    assert gpu.bgzf_compress(data[:2 * BLOCK], dynamic=True) + gpu.bgzf_compress(data[2 * BLOCK:], dynamic=True) == first
    clone = gpu.clone()
    try:
        assert clone.bgzf_compress(data, dynamic=True) == first
    finally:
        clone.close()


def test_fixed_mode_is_unchanged(gpu, workdir):
    data = dyn.text(BLOCK + 7000, seed=4) + b"I" * 700 + np.random.default_rng(6).integers(0, 256, 9000, dtype=np.uint8).tobytes()
    z = gpu.bgzf_compress(data)
    assert z == bdi.host_deflate(workdir, data)
    nb = C.c_size_t(0)
    a = np.frombuffer(data + b"\0", np.uint8)
    assert gpu.lib.dg_bgzf_compress_flags(gpu.ctx, a.ctypes.data, len(data), 0, C.byref(nb), None) == 0 and nb.value == len(z)


def test_length_probe_equals_the_host_builder(gpu, workdir):
    for name, limit, freq in dyn.histograms():
        want, repaired = dyn.host_lengths(workdir, freq, limit)
        assert gpu.probe_huff_lengths(freq, limit) == want, name
        assert max(want) <= limit and (repaired == 1) == name.startswith("fib")


def _decodes_to(ix, blocks: bytes, golden_text: str):
    _, refs, lines, _ = bam_decode.decode(bdi.bam_file(ix.names, ix.chr_len, blocks))
    want = bdi.golden_as_bam_stores_it(golden_text)
    assert len(lines) == len(want)
    for a, b in zip(lines, want):
        assert a == b, (a, b)


def _both_modes(gpu, headers, quals, npm, unique=False):
    raw, ct_raw = gpu.format_bam(headers, quals, npm, unique_only=unique, raw=True, dynamic=True)      # (DG_BAM_DYNAMIC is ignored beside DG_BAM_RAW)
    fixed, ct_fixed = gpu.format_bam(headers, quals, npm, unique_only=unique)
    n_raw_fixed = gpu.bam_raw_bytes
    z, ct = gpu.format_bam(headers, quals, npm, unique_only=unique, dynamic=True)
    assert ct == ct_fixed == ct_raw and gpu.bam_raw_bytes == n_raw_fixed == len(raw) and gpu.bam_device_ms > 0
    assert b"".join(b for b, _ in bam_decode.bgzf_blocks(z)) == raw
    assert len(z) < len(fixed)
    return z, raw


def test_dynamic_bam_of_a_golden_paired_case(case, workdir):
    c, ix, gpu = case
    so, rl, flat = host.pack_reads(c["reads"])
    run = c["runs"][0]
    p, h = common.parse_flags(run["flags"])
    gpu.set_params(host.default_params(paired=1, **p))
    gpu.map_batch(so, rl, flat)
    z, raw = _both_modes(gpu, c["headers"], c["quals"], len(c["reads"]), unique=h["unique"])
    _decodes_to(ix, z, common.golden_sam(run["base"]))
    assert z == dyn.host_deflate_dyn(workdir, raw)[0]


def test_dynamic_bam_of_the_odd_character_reads(case):
    c, ix, gpu = case
    seqs = common.odd_character_reads(c["genome"])
    so, rl, flat = host.pack_reads(seqs)
    gpu.set_params(host.default_params(paired=0, max_mismatch=12))
    gpu.map_batch(so, rl, flat)
    headers = ["r%d" % i for i in range(len(seqs))]; quals = ["I" * len(s) for s in seqs]
    z, raw = _both_modes(gpu, headers, quals, 0)
    _decodes_to(ix, z, gzip.open(os.path.join(common.GOLDEN, "odd_characters.mis12.sam.gz"), "rt").read())


def test_dynamic_bam_resident_form_equals_the_host_array_form(case):
    c, ix, gpu = case
    n = 600
    names = [("q%d" % (i // 2)).encode() for i in range(n)]
    seqs = [c["reads"][i].tobytes() for i in range(n)]
    quals = [bytes(33 + (5 * i + j) % 41 for j in range(len(seqs[i]))) for i in range(n)]
    rc = lambda s: bytes({65: 84, 67: 71, 71: 67, 84: 65}.get(ch, 78) for ch in reversed(s))
    t1 = b"".join(b"@%s/1\n%s\n+\n%s\n" % (names[i], seqs[i], quals[i]) for i in range(0, n, 2))
    t2 = b"".join(b"@%s/2\n%s\n+\n%s\n" % (names[i], rc(seqs[i]), quals[i][::-1]) for i in range(1, n, 2))
    gpu.set_params(host.default_params(paired=1, max_mismatch=5))
    assert gpu.upload_fastq(t1, t2, rc_odd_reads=True) == n
    gpu.run()
    res, ct = gpu.format_bam_resident(n, dynamic=True)
    arr, ct2 = gpu.format_bam(names, quals, n, dynamic=True)
    fixed, _ = gpu.format_bam_resident(n)
    assert res == arr and ct == ct2 and ct["records"] >= n and len(res) < len(fixed)


def test_unknown_flag_bits_are_refused(gpu):
    data = dyn.text(5000)
    a = np.frombuffer(data + b"\0", np.uint8)
    for flags in (2, 4, 0x80000000, 3):
        nb = C.c_size_t(777); ms = C.c_float(7)
        assert gpu.lib.dg_bgzf_compress_flags(gpu.ctx, a.ctypes.data, len(data), flags, C.byref(nb), C.byref(ms)) == -3
        assert nb.value == 0 and ms.value == 0 and "flag" in (gpu.lib.dg_last_error(gpu.ctx) or b"").decode()
        assert gpu.lib.dg_batch_download_bam(gpu.ctx, None, 0) == -3         # no result was left behind
    z = gpu.bgzf_compress(data, dynamic=True)                     # the context stays usable
    assert bam_decode.bgzf_blocks(z)[0][0] == data


def test_phase_probe_leaves_the_bytes_alone(gpu):
    """dg_probe_bgzf_phases switches the kernel's clocks on: the same stream, and a count for every phase"""
    data = dyn.text(2 * BLOCK + 999, seed=6)
    cycles, z = gpu.probe_bgzf_phases(data)
    assert z == gpu.bgzf_compress(data, dynamic=True)
    assert list(cycles) == list(gpu.BGZF_PHASES) and all(v > 0 for v in cycles.values()), cycles
    assert gpu.lib.dg_probe_bgzf_phases(gpu.ctx, None, 5, None, None, None) == -3
