"""GPU suite (-m gpu): BAM made on the device (dg_batch_format_bam, dart_amd/csrc/dg_bamfmt.h and dg_bgzf.h).  The uncompressed records against the host
writer's bytes for the device's own SAM text (tests/native/bam_raw_checks.cpp), the BGZF blocks through an independent decoder (tests/bam_decode.py: zlib
inflates every block and checks CRC32 and ISIZE) against the reference's golden SAM."""
import ctypes as C
import gzip, os
import numpy as np
import pytest
import common, bam_decode
import sam_device_inputs as sdi
import bam_device_inputs as bdi
from dart_amd import host

pytestmark = pytest.mark.gpu
CASES = sorted(common.MANIFEST["cases"])
BLOCK = 0xFF00


@pytest.fixture(scope="module")
def ctxs(workdir):
    out = {}
    for name in CASES:
        c = common.build_case(name, workdir)
        ix = host.Index(c["prefix"])
        out[name] = (c, ix, host.DartGPU(ix))
    yield out
    for c, ix, gpu in out.values():
        gpu.close()


@pytest.fixture(scope="module")
def gpu(ctxs):
    return ctxs["pe101_spliced"][2]


def _text(n, seed=1):
    """English-like text: words of a small vocabulary in random order"""
    rng = np.random.default_rng(seed)
    words = [b"the", b"read", b"maps", b"to", b"chromosome", b"twenty", b"with", b"a", b"junction", b"and", b"its", b"mate", b"quality", b"of", b"alignment,", b"spliced.", b"score"]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + b" "
    return bytes(out[:n])


def _roundtrip(gpu, data: bytes):
    """compress on the device, inflate with zlib: content, block count, block sizes, the stored-form bound -> [(block's bytes, its compressed size)]"""
    z = gpu.bgzf_compress(data)
    blocks = bam_decode.bgzf_blocks(z)
    n_blocks = (len(data) + BLOCK - 1) // BLOCK
    assert b"".join(b for b, _ in blocks) == data
    assert len(blocks) == n_blocks and [len(b) for b, _ in blocks] == [min(BLOCK, len(data) - i * BLOCK) for i in range(n_blocks)]
    assert all(sz <= 65536 for _, sz in blocks) and len(z) <= len(data) + 31 * n_blocks
    return blocks, z


@pytest.mark.parametrize("n", [0, 1, 2, 3, 258, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7])
def test_bgzf_blocks_of_text_inflate_to_their_input(n, gpu):
    blocks, z = _roundtrip(gpu, _text(n))
    if n >= BLOCK - 1:
        assert len(z) < 0.8 * n, "text did not compress: %d of %d" % (len(z), n)


def test_bgzf_incompressible_block_is_stored_and_fits(gpu):
    data = np.random.default_rng(0).integers(0, 256, BLOCK, dtype=np.uint8).tobytes()
    blocks, z = _roundtrip(gpu, data)
    assert blocks[0][1] == BLOCK + 31


def test_bgzf_runs_and_repeats(gpu):
    blocks, z = _roundtrip(gpu, b"I" * BLOCK)                 # distance 1, runs of 258
    assert len(z) < 1000, len(z)                              # about BLOCK / 256 tokens of 18 bits; 3599 bytes if no match outgrew its 32-byte segment
    rng = np.random.default_rng(3)
    noise = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    phrase = _text(300, seed=9)
    far = {}
    for dist in (32768, 32769):                               # the farthest distance deflate has, and one beyond it
        _roundtrip(gpu, noise(100) + phrase + noise(dist - 300) + phrase + noise(50))
        piece = noise(300)                                    # (between zeros the far copy is the table's only candidate; between text the block is coded)
        blocks, z = _roundtrip(gpu, bytes(100) + piece + bytes(dist - 300) + piece + bytes(50))
        far[dist] = len(z)
        _roundtrip(gpu, _text(100, 2) + piece + _text(dist - 300, 3) + piece + _text(50, 4))
    assert far[32768] + 200 < far[32769], far               # the copy at 32768 was found and used, the one at 32769 could not be
    for k in (259, 600):                                      # repeats longer than one match
        piece = noise(k)
        _roundtrip(gpu, noise(10000) + piece + noise(9000) + piece + noise(77))
        _roundtrip(gpu, noise(1) + piece + piece)


def test_bgzf_repeats_on_the_kernels_seams(gpu):
    """repeats whose source, and whose destination, straddle the seams dg_bgzf_granules reports (the strip the match table lags by, the segment a lane
    codes), one byte before and one byte after them included"""
    strip, seg = gpu.bgzf_granules()
    assert strip > 0 and BLOCK > 2 * strip
    rng = np.random.default_rng(4)
    noise = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    seams = [strip, 2 * strip] + ([strip + seg, 3 * seg, strip - seg] if seg else [])
    for seam in seams:
        for shift in (-1, 0, 1):
            for length in (5, 40, 300):
                piece = noise(length)
                # source across the seam, destination later
                a = bytearray(_text(3 * strip + 500, seed=seam + shift))
                at = max(0, seam + shift - length // 2)
                a[at:at + length] = piece
                a[2 * strip + 700:2 * strip + 700 + length] = piece
                _roundtrip(gpu, bytes(a))
                # destination across the seam, source earlier
                b = bytearray(_text(3 * strip + 500, seed=seam + shift + 1))
                b[17:17 + length] = piece
                b[at:at + length] = piece
                _roundtrip(gpu, bytes(b))


def test_bgzf_is_deterministic(gpu, workdir):
    data = _text(3 * BLOCK + 7)
    first = gpu.bgzf_compress(data)
    assert gpu.bgzf_compress(data) == first
    # the kernel's bytes are those of its lane functions run on the host in the kernel's order (tests/native/bam_lane_checks.hip, the CPU suite's coder)
    assert bdi.host_deflate(workdir, data) == first
    mixed = b"I" * 700 + _text(20000, 5) + np.random.default_rng(6).integers(0, 256, 70000, dtype=np.uint8).tobytes() + _text(999, 7)
    assert bdi.host_deflate(workdir, mixed) == gpu.bgzf_compress(mixed)
    clone = gpu.clone()
    try:
        assert clone.bgzf_compress(data) == first
    finally:
        clone.close()


def _device_vs_host_writer(gpu, ix, workdir, tag, headers, quals, npm, unique=False, names=None):
    """raw records against the host writer's bytes for the device's own SAM text; counters; -> (raw, counters)"""
    text, ct_sam = gpu.format_sam(headers, quals, npm, unique_only=unique)
    raw, ct = gpu.format_bam(headers, quals, npm, unique_only=unique, raw=True)
    want, n_rec, n_refused = bdi.host_writer_bytes(workdir, tag, names or ix.names, text)
    assert raw == want, "%s: %d bytes against the host writer's %d" % (tag, len(raw), len(want))
    assert ct == dict(ct_sam, records=n_rec, refused=n_refused)
    assert gpu.bam_raw_bytes == len(raw)
    return raw, ct


def _decodes_to(ix, blocks: bytes, golden_text: str):
    _, refs, lines, _ = bam_decode.decode(bdi.bam_file(ix.names, ix.chr_len, blocks))
    want = bdi.golden_as_bam_stores_it(golden_text)
    assert len(lines) == len(want)
    for a, b in zip(lines, want):
        assert a == b, (a, b)


@pytest.mark.parametrize("name", CASES)
def test_device_bam_equals_the_host_writer_and_decodes_to_golden_sam(name, ctxs, workdir):
    c, ix, gpu = ctxs[name]
    so, rl, flat = host.pack_reads(c["reads"])
    paired = bool(c["spec"]["paired"])
    npm = len(c["reads"]) if paired else 0
    for run in c["runs"]:
        p, h = common.parse_flags(run["flags"])
        gpu.set_params(host.default_params(paired=int(paired), **p))
        gpu.map_batch(so, rl, flat)
        timings_before, counters_before = gpu.timings(), gpu.counters()
        raw, ct = _device_vs_host_writer(gpu, ix, workdir, "gpu_" + run["base"], c["headers"], c["quals"], npm, unique=h["unique"])
        z, ct2 = gpu.format_bam(c["headers"], c["quals"], npm, unique_only=h["unique"])
        assert ct2 == ct and gpu.bam_raw_bytes == len(raw) and gpu.bam_device_ms > 0
        n_blocks = (len(raw) + BLOCK - 1) // BLOCK
        assert len(z) <= len(raw) + 31 * n_blocks and len(z) < len(raw)
        assert b"".join(b for b, _ in bam_decode.bgzf_blocks(z)) == raw
        _decodes_to(ix, z, common.golden_sam(run["base"]))
        t = gpu.device_bam_tensor()
        assert t.numel() == len(z) and bytes(t.cpu().numpy().tobytes()) == z
        # SAM after BAM on the same batch; dg_last_timings and dg_last_counters still hold the batch's contents
        text, _ = gpu.format_sam(c["headers"], c["quals"], npm, unique_only=h["unique"])
        assert text == sdi.body_of(common.golden_sam(run["base"]))
        assert len(timings_before) > 3 and gpu.timings() == timings_before
        assert counters_before["seeds"] > 0 and gpu.counters() == counters_before


def test_device_bam_of_the_odd_character_reads(ctxs, workdir):
    c, ix, gpu = ctxs["pe101_spliced"]
    seqs = common.odd_character_reads(c["genome"])
    so, rl, flat = host.pack_reads(seqs)
    gpu.set_params(host.default_params(paired=0, max_mismatch=12))
    gpu.map_batch(so, rl, flat)
    headers = ["r%d" % i for i in range(len(seqs))]; quals = ["I" * len(s) for s in seqs]
    _device_vs_host_writer(gpu, ix, workdir, "gpu_odd", headers, quals, 0)
    z, _ = gpu.format_bam(headers, quals, 0)
    _decodes_to(ix, z, gzip.open(os.path.join(common.GOLDEN, "odd_characters.mis12.sam.gz"), "rt").read())


def test_device_bam_of_the_read_structures(ctxs, workdir):
    """the classes of tests/read_structures.py, paired, -mis 12 -m (several N in a CIGAR, long insertions, chains of one-base operations, improper and unpaired flags,
    mates of 14 to 101 bases): raw against the host writer, and the blocks decoded against the SAM the reference's object code wrote"""
    import read_structures as rs, read_structure_inputs as rsi
    c, ix, gpu = ctxs["pe101_spliced"]
    _, classes, _ = rsi.read_set("rs101", workdir)
    seqs = rs.as_reads(rs.all_pairs(classes)[0])
    so, rl, flat = host.pack_reads(seqs)
    p, _ = common.parse_flags(rsi.FIXTURE_FLAGS)
    gpu.set_params(host.default_params(paired=1, **p))
    gpu.map_batch(so, rl, flat)
    headers = ["p%d" % (i // 2) for i in range(len(seqs))]; quals = ["I" * len(s) for s in seqs]
    _device_vs_host_writer(gpu, ix, workdir, "gpu_read_structures", headers, quals, len(seqs))
    z, _ = gpu.format_bam(headers, quals, len(seqs))
    _decodes_to(ix, z, rsi.fixture_sam())


def test_device_bam_edge_input_through_the_kernels(ctxs, workdir):
    """sdi.edge_reads (a 1-base and a 1000-base read, a 5000-byte name, a NUL inside a quality, a quality longer than its read, 6 pairs + a single tail) on
    records of a real mapping, in the four flag combinations, raw against the host writer"""
    c, ix, gpu = ctxs["pe101_spliced"]
    seqs, headers, quals = sdi.edge_reads(c["genome"])
    so, rl, flat = host.pack_reads(seqs)
    for unique, multi, fasta in ((False, False, False), (True, False, False), (False, True, False), (True, True, True)):
        q = None if fasta else quals
        tag = "gpu_edge_%d%d%d" % (unique, multi, fasta)
        gpu.set_params(host.default_params(paired=1, max_mismatch=5, multi_hit=int(multi)))
        gpu.map_batch(so[:12], rl[:12], flat)
        _, ct = _device_vs_host_writer(gpu, ix, workdir, tag + "_pairs", headers[:12], None if fasta else quals[:12], 12, unique=unique)
        assert ct["refused"] > 0
        gpu.set_params(host.default_params(paired=0, max_mismatch=5, multi_hit=int(multi)))
        gpu.map_batch(so, rl, flat)                                  # n_pair_mode = n - 1: the last read left single
        raw, ct13 = _device_vs_host_writer(gpu, ix, workdir, tag + "_13", headers, q, 12, unique=unique)
        assert ct13["refused"] > 0 and ct13["records"] > 0 and b"N" * 255 not in raw
        z, _ = gpu.format_bam(headers, q, 12, unique_only=unique)
        assert b"".join(b for b, _ in bam_decode.bgzf_blocks(z)) == raw


def test_device_bam_does_not_depend_on_how_the_batch_is_split(ctxs):
    c, ix, gpu = ctxs["pe101_spliced"]
    n = len(c["reads"])
    p, _ = common.parse_flags(c["runs"][0]["flags"])
    gpu.set_params(host.default_params(paired=1, **p))
    def part(g, lo, hi, raw):
        so, rl, flat = host.pack_reads(c["reads"][lo:hi])
        g.map_batch(so, rl, flat)
        return g.format_bam(c["headers"][lo:hi], c["quals"][lo:hi], hi - lo, raw=raw)
    inflate = lambda z: b"".join(b for b, _ in bam_decode.bgzf_blocks(z))
    whole, ctw = part(gpu, 0, n, True)
    cut = (n // 2) & ~1
    a, cta = part(gpu, 0, cut, True); b, ctb = part(gpu, cut, n, True)
    assert a + b == whole and {k: cta[k] + ctb[k] for k in cta} == ctw
    za, _ = part(gpu, 0, cut, False); zb, _ = part(gpu, cut, n, False); zw, _ = part(gpu, 0, n, False)
    assert inflate(za) + inflate(zb) == whole == inflate(zw)
    clone = gpu.clone()
    try:
        clone.set_params(host.default_params(paired=1, **p))
        on_clone, ctc = part(clone, 0, n, True)
        assert on_clone == whole and ctc == ctw
        zc, _ = part(clone, 0, n, False)
        assert zc == zw                                           # the same input on a clone: the same compressed bytes
    finally:
        clone.close()
    for raw in (True, False):                                     # a batch of no reads: no bytes, no blocks
        empty, cte = part(gpu, 0, 0, raw)
        assert empty == b"" and set(cte.values()) == {0}


def test_device_bam_records_that_outgrow_their_first_buffer(ctxs, monkeypatch, workdir):
    """DG_BAM_FIRST_CAP makes a new context's first record buffer 1000 bytes: complete records can only come from the writing kernel's second launch"""
    c, ix, gpu = ctxs["pe101_spliced"]
    n = len(c["reads"])
    monkeypatch.setenv("DG_BAM_FIRST_CAP", "1000")
    small = gpu.clone()                                      # (a context reads its switches when it is created)
    monkeypatch.delenv("DG_BAM_FIRST_CAP")
    try:
        small.set_params(host.default_params(paired=1, max_mismatch=5, multi_hit=1))
        so, rl, flat = host.pack_reads(c["reads"])
        small.map_batch(so, rl, flat)
        for k in range(2):                                   # the second call finds the grown buffer
            raw, ct = _device_vs_host_writer(small, ix, workdir, "gpu_grow%d" % k, c["headers"], c["quals"], n)
            assert len(raw) > 100000
            z, _ = small.format_bam(c["headers"], c["quals"], n)
            assert b"".join(b for b, _ in bam_decode.bgzf_blocks(z)) == raw
    finally:
        small.close()


def test_device_bam_resident_form_equals_the_host_array_form(ctxs):
    c, ix, gpu = ctxs["pe101_spliced"]
    n = 600
    names = [("q%d" % (i // 2)).encode() for i in range(n)]
    seqs = [c["reads"][i].tobytes() for i in range(n)]
    quals = [bytes(33 + (5 * i + j) % 41 for j in range(len(seqs[i]))) for i in range(n)]
    # the two files of a paired library: mate 2 as the sequencer wrote it (the upload stores it reverse-complemented, its quality reversed)
    rc = lambda s: bytes({65: 84, 67: 71, 71: 67, 84: 65}.get(ch, 78) for ch in reversed(s))
    t1 = b"".join(b"@%s/1\n%s\n+\n%s\n" % (names[i], seqs[i], quals[i]) for i in range(0, n, 2))
    t2 = b"".join(b"@%s/2\n%s\n+\n%s\n" % (names[i], rc(seqs[i]), quals[i][::-1]) for i in range(1, n, 2))
    gpu.set_params(host.default_params(paired=1, max_mismatch=5))
    assert gpu.upload_fastq(t1, t2, rc_odd_reads=True) == n
    gpu.run()
    for raw in (True, False):
        res, ct = gpu.format_bam_resident(n, raw=raw)
        arr, ct2 = gpu.format_bam(names, quals, n, raw=raw)
        assert res == arr and ct == ct2 and ct["records"] >= n
    so, rl, flat = host.pack_reads(c["reads"][:n])
    gpu.map_batch(so, rl, flat)                               # an upload of arrays: nothing resident
    nb = C.c_size_t(7); nr = C.c_size_t(7); ct = (C.c_uint64 * 5)()
    rc_ = gpu.lib.dg_batch_format_bam_resident(gpu.ctx, n, 0, C.byref(nb), C.byref(nr), ct, None)
    assert rc_ == -3 and nb.value == 0 and nr.value == 0 and "dg_batch_upload_fastq" in (gpu.lib.dg_last_error(gpu.ctx) or b"").decode()


def test_device_bam_error_contract(ctxs):
    c, ix, gpu = ctxs["pe101_spliced"]
    lib = gpu.lib
    n = 200
    reads = c["reads"][:n]
    so, rl, flat = host.pack_reads(reads)
    ho, hb = host.flatten_strings(c["headers"][:n]); qo, qb = host.flatten_strings(c["quals"][:n])
    def call(ctx, hdr_off=ho, qual_off=qo, npm=n, flags=0):
        t = host.SamText(); t.hdr_off, t.hdr, t.qual_off, t.qual, t.n_pair_mode = hdr_off.ctypes.data, hb.ctypes.data, qual_off.ctypes.data, qb.ctypes.data, npm
        nb = C.c_size_t(12345); nr = C.c_size_t(12345); ct = (C.c_uint64 * 5)(9, 9, 9, 9, 9)
        rc = lib.dg_batch_format_bam(ctx, C.byref(t), flags, C.byref(nb), C.byref(nr), ct, None)
        if rc:
            assert nb.value == 0 and nr.value == 0 and list(ct) == [0] * 5
        return rc, int(nb.value), (lib.dg_last_error(ctx) or b"").decode()
    ARG, CAPACITY = -3, -4
    fresh = gpu.clone()                                       # no batch yet
    try:
        rc, nb, msg = call(fresh.ctx)
        assert rc == ARG and "dg_batch_format_bam" in msg and "no finished batch" in msg
        fresh.upload(so, rl, flat)                                # uploaded, not run
        rc, nb, msg = call(fresh.ctx)
        assert rc == ARG and "no finished batch" in msg
        fresh.set_params(host.default_params(paired=1, max_mismatch=5))
        fresh.run()
        rc, nb, msg = call(fresh.ctx, npm=n - 1)
        assert rc == ARG and "n_pair_mode" in msg
        rc, nb, msg = call(fresh.ctx, npm=n + 2)
        assert rc == ARG and "n_pair_mode" in msg
        bad = ho.copy(); bad[7] = bad[9] + 1
        rc, nb, msg = call(fresh.ctx, hdr_off=bad)
        assert rc == ARG and "hdr_off decreases" in msg
        badq = qo.copy(); badq[n] = 0
        rc, nb, msg = call(fresh.ctx, qual_off=badq)
        assert rc == ARG and "qual_off decreases" in msg
        assert lib.dg_batch_download_bam(fresh.ctx, None, 0) == ARG and "no BAM bytes" in (lib.dg_last_error(fresh.ctx) or b"").decode()
        rc, nb, msg = call(fresh.ctx)                             # and now it works: the errors above left the batch usable
        assert rc == 0 and nb > 0
        # a too-small buffer stays untouched, the text says the need
        buf = np.full(nb, 0xAB, np.uint8)
        rc = lib.dg_batch_download_bam(fresh.ctx, buf.ctypes.data, nb - 1)
        assert rc == CAPACITY and (buf == 0xAB).all() and str(nb) in (lib.dg_last_error(fresh.ctx) or b"").decode()
        assert lib.dg_batch_download_bam(fresh.ctx, buf.ctypes.data, nb) == 0 and bytes(buf[:4]) == b"\x1f\x8b\x08\x04"
        # dg_map_batch_compact: no full records to write
        rc_ = np.zeros(n, host.READ_C); pc_ = np.zeros(4 * n + 64, host.REPORT_C); cg_ = np.zeros(16 * n + 64, np.uint32); sj_ = np.zeros(n + 64, host.SJ_OUT)
        caps = (C.c_size_t * 3)(len(pc_), len(cg_), len(sj_)); used = (C.c_size_t * 3)()
        assert lib.dg_map_batch_compact(fresh.ctx, n, so.ctypes.data, rl.ctypes.data, flat.ctypes.data, 0, 0, None, None, 0,
                                        rc_.ctypes.data, pc_.ctypes.data, cg_.ctypes.data, sj_.ctypes.data, caps, used) == 0
        rc, nb, msg = call(fresh.ctx)
        assert rc == ARG and "full records" in msg and "packed" not in msg
        # packed reads: full records, but no ASCII copy of the reads
        words, nlist = host.pack_reads_2bit(np.where(reads == ord("N"), ord("N"), reads))
        fresh.map_batch_packed(words, nlist, reads.shape[1])
        rc, nb, msg = call(fresh.ctx)
        assert rc == ARG and "packed" in msg
        # dg_bgzf_compress needs no batch
        assert bam_decode.bgzf_blocks(fresh.bgzf_compress(b"no batch needed"))[0][0] == b"no batch needed"
    finally:
        fresh.close()
    # a context whose index never got names cannot format
    st = C.c_int(0); f = ix.files(0); pr = host.default_params(paired=1, max_mismatch=5)
    bare = lib.dg_init_files(C.byref(f), C.byref(pr), 0, 0, C.byref(st))
    assert bare
    try:
        assert lib.dg_batch_upload(bare, n, so.ctypes.data, rl.ctypes.data, flat.ctypes.data) == 0
        used = (C.c_size_t * 3)()
        assert lib.dg_batch_run(bare, used) == 0
        rc, nb, msg = call(bare)
        assert rc == ARG and "chromosome names" in msg
    finally:
        lib.dg_destroy(bare)
