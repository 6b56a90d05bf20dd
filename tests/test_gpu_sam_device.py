"""GPU suite (-m gpu): SAM text formatted on the device (dg_batch_format_sam, dart_amd/csrc/dg_samfmt.h) against the reference's golden SAM, the Python
twin (dart_amd/sam.py::format_records) and, at full size, the host formatter of the `dart` command line."""
import ctypes as C
import gzip, hashlib, os, subprocess
import numpy as np
import pytest
import common
import sam_device_inputs as sdi
from dart_amd import host, synth

pytestmark = pytest.mark.gpu
CASES = sorted(common.MANIFEST["cases"])


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


def _same(got: bytes, want: bytes):
    assert got == want, common.first_diff(got.decode("latin1"), want.decode("latin1"))


@pytest.mark.parametrize("name", CASES)
def test_device_sam_equals_golden_sam_and_the_python_twin(name, ctxs):
    c, ix, gpu = ctxs[name]
    so, rl, flat = host.pack_reads(c["reads"])
    paired = bool(c["spec"]["paired"])
    npm = len(c["reads"]) if paired else 0
    for run in c["runs"]:
        p, h = common.parse_flags(run["flags"])
        gpu.set_params(host.default_params(paired=int(paired), **p))
        res = gpu.map_batch(so, rl, flat)
        timings_before, counters_before = gpu.timings(), gpu.counters()
        text, ct = gpu.format_sam(c["headers"], c["quals"], npm, unique_only=h["unique"])
        _same(text, sdi.body_of(common.golden_sam(run["base"])))
        twin, st = sdi.twin_text(c["headers"], c["seqs"], c["quals"], res.reads, res.reports, res.cigar, ix.names, npm, multi=bool(p["multi_hit"]), unique=h["unique"])
        _same(text, twin)
        assert ct == dict(unmapped=st.unmapped, unique=st.unique, paired=st.paired)
        assert gpu.sam_device_ms > 0
        t = gpu.device_sam_tensor()
        assert t.numel() == len(text) and bytes(t.cpu().numpy().tobytes()) == text
        # dg_last_timings and dg_last_counters still hold the batch's contents
        assert len(timings_before) > 3 and gpu.timings() == timings_before
        assert counters_before["seeds"] > 0 and gpu.counters() == counters_before


def test_device_sam_of_the_odd_character_reads(ctxs):
    c, ix, gpu = ctxs["pe101_spliced"]
    seqs = common.odd_character_reads(c["genome"])
    so, rl, flat = host.pack_reads(seqs)
    gpu.set_params(host.default_params(paired=0, max_mismatch=12))
    res = gpu.map_batch(so, rl, flat)
    headers = ["r%d" % i for i in range(len(seqs))]; quals = ["I" * len(s) for s in seqs]
    text, ct = gpu.format_sam(headers, quals, 0)
    _same(text, sdi.body_of(gzip.open(os.path.join(common.GOLDEN, "odd_characters.mis12.sam.gz"), "rt").read()))
    twin, st = sdi.twin_text(headers, seqs, quals, res.reads, res.reports, res.cigar, ix.names, 0)
    _same(text, twin)
    assert ct == dict(unmapped=st.unmapped, unique=st.unique, paired=st.paired)


def test_device_sam_of_the_read_structures(ctxs, workdir):
    """the classes of tests/read_structures.py, paired, -mis 12 -m: CIGARs with several N, insertions of up to 30 bases, chains of one-base operations, improper and
    unpaired flags, mates of 14 to 101 bases -- against the SAM the reference's object code wrote for them"""
    import read_structures as rs, read_structure_inputs as rsi
    c, ix, gpu = ctxs["pe101_spliced"]
    _, classes, _ = rsi.read_set("rs101", workdir)
    seqs = rs.as_reads(rs.all_pairs(classes)[0])
    so, rl, flat = host.pack_reads(seqs)
    p, _ = common.parse_flags(rsi.FIXTURE_FLAGS)
    gpu.set_params(host.default_params(paired=1, **p))
    res = gpu.map_batch(so, rl, flat)
    headers = ["p%d" % (i // 2) for i in range(len(seqs))]; quals = ["I" * len(s) for s in seqs]
    text, ct = gpu.format_sam(headers, quals, len(seqs))
    _same(text, sdi.body_of(rsi.fixture_sam()))
    twin, st = sdi.twin_text(headers, seqs, quals, res.reads, res.reports, res.cigar, ix.names, len(seqs), multi=True)
    _same(text, twin)
    assert ct == dict(unmapped=st.unmapped, unique=st.unique, paired=st.paired)


def test_device_sam_does_not_depend_on_how_the_batch_is_split(ctxs):
    c, ix, gpu = ctxs["pe101_spliced"]
    n = len(c["reads"])
    p, _ = common.parse_flags(c["runs"][0]["flags"])
    gpu.set_params(host.default_params(paired=1, **p))
    def part(g, lo, hi):
        so, rl, flat = host.pack_reads(c["reads"][lo:hi])
        g.map_batch(so, rl, flat)
        return g.format_sam(c["headers"][lo:hi], c["quals"][lo:hi], hi - lo)
    whole, ctw = part(gpu, 0, n)
    cut = (n // 2) & ~1
    a, cta = part(gpu, 0, cut); b, ctb = part(gpu, cut, n)
    assert a + b == whole and {k: cta[k] + ctb[k] for k in cta} == ctw
    clone = gpu.clone()
    clone.set_params(host.default_params(paired=1, **p))
    on_clone, ctc = part(clone, 0, n)
    assert on_clone == whole and ctc == ctw
    # a batch of no reads: no bytes, DG_OK
    empty, cte = part(gpu, 0, 0)
    assert empty == b"" and cte == dict(unmapped=0, unique=0, paired=0)


def test_device_sam_text_that_outgrows_its_first_buffer(ctxs, monkeypatch):
    """the text buffer's first size is a guess; when the text is larger k_sam_write writes nothing, the buffer grows to the scanned total and that kernel
    alone runs again.  DG_SAM_TEXT_FIRST_CAP makes a new context's first buffer 1000 bytes: a complete text can only come from the second launch."""
    c, ix, gpu = ctxs["pe101_spliced"]
    n = len(c["reads"])
    monkeypatch.setenv("DG_SAM_TEXT_FIRST_CAP", "1000")
    small = gpu.clone()                                      # (a context reads its switches when it is created)
    monkeypatch.delenv("DG_SAM_TEXT_FIRST_CAP")
    small.set_params(host.default_params(paired=1, max_mismatch=5, multi_hit=1))
    so, rl, flat = host.pack_reads(c["reads"])
    res = small.map_batch(so, rl, flat)
    for _ in range(2):                                       # the second call finds the grown buffer
        text, ct = small.format_sam(c["headers"], c["quals"], n)
        twin, st = sdi.twin_text(c["headers"], c["seqs"], c["quals"], res.reads, res.reports, res.cigar, ix.names, n, multi=True)
        assert len(twin) > 100000
        _same(text, twin)
        assert ct == dict(unmapped=st.unmapped, unique=st.unique, paired=st.paired)


def test_device_sam_fields_too_long_for_the_staging_area(ctxs):
    """chromosome names of 300 bytes: FLAG..TLEN of every mapped line exceed the 192 bytes of LDS k_sam_write stages them in, so lane 0 writes them straight
    to the text (the plain path) while the other lanes copy the name in front of them; an index of its own, so no other test sees these names"""
    c, ix, _ = ctxs["pe101_spliced"]
    gpu = host.DartGPU(ix, host.default_params(paired=1, max_mismatch=5, multi_hit=1))
    try:
        names = [("%s_" % nm) + "x" * 300 for nm in ix.names]
        gpu.set_chr_names(names)
        n = len(c["reads"])
        so, rl, flat = host.pack_reads(c["reads"])
        res = gpu.map_batch(so, rl, flat)
        headers = [h if k % 3 else h + "y" * (k % 200) for k, h in enumerate(c["headers"])]      # names of many lengths in front of the fields
        headers[1::2] = headers[0::2]
        text, ct = gpu.format_sam(headers, c["quals"], n)
        twin, st = sdi.twin_text(headers, c["seqs"], c["quals"], res.reads, res.reports, res.cigar, names, n, multi=True)
        _same(text, twin)
        assert text.count(b"x" * 300) > n // 2
    finally:
        gpu.close()


def test_device_sam_error_contract(ctxs, workdir):
    c, ix, gpu = ctxs["pe101_spliced"]
    lib = gpu.lib
    n = 200
    reads = c["reads"][:n]
    so, rl, flat = host.pack_reads(reads)
    ho, hb = host.flatten_strings(c["headers"][:n]); qo, qb = host.flatten_strings(c["quals"][:n])
    def call(ctx, hdr_off=ho, qual_off=qo, npm=n):
        t = host.SamText(); t.hdr_off, t.hdr, t.qual_off, t.qual, t.n_pair_mode = hdr_off.ctypes.data, hb.ctypes.data, qual_off.ctypes.data, qb.ctypes.data, npm
        nb = C.c_size_t(12345); ct = (C.c_uint64 * 3)()
        rc = lib.dg_batch_format_sam(ctx, C.byref(t), 0, C.byref(nb), ct, None)
        return rc, int(nb.value), (lib.dg_last_error(ctx) or b"").decode()
    ARG, CAPACITY = -3, -4
    fresh = gpu.clone()                                       # no batch yet
    rc, nb, msg = call(fresh.ctx)
    assert rc == ARG and "no finished batch" in msg and nb == 0
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
    rc, nb, msg = call(fresh.ctx)                             # and now it works: the errors above left the batch usable
    assert rc == 0 and nb > 0
    # a too-small buffer stays untouched, the text says the need
    buf = np.full(nb, 0xAB, np.uint8)
    rc = lib.dg_batch_download_sam(fresh.ctx, buf.ctypes.data, nb - 1)
    assert rc == CAPACITY and (buf == 0xAB).all() and str(nb) in (lib.dg_last_error(fresh.ctx) or b"").decode()
    assert lib.dg_batch_download_sam(fresh.ctx, buf.ctypes.data, nb) == 0 and buf[-1] == 10
    # dg_map_batch_compact with ASCII reads: the bases are in HBM, but the units k_pair finished have no full records to print
    rc_ = np.zeros(n, host.READ_C); pc_ = np.zeros(4 * n + 64, host.REPORT_C); cg_ = np.zeros(16 * n + 64, np.uint32); sj_ = np.zeros(n + 64, host.SJ_OUT)
    caps = (C.c_size_t * 3)(len(pc_), len(cg_), len(sj_)); used = (C.c_size_t * 3)()
    assert lib.dg_map_batch_compact(fresh.ctx, n, so.ctypes.data, rl.ctypes.data, flat.ctypes.data, 0, 0, None, None, 0,
                                    rc_.ctypes.data, pc_.ctypes.data, cg_.ctypes.data, sj_.ctypes.data, caps, used) == 0
    rc, nb, msg = call(fresh.ctx)
    assert rc == ARG and nb == 0 and "full records" in msg and "packed" not in msg
    # packed reads: full records, but no ASCII copy of the reads
    words, nlist = host.pack_reads_2bit(np.where(reads == ord("N"), ord("N"), reads))
    fresh.map_batch_packed(words, nlist, reads.shape[1])
    rc, nb, msg = call(fresh.ctx)
    assert rc == ARG and nb == 0 and "packed" in msg
    # chromosome names: the wrong count is refused; a context whose index never got names cannot format
    off, flat_names = host.flatten_strings(ix.names + ["extra"])
    assert lib.dg_set_chr_names(gpu.ctx, len(ix.names) + 1, off.ctypes.data, flat_names.ctypes.data) == ARG
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


def test_device_sam_edge_input_through_the_kernels(ctxs):
    """the CPU test's edge names, qualities and read lengths (a 1-base and a 1000-base read, a 5000-byte name, a NUL inside a quality, a quality longer
    than its read, 6 pairs + a single tail, FASTA, -unique, -m) on records of a real mapping, against sam.format_records"""
    c, ix, gpu = ctxs["pe101_spliced"]
    seqs, headers, quals = sdi.edge_reads(c["genome"])
    so, rl, flat = host.pack_reads(seqs)
    for unique, multi, fasta in ((False, False, False), (True, False, False), (False, True, False), (True, True, True)):
        gpu.set_params(host.default_params(paired=1, max_mismatch=5, multi_hit=int(multi)))
        res = gpu.map_batch(so[:12], rl[:12], flat)          # the pairs are mapped as pairs, the tail as a single read
        gpu.set_params(host.default_params(paired=0, max_mismatch=5, multi_hit=int(multi)))
        tail = gpu.map_batch(so[12:], rl[12:], flat)
        q = None if fasta else quals
        t_tail, ct_tail = gpu.format_sam(headers[12:], None if fasta else quals[12:], 0, unique_only=unique)
        gpu.set_params(host.default_params(paired=1, max_mismatch=5, multi_hit=int(multi)))
        gpu.map_batch(so[:12], rl[:12], flat)
        t_pairs, ct_pairs = gpu.format_sam(headers[:12], None if fasta else quals[:12], 12, unique_only=unique)
        w_pairs, st = sdi.twin_text(headers[:12], seqs[:12], None if fasta else quals[:12], res.reads, res.reports, res.cigar, ix.names, 12, multi=multi, unique=unique)
        w_tail, st2 = sdi.twin_text(headers[12:], seqs[12:], None if fasta else quals[12:], tail.reads, tail.reports, tail.cigar, ix.names, 0, multi=multi, unique=unique)
        _same(t_pairs, w_pairs); _same(t_tail, w_tail)
        assert ct_pairs == dict(unmapped=st.unmapped, unique=st.unique, paired=st.paired)
        # one batch whose last read is left single: n_pair_mode = n - 1 ... through the kernels on the single-end records of all 13 reads
        gpu.set_params(host.default_params(paired=0, max_mismatch=5, multi_hit=int(multi)))
        res13 = gpu.map_batch(so, rl, flat)
        t13, ct13 = gpu.format_sam(headers, q, 12, unique_only=unique)
        w13, st13 = sdi.twin_text(headers, seqs, q, res13.reads, res13.reports, res13.cigar, ix.names, 12, multi=multi, unique=unique)
        _same(t13, w13)
        assert ct13 == dict(unmapped=st13.unmapped, unique=st13.unique, paired=st13.paired)
        assert (b"N" * 5000 + b"\t") in t13


def test_device_sam_full_size_batch_has_the_host_formatter_digest(workdir):
    """BASELINE configs[1] at full size (chr20-sized genome, 1 M pairs 2x101, -mis 5, generated as tests/test_gpu_parity.py generates it): the SHA-256 of the
    device's text against the SHA-256 of the SAM body the HOST formatter of the `dart` command line writes for the same reads (the Python twin needs minutes
    for 2 M reads, so the command line's formatter -- pinned on the reference by tests/test_gpu_cli.py -- is the one used here)."""
    import bench
    cache = os.path.join(workdir, "bench_cache")
    prefix, g = bench.prepare_index(cache, bench.CHR20_LEN, 0, lambda: None)
    m1, m2 = synth.make_reads(g, 1000000, rlen=101, seed=1000, sub_rate=0.01, indel_frac=0.02, n_frac=0.002)
    d = os.path.join(workdir, "sam_full"); os.makedirs(d, exist_ok=True)
    synth.write_fastq_fast(os.path.join(d, "1.fq"), m1, 1); synth.write_fastq_fast(os.path.join(d, "2.fq"), m2, 2)
    r = subprocess.run([os.path.join(common.ROOT, "dart_amd", "dart"), "-i", prefix, "-f", "1.fq", "-f2", "2.fq", "-o", "host.sam", "-j", "host.j", "-t", "16", "-mis", "5"],
                       cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(os.environ, DART_TIMING="1"))
    assert r.returncode == 0 and b"format=host" in r.stderr, r.stderr[-400:]
    ix = host.Index(prefix)
    want = hashlib.sha256(); n_want = 0
    with open(os.path.join(d, "host.sam"), "rb") as f:
        for line in f:
            if not line.startswith(b"@") or n_want:
                want.update(line); n_want += len(line)
    arr = host.interleave_pairs(m1, m2)
    so, rl, flat = host.pack_reads(arr)
    gpu = host.DartGPU(ix, host.default_params(paired=1, max_mismatch=5))
    gpu.map_batch(so, rl, flat)
    ids = np.char.add("r", np.char.zfill(np.repeat(np.arange(1000000), 2).astype(str), 9))
    text, ct = gpu.format_sam([s.encode() for s in ids.tolist()], [b"I" * 101] * 2000000, 2000000)
    print("full size: %d bytes of SAM, device %.3f ms" % (len(text), gpu.sam_device_ms))
    gpu.close()
    assert len(text) == n_want and hashlib.sha256(text).hexdigest() == want.hexdigest()
