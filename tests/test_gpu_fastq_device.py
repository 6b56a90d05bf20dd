"""GPU suite (-m gpu): FASTQ text parsed on the device (dg_batch_upload_fastq, dart_amd/csrc/dg_fastq.h) against the host packer on the golden cases, against a
Python restatement of the reference's reader (tests/fastq_device_inputs.py) on an awkward text, on line ends at the seams of the kernels' tiles, split into two
uploads, and on its error contract; the SAM text formatted from the resident names and qualities (dg_batch_format_sam_resident) against the golden SAM."""
import ctypes as C
import os
import numpy as np
import pytest
import common
import fastq_device_inputs as fdi
import sam_device_inputs as sdi
from dart_amd import host, synth

pytestmark = pytest.mark.gpu
CASES = sorted(common.MANIFEST["cases"])
ARG, CAPACITY = -3, -4


@pytest.fixture(scope="module")
def ctxs(workdir):
    out = {}
    for name in CASES:
        c = common.build_case(name, workdir)
        ix = host.Index(c["prefix"])
        d = os.path.join(workdir, "fqdev_" + name); os.makedirs(d, exist_ok=True)
        synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
        t1 = open(os.path.join(d, "1.fq"), "rb").read(); t2 = None
        if c["spec"]["paired"]:
            synth.write_fastq(os.path.join(d, "2.fq"), c["m2"], 2)
            t2 = open(os.path.join(d, "2.fq"), "rb").read()
        out[name] = (c, ix, host.DartGPU(ix), t1, t2)
    yield out
    for v in out.values():
        v[2].close()


def _same_text(got: bytes, want: bytes):
    assert got == want, common.first_diff(got.decode("latin1"), want.decode("latin1"))


def _batch(gpu):
    """the parsed batch as [(name, stored read, stored quality)]"""
    so, rl, flat, names, quals = gpu.download_reads()
    raw = flat.tobytes()
    return [(names[k], raw[int(so[k]):int(so[k]) + int(rl[k])], quals[k]) for k in range(len(rl))]


def _same_reads(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)


@pytest.mark.parametrize("name", CASES)
def test_fastq_upload_equals_the_host_packer_and_maps_and_prints_the_golden_sam(name, ctxs):
    c, ix, gpu, t1, t2 = ctxs[name]
    paired = bool(c["spec"]["paired"])
    n = len(c["reads"]); npm = n if paired else 0
    so, rl, flat = host.pack_reads(c["reads"])
    for run in c["runs"]:
        p, h = common.parse_flags(run["flags"])
        gpu.set_params(host.default_params(paired=int(paired), **p))
        want = gpu.map_batch(so, rl, flat)
        assert gpu.upload_fastq(t1, t2, rc_odd_reads=paired) == n
        assert gpu.fastq_device_ms > 0
        gso, grl, gflat, names, quals = gpu.download_reads()
        assert np.array_equal(gso, so) and np.array_equal(grl, rl) and np.array_equal(gflat, flat.reshape(-1))
        assert names == [x.encode() for x in c["headers"]] and quals == [q.encode() for q in c["quals"]]
        gpu.run()
        common.assert_same(gpu.download(), (want.reads, want.reports, want.cigar, want.sj))
        text, ct = gpu.format_sam_resident(npm, unique_only=h["unique"])
        _same_text(text, sdi.body_of(common.golden_sam(run["base"])))
        # the host-array formatter on the same FASTQ-uploaded batch: the same bytes, and the resident arrays are still there afterwards
        text2, ct2 = gpu.format_sam(c["headers"], c["quals"], npm, unique_only=h["unique"])
        assert text2 == text and ct2 == ct
        text3, ct3 = gpu.format_sam_resident(npm, unique_only=h["unique"])
        assert text3 == text and ct3 == ct


@pytest.fixture(scope="module")
def awkward():
    return fdi.awkward_texts(fdi.random_reads(23, seed=5), fdi.random_reads(23, seed=6))


@pytest.mark.parametrize("layout", ["two_files_paired", "interleaved_paired", "one_file_single", "two_files_single"])
def test_fastq_upload_of_the_awkward_text_equals_the_reference_reader(layout, awkward, ctxs):
    gpu = ctxs["pe101_spliced"][2]
    t1, t2, inter = awkward
    a, b = (inter, None) if layout == "interleaved_paired" else (t1, None) if layout == "one_file_single" else (t1, t2)
    paired = layout.endswith("paired")
    want = fdi.reference_reads(a, b, paired)
    assert gpu.upload_fastq(a, b, rc_odd_reads=paired) == len(want)
    _same_reads(_batch(gpu), want)
    lens = [len(s) for h, s, q in want]
    assert 1 in lens and 1000 in lens and any(len(h) == 5000 for h, s, q in want) and any(h == b"" for h, s, q in want) and any(b"\0" in q for h, s, q in want)


def test_fastq_upload_with_line_ends_on_tile_seams(ctxs):
    gpu = ctxs["pe101_spliced"][2]
    tile = gpu.fastq_tile()
    assert tile > 0 and tile % 16 == 0
    for label, text in fdi.seam_texts(tile):
        want = fdi.reference_reads(text, None, False)
        assert len(want) > 3 * tile // 200 and gpu.upload_fastq(text) == len(want), label
        _same_reads(_batch(gpu), want)
        # the same text as file 2 of a pair of files: its own tiles, its odd reads reverse-complemented
        want2 = fdi.reference_reads(text, text, True)
        assert gpu.upload_fastq(text, text, rc_odd_reads=True) == len(want2) == 2 * len(want), label
        _same_reads(_batch(gpu), want2)


def test_fastq_upload_of_more_reads_than_one_scan_of_the_workgroup_sums_holds(ctxs):
    """65 537 single reads: 257 workgroups of k_fq_len, so k_fq_top3's scan of their sums takes a second trip with a carry, for all three lengths"""
    gpu = ctxs["pe101_spliced"][2]
    n = 65537
    seqs = [bytes(r) for r in fdi.random_reads(n, rlen=20, seed=9)]
    names = [b"r%d" % (k * 7919 % n) + b"x" * (k % 5) for k in range(n)]
    quals = [bytes(33 + (k + j) % 41 for j in range(20 - k % 4)) for k in range(n)]
    text = b"".join(b"@%s\n%s\n+\n%s\n" % (names[k], seqs[k], quals[k]) for k in range(n))
    so, rl, flat = host.pack_reads(seqs)
    assert gpu.upload_fastq(text) == n
    gso, grl, gflat, gnames, gquals = gpu.download_reads()
    assert np.array_equal(gso, so) and np.array_equal(grl, rl) and np.array_equal(gflat, flat)
    want = fdi.reference_reads(text, None, False)           # (a quality shorter than its read is stored with its line end, as the reference's reader keeps it)
    assert [h for h, s, q in want] == names and [s for h, s, q in want] == seqs
    assert gnames == names and gquals == [q for h, s, q in want]
    assert len({len(x) for x in names}) > 4 and {len(q) for q in quals} == {17, 18, 19, 20}


def test_fastq_upload_does_not_depend_on_how_the_text_is_split(ctxs):
    c, ix, gpu, t1, t2 = ctxs["pe101_spliced"]
    n = len(c["reads"])
    p, _ = common.parse_flags(c["runs"][0]["flags"])
    def part(g, a, b):
        g.set_params(host.default_params(paired=1, **p))
        k = g.upload_fastq(a, b, rc_odd_reads=True)
        reads = _batch(g)
        g.run()
        return reads, g.format_sam_resident(k)
    whole_reads, (whole, ctw) = part(gpu, t1, t2)
    assert len(whole_reads) == n
    def cut_at(t, rec):                       # the byte offset of record `rec`: behind its 4 * rec-th newline
        pos = 0
        for _ in range(4 * rec):
            pos = t.index(b"\n", pos) + 1
        return pos
    rec = n // 4 + 1
    c1, c2 = cut_at(t1, rec), cut_at(t2, rec)
    ra, (a, cta) = part(gpu, t1[:c1], t2[:c2]); rb, (b, ctb) = part(gpu, t1[c1:], t2[c2:])
    assert ra + rb == whole_reads and a + b == whole and {k: cta[k] + ctb[k] for k in cta} == ctw
    clone = gpu.clone()
    rc_, (on_clone, ctc) = part(clone, t1, t2)
    assert rc_ == whole_reads and on_clone == whole and ctc == ctw


def test_fastq_upload_error_contract(ctxs):
    c, ix, gpu, t1, t2 = ctxs["pe101_spliced"]
    lib = gpu.lib
    p, _ = common.parse_flags(c["runs"][0]["flags"])
    gpu.set_params(host.default_params(paired=1, **p))
    n_small = 400
    def cut_at(t, rec):
        pos = 0
        for _ in range(4 * rec):
            pos = t.index(b"\n", pos) + 1
        return pos
    s1, s2 = t1[:cut_at(t1, n_small // 2)], t2[:cut_at(t2, n_small // 2)]
    so, rl, flat = host.pack_reads(c["reads"][:n_small])
    want = gpu.map_batch(so, rl, flat)
    def normal_batch_still_maps():
        assert gpu.upload_fastq(s1, s2, rc_odd_reads=True) == n_small
        gpu.run()
        common.assert_same(gpu.download(), (want.reads, want.reports, want.cigar, want.sj))
    def call(a, b, max_reads=None):
        ka = np.frombuffer(a + b"\0", np.uint8); kb = np.frombuffer(b + b"\0", np.uint8) if b is not None else None
        t = host.FastqText(); t.text1, t.n1 = ka.ctypes.data, len(a)
        if kb is not None:
            t.text2, t.n2 = kb.ctypes.data, len(b)
        t.rc_odd_reads = 1; t.max_reads = 1 << 20 if max_reads is None else max_reads
        n = C.c_int(-7)
        rc = lib.dg_batch_upload_fastq(gpu.ctx, C.byref(t), C.byref(n))
        return rc, int(n.value), (lib.dg_last_error(gpu.ctx) or b"").decode()
    # a record without bases in the middle of one text: read 7
    r = lambda i, s=b"ACGTACGTACGTACGTACGTACGT": b"@e%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n"
    text = b"".join(r(i) for i in range(7)) + b"@empty\n\n+\n\n" + b"".join(r(i) for i in range(8, 12))
    rc, n, msg = call(text, None)
    assert rc == ARG and "read 7 " in msg and "without bases" in msg, msg
    used = (C.c_size_t * 3)()
    assert lib.dg_batch_run(gpu.ctx, used) == 0 and list(used) == [0, 0, 0]        # the context holds no batch
    normal_batch_still_maps()
    # the same in file 2 of two files: record 3 of text2 is read 7
    rc, n, msg = call(b"".join(r(i) for i in range(6)), b"".join(r(i) for i in range(3)) + b"@gone\n\n+\n\n" + b"".join(r(i) for i in range(4, 6)))
    assert rc == ARG and "read 7 " in msg, msg
    normal_batch_still_maps()
    # a 1001-base read (and a 1000-base one is fine)
    rc, n, msg = call(r(0) + r(1, b"A" * 1001) + r(2), None)
    assert rc == ARG and "DG_MAX_RLEN" in msg and "read 1 " in msg, msg
    normal_batch_still_maps()
    rc, n, msg = call(r(0) + r(1, b"A" * 1000) + r(2), None)
    assert rc == 0 and n == 3
    # max_reads one too small: the need comes back
    rc, n, msg = call(s1, s2, max_reads=n_small - 1)
    assert rc == CAPACITY and n == n_small and str(n_small) in msg, msg
    normal_batch_still_maps()
    rc, n, msg = call(s1, s2, max_reads=n_small)
    assert rc == 0 and n == n_small
    # text2 with two records fewer; with one fewer the stream has an odd last read
    rc, n, msg = call(s1, s2[:cut_at(s2, n_small // 2 - 2)])
    assert rc == ARG and "records" in msg, msg
    normal_batch_still_maps()
    rc, n, msg = call(s1, s2[:cut_at(s2, n_small // 2 - 1)])
    assert rc == 0 and n == n_small - 1
    # no text: no reads
    rc, n, msg = call(b"", None)
    assert rc == 0 and n == 0
    assert lib.dg_batch_run(gpu.ctx, used) == 0
    nb = C.c_size_t(5); ct = (C.c_uint64 * 3)()
    assert lib.dg_batch_format_sam_resident(gpu.ctx, 0, 0, C.byref(nb), ct, None) == 0 and nb.value == 0
    # the resident formatter after a plain upload: refused; download_reads too
    gpu.map_batch(so, rl, flat)
    assert lib.dg_batch_format_sam_resident(gpu.ctx, n_small, 0, C.byref(nb), ct, None) == ARG and "dg_batch_upload_fastq" in (lib.dg_last_error(gpu.ctx) or b"").decode()
    caps = (C.c_size_t * 3)(0, 0, 0)
    assert lib.dg_batch_download_reads(gpu.ctx, None, None, None, None, None, None, None, caps, used) == ARG
    # download_reads with too little room says what it needs
    normal_batch_still_maps()
    assert lib.dg_batch_download_reads(gpu.ctx, None, None, None, None, None, None, None, caps, used) == CAPACITY
    assert list(used) == [int(rl.astype(np.int64).sum()), sum(len(h) for h in c["headers"][:n_small]), int(rl.astype(np.int64).sum())]
