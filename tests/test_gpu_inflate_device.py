"""GPU suite (-m gpu): BGZF inflated on the device (dg_bgzf_inflate, dart_amd/csrc/dg_inflate.h) against zlib -- the same bytes where zlib inflates, DG_ERR_ARG
naming the block and the rule where zlib refuses -- and in front of the device's FASTQ parser (dg_batch_upload_fastq_bgzf): texts cut into blocks of every
awkward size, chained calls whose tails become the next heads, the last call's end-of-text rules, DG_FQ_CHECK_ONLY, the count of records the reference's gz
reader would read differently, and one mapped batch.  The streams and the Python restatements are tests/gz_device_inputs.py's."""
import ctypes as C
import zlib
import numpy as np
import pytest
import common
import fastq_device_inputs as fdi
import gz_device_inputs as gz
from dart_amd import host

pytestmark = pytest.mark.gpu
ARG, CAPACITY = -3, -4
RULES = {gz.E_BTYPE: "invalid block type", gz.E_STORED: "invalid stored block lengths", gz.E_SYMBOLS: "too many length or distance symbols",
         gz.E_CODELEN_SET: "invalid code lengths set", gz.E_REPEAT: "invalid bit length repeat", gz.E_NO_EOB: "missing end-of-block",
         gz.E_LITLEN_SET: "invalid literal/lengths set", gz.E_DIST_SET: "invalid distances set", gz.E_LITLEN_CODE: "invalid literal/length code",
         gz.E_DIST_CODE: "invalid distance code", gz.E_FAR: "invalid distance too far back", gz.E_INPUT: "the input ends before the final block",
         gz.E_ISIZE: "length is not ISIZE", gz.E_CRC: "CRC32 mismatch"}


@pytest.fixture(scope="module")
def case(workdir):
    c = common.build_case("pe101_spliced", workdir)
    gpu = host.DartGPU(host.Index(c["prefix"]))
    yield c, gpu
    gpu.close()


@pytest.fixture(scope="module")
def gpu(case):
    return case[1]


def _inflate_rc(gpu, data: bytes):
    a = np.frombuffer(data + b"\0", np.uint8)
    nb = C.c_size_t(7); nk = C.c_size_t(7); ms = C.c_float(0)
    rc = gpu.lib.dg_bgzf_inflate(gpu.ctx, a.ctypes.data, len(data), C.byref(nb), C.byref(nk), C.byref(ms))
    return rc, int(nb.value), (gpu.lib.dg_last_error(gpu.ctx) or b"").decode()


def _batch(gpu):
    so, rl, flat, names, quals = gpu.download_reads()
    raw = flat.tobytes()
    return [(names[k], raw[int(so[k]):int(so[k]) + int(rl[k])], quals[k]) for k in range(len(rl))]


def _same_reads(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)


# ---- the inflater against zlib -----------------------------------------------------------------------------------------------------------------------
def test_round_trip_through_the_devices_own_writers(gpu):
    noise = np.random.default_rng(2).integers(0, 256, 100 * 1024, dtype=np.uint8).tobytes()
    for x in [gz.fastq_like(n, seed=n % 7) for n in (0, 1, gz.BLOCK, gz.BLOCK + 1, 3 * gz.BLOCK + 17)] + [b"G" * (200 * 1024), noise]:
        for dynamic in (False, True):
            blocks = gpu.bgzf_compress(x, dynamic=dynamic)
            assert gz.bgzf_reference(blocks) == x
            assert gpu.bgzf_inflate(blocks) == x, (len(x), dynamic)
            assert gpu.inflate_blocks == (len(x) + gz.BLOCK - 1) // gz.BLOCK and (gpu.inflate_device_ms > 0 or not x)


def test_zlib_made_blocks(gpu):
    per_wg = gpu.inflate_granules()[0]
    assert per_wg >= 1
    t = gz.fastq_like(3 * gz.BLOCK + 17)
    cases = [(gz.bgzf(t, level=lvl), t) for lvl in (0, 1, 6, 9)]
    cases += [(gz.bgzf(t, strategy=st), t) for st in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)]
    big = gz.fastq_like(65536, 5)
    cases.append((gz.member(gz.deflate_raw(big), big), big))
    part = t[:60000]
    cases.append((gz.member(gz.deflate_raw(part, 6, full_flush_at=(100, 100, 5000, 30000)), part), part))
    cases += [(gz.EOF_MEMBER, b""), (gz.EOF_MEMBER + gz.bgzf(t[:1000], block=300) + gz.EOF_MEMBER + gz.bgzf(t[1000:2000], eof=True), t[:2000])]
    cases.append((gz.bgzf(t[:5000], block=700, extra_front=b"XY\x03\x00abc"), t[:5000]))
    for k in (per_wg - 1, per_wg, per_wg + 1, 2 * per_wg + 1):
        cases.append((gz.bgzf(t[:300 * k], block=300), t[:300 * k]))
    for blocks, want in cases:
        assert gz.bgzf_reference(blocks) == want
        assert gpu.bgzf_inflate(blocks) == want, len(want)


def test_hand_made_valid_streams(gpu):
    v = gz.valid_streams(round_tokens=gpu.inflate_granules()[1])
    for name, (raw, data) in v.items():
        assert gpu.bgzf_inflate(gz.as_member(raw, data)) == data, name
    assert gpu.bgzf_inflate(b"".join(gz.as_member(*x) for x in v.values())) == b"".join(x[1] for x in v.values())


def test_invalid_streams_and_files_are_refused_and_the_context_stays_usable(gpu):
    """every rule of the inflater and of the member walker once: DG_ERR_ARG naming the block and the rule; a good inflate follows on the same context"""
    good_text = gz.fastq_like(900, 4)
    good = gz.bgzf(good_text, block=500)
    for name, (raw, rule) in gz.invalid_streams().items():
        rc, nb, msg = _inflate_rc(gpu, good + gz.as_member(raw, None) + good)
        assert rc == ARG and nb == 0 and "block 2:" in msg and RULES[rule] in msg, (name, rc, msg)
        assert gpu.bgzf_inflate(good) == good_text, name
    for name, (data, rule, idx, _) in gz.invalid_files().items():
        rc, nb, msg = _inflate_rc(gpu, data)
        assert rc == ARG and nb == 0 and "block %d:" % idx in msg and (rule == gz.WALKER or RULES[rule] in msg), (name, rc, msg)
        assert gpu.bgzf_inflate(good) == good_text, name
    # two failing blocks: the first is named
    iv = gz.invalid_streams()
    rc, nb, msg = _inflate_rc(gpu, good + gz.as_member(iv["block_type_3"][0], None) + gz.as_member(iv["distance_one_too_far"][0], None))
    assert rc == ARG and "block 2:" in msg and "invalid block type" in msg, msg
    # download with too little room; the device pointer
    assert gpu.bgzf_inflate(good) == good_text
    out = np.zeros(len(good_text), np.uint8)
    assert gpu.lib.dg_inflate_download(gpu.ctx, out.ctypes.data, len(good_text) - 1) == CAPACITY and not out.any()
    ptr = C.c_void_p(); n = C.c_size_t(0)
    assert gpu.lib.dg_inflate_device(gpu.ctx, C.byref(ptr), C.byref(n)) == 0 and n.value == len(good_text) and ptr.value
    rc, nb, msg = _inflate_rc(gpu, b"")
    assert rc == 0 and nb == 0


# ---- FASTQ through blocks ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def awkward():
    return fdi.awkward_texts(fdi.random_reads(23, seed=5), fdi.random_reads(23, seed=6))


@pytest.mark.parametrize("block", [1, 7, 100, gz.BLOCK])
def test_fastq_through_blocks_of_every_size_equals_the_reference_reader(block, awkward, gpu):
    t1, t2, inter = awkward
    for a, b, paired in ((t1, t2, True), (inter, None, True), (t1, None, False)):
        want = fdi.reference_reads(a, b, paired)
        n, tail1, tail2, unlike = gpu.upload_fastq_bgzf(b"", gz.bgzf(a, block=block), None if b is None else b"", None if b is None else gz.bgzf(b, block=block),
                                                        rc_odd_reads=paired, last=True)
        assert n == len(want) and tail1 == b"" and tail2 in (None, b"")
        _same_reads(_batch(gpu), want)
        assert gpu.fastq_device_ms > 0


def test_fastq_through_blocks_with_line_ends_on_tile_seams(gpu):
    tile = gpu.fastq_tile()
    for label, text in fdi.seam_texts(tile):
        want = fdi.reference_reads(text, None, False)
        for block in (gz.BLOCK, 1000):
            n, tail1, _, unlike = gpu.upload_fastq_bgzf(b"", gz.bgzf(text, block=block), last=True)
            assert n == len(want) and unlike == 0, (label, block)
            _same_reads(_batch(gpu), want)
        # the same without `last`: whole records only; a text that ends without its newline leaves its last record as the tail
        k, pos = gz.whole_records(text)
        n, tail1, _, unlike = gpu.upload_fastq_bgzf(text[:77], gz.bgzf(text[77:], block=3000))
        assert n == k and tail1 == text[pos:], label
        _same_reads(_batch(gpu), want[:k])


def _chain(gpu, t1, t2, blocks1, blocks2, per_call, paired, check_only=False):
    """the members of each text `per_call` at a time, tails chained -> (batches concatenated, [(n, tail1, tail2, unlike)] per call); every call's tails are
    compared with the Python restatement"""
    two = t2 is not None
    m1 = _members(blocks1); m2 = _members(blocks2) if two else []
    calls = max((len(m1) + per_call - 1) // per_call, (len(m2) + per_call - 1) // per_call, 1)
    head1, head2, reads, log = b"", b"", [], []
    for i in range(calls):
        last = i == calls - 1
        c1 = b"".join(m1[i * per_call:(i + 1) * per_call]); c2 = b"".join(m2[i * per_call:(i + 1) * per_call])
        x1 = head1 + gz.bgzf_reference(c1); x2 = head2 + gz.bgzf_reference(c2)
        n, tail1, tail2, unlike = gpu.upload_fastq_bgzf(head1, c1, head2 if two else None, c2 if two else None, rc_odd_reads=paired, last=last, check_only=check_only)
        if last:
            want_tails = (b"", b"" if two else None)
        else:
            k = min(gz.whole_records(x1)[0], gz.whole_records(x2)[0]) if two else gz.whole_records(x1)[0]
            assert n == (2 * k if two else k), (i, n, k)
            want_tails = (x1[gz.cut_records(x1, k):], x2[gz.cut_records(x2, k):] if two else None)
        assert (tail1, tail2) == want_tails, (i, len(tail1), len(want_tails[0]))
        if not check_only:
            reads += _batch(gpu)
        log.append((n, tail1, tail2, unlike))
        head1, head2 = tail1, tail2 if two else b""
    return reads, log


def _members(blocks: bytes):
    out = []
    while blocks:
        bsize = int.from_bytes(blocks[16:18], "little") + 1            # (gz.bgzf writes BC as the only subfield)
        out.append(blocks[:bsize]); blocks = blocks[bsize:]
    return out


@pytest.mark.parametrize("per_call", [1, 2, 5])
def test_chained_calls_with_tails_equal_the_plain_upload(per_call, awkward, gpu):
    t1, t2, inter = awkward
    # one text (unpaired: a call may take an odd number of records, and which reads are odd is counted from the call's first); two texts whose blocks --
    # and so whose record boundaries -- are skewed against each other
    for a, b, paired, blk in ((inter, None, False, (1500, 0)), (t1, t2, True, (900, 2100)), (t1, t2, False, (2500, 700))):
        assert gpu.upload_fastq(a, b, rc_odd_reads=paired) == len(fdi.reference_reads(a, b, paired))
        want = _batch(gpu)
        reads, log = _chain(gpu, a, b, gz.bgzf(a, block=blk[0]), gz.bgzf(b, block=blk[1]) if b is not None else None, per_call, paired)
        _same_reads(reads, want)
        assert len(log) > 2 and any(l[1] for l in log[:-1])               # several calls, and tails that are not empty
        if b is not None:
            assert any(l[1] and l[2] and len(l[1]) != len(l[2]) for l in log[:-1])


def test_last_call_takes_a_line_without_newline_and_one_more_record_in_text_1(awkward, gpu):
    t1, t2, inter = awkward
    assert not t1.endswith(b"\n")
    t2_short = t2[:gz.cut_records(t2, gz.whole_records(t2)[0] - 1)]
    want = fdi.reference_reads(t1, t2_short, True)
    assert len(want) % 2 == 1
    n, tail1, tail2, unlike = gpu.upload_fastq_bgzf(t1[:1000], gz.bgzf(t1[1000:], block=1300), t2_short[:10], gz.bgzf(t2_short[10:], block=800), rc_odd_reads=True, last=True)
    assert n == len(want) and tail1 == b"" and tail2 == b""
    _same_reads(_batch(gpu), want)
    # without `last` the same texts give whole records, equally many of each text, and the rest as tails
    n, tail1, tail2, unlike = gpu.upload_fastq_bgzf(t1[:1000], gz.bgzf(t1[1000:], block=1300), t2_short[:10], gz.bgzf(t2_short[10:], block=800), rc_odd_reads=True)
    k = min(gz.whole_records(t1)[0], gz.whole_records(t2_short)[0])
    assert n == 2 * k and tail1 == t1[gz.cut_records(t1, k):] and tail2 == t2_short[gz.cut_records(t2_short, k):] and tail1 and not tail2
    _same_reads(_batch(gpu), want[:2 * k])
    # a text 2 that is two records short at the files' end is refused as by the plain call
    t2_shorter = t2[:gz.cut_records(t2, gz.whole_records(t2)[0] - 2)]
    with pytest.raises(RuntimeError, match="records"):
        gpu.upload_fastq_bgzf(b"", gz.bgzf(t1), b"", gz.bgzf(t2_shorter), rc_odd_reads=True, last=True)


def test_check_only_gives_the_same_counts_and_leaves_no_batch(awkward, case):
    c, gpu = case
    t1, t2, inter = awkward
    b1, b2 = gz.bgzf(t1, block=900), gz.bgzf(t2, block=2100)
    reads, log = _chain(gpu, t1, t2, b1, b2, 3, True)
    _, log_check = _chain(gpu, t1, t2, b1, b2, 3, True, check_only=True)
    assert log_check == log
    used = (C.c_size_t * 3)()
    assert gpu.lib.dg_batch_run(gpu.ctx, used) == ARG and "no batch" in (gpu.lib.dg_last_error(gpu.ctx) or b"").decode()
    caps = (C.c_size_t * 3)(0, 0, 0)
    assert gpu.lib.dg_batch_download_reads(gpu.ctx, None, None, None, None, None, None, None, caps, used) == ARG
    # the next upload gives the context a batch again
    assert gpu.upload_fastq(t1, t2, rc_odd_reads=True) == len(reads)
    assert gpu.lib.dg_batch_run(gpu.ctx, used) == 0


def _upload_raw(gpu, head1, blocks1, head2=None, blocks2=None, max_reads=1 << 20, last=True, flags=0):
    bufs = [np.frombuffer((x or b"") + b"\0", np.uint8) for x in (head1, blocks1, head2, blocks2)]
    t = host.FastqBgzf()
    t.head1, t.n_head1, t.blocks1, t.n_blocks1 = bufs[0].ctypes.data, len(bufs[0]) - 1, bufs[1].ctypes.data, len(bufs[1]) - 1
    if head2 is not None or blocks2 is not None:
        t.head2, t.n_head2, t.blocks2, t.n_blocks2 = bufs[2].ctypes.data, len(bufs[2]) - 1, bufs[3].ctypes.data, len(bufs[3]) - 1
    t.rc_odd_reads, t.max_reads, t.last = 0, max_reads, int(last)
    n = C.c_int(-7); tail = (C.c_size_t * 2)(9, 9); nu = C.c_uint64(99)
    rc = gpu.lib.dg_batch_upload_fastq_bgzf(gpu.ctx, C.byref(t), flags, C.byref(n), tail, C.byref(nu))
    return rc, int(n.value), (int(tail[0]), int(tail[1])), int(nu.value), (gpu.lib.dg_last_error(gpu.ctx) or b"").decode()


def test_n_unlike_counts_what_the_references_gz_reader_would_read_differently(gpu):
    r = lambda i, h=None, s=b"ACGTACGTACGTACGTACGTACGT", q=None: (h if h is not None else b"@u%d/1" % i) + b"\n" + s + b"\n+\n" + (q if q is not None else b"I" * len(s)) + b"\n"
    kinds = {
        "header_of_1024_bytes": r(0, h=b"@" + b"n" * 1022),                       # 1023 bytes and the newline
        "plus_line_of_1024_bytes": b"@p\nACGT\n+" + b"x" * 1022 + b"\nIIII\n",
        "quality_of_1024_bytes": r(0, s=b"ACGT", q=b"I" * 1023),
        "nul_in_the_quality": r(0, q=b"IIII\0" + b"I" * 19),
        "nul_in_the_name": r(0, h=b"@a\0b"),
        "header_without_at": r(0, h=b">fasta_like"),
        "header_names_nothing": r(0, h=b"@@@"),
        "header_names_nothing_blank": r(0, h=b"@ comment"),
    }
    fine = {"header_of_1023_bytes": r(0, h=b"@" + b"n" * 1021), "read_of_1000_bases": r(0, s=b"A" * 1000), "crlf": b"@c\r\nACGT\r\n+\r\nIIII\r\n"}
    text = b"".join(r(i) for i in range(5)) + b"".join(kinds.values()) + b"".join(r(i) for i in range(5, 9)) + b"".join(fine.values())
    recs = gz.record_lines(text)
    want = sum(gz.unlike(x) for x in recs)
    assert want == len(kinds) and all(gz.unlike(gz.record_lines(k)[0]) for k in kinds.values()) and not any(gz.unlike(gz.record_lines(k)[0]) for k in fine.values())
    blocks = gz.bgzf(text, block=777)
    for flags in (0, host.FQ_CHECK_ONLY):
        rc, n, tails, nu, msg = _upload_raw(gpu, b"", blocks, flags=flags)
        assert rc == 0 and n == len(recs) and nu == want and tails == (0, 0), (rc, n, nu, msg)
    # in chained calls every record is counted once, in the call that takes it
    reads, log = _chain(gpu, text, None, blocks, None, 2, False)
    assert sum(l[3] for l in log) == want and len(reads) == len(recs)
    # a record without bases: counted, and refused as the plain call refuses it; a record with fewer than four lines at the files' end
    text = r(0) + b"@empty\n\n+\n\n" + r(2)
    rc, n, tails, nu, msg = _upload_raw(gpu, b"", gz.bgzf(text))
    assert rc == ARG and "read 1 " in msg and "without bases" in msg and nu == 1 == sum(gz.unlike(x) for x in gz.record_lines(text)), (rc, nu, msg)
    text = r(0) + r(1, s=b"A" * 1023) + r(2)               # (a read line of 1024 bytes is also longer than the library takes)
    rc, n, tails, nu, msg = _upload_raw(gpu, b"", gz.bgzf(text))
    assert rc == ARG and "DG_MAX_RLEN" in msg and nu == 1 == sum(gz.unlike(x) for x in gz.record_lines(text)), (rc, nu, msg)
    text = r(0) + b"@cut\nACGT\n+"
    rc, n, tails, nu, msg = _upload_raw(gpu, b"", gz.bgzf(text))
    assert rc == 0 and n == 2 and nu == 1 == sum(gz.unlike(x) for x in gz.record_lines(text)), (rc, n, nu, msg)


def test_fastq_bgzf_error_contract(awkward, gpu):
    t1, t2, inter = awkward
    b1, b2 = gz.bgzf(t1, block=1000), gz.bgzf(t2, block=1000)
    n_all = len(fdi.reference_reads(t1, t2, True))
    def still_works():
        n, tail1, tail2, _ = gpu.upload_fastq_bgzf(b"", b1, b"", b2, rc_odd_reads=True, last=True)
        assert n == n_all
    iv = gz.invalid_streams()
    bad = gz.as_member(iv["distance_one_too_far"][0], None)
    m2 = _members(b2)
    rc, n, tails, nu, msg = _upload_raw(gpu, b"", b1, b"", b"".join(m2[:3]) + bad + b"".join(m2[3:]))
    assert rc == ARG and n == 0 and tails == (0, 0) and "text 2 block 3:" in msg and "too far back" in msg, msg
    still_works()
    rc, n, tails, nu, msg = _upload_raw(gpu, b"", b1[:-1], b"", b2)
    assert rc == ARG and "text 1 block %d:" % (len(_members(b1)) - 1) in msg, msg
    still_works()
    flipped = bytearray(b1); flipped[len(_members(b1)[0]) - 8] ^= 1
    rc, n, tails, nu, msg = _upload_raw(gpu, b"", bytes(flipped), b"", b2)
    assert rc == ARG and "text 1 block 0:" in msg and "CRC32" in msg, msg
    still_works()
    rc, n, tails, nu, msg = _upload_raw(gpu, b"", b1, b"", b2, max_reads=n_all - 1)
    assert rc == CAPACITY and n == n_all and str(n_all) in msg, msg
    rc, n, tails, nu, msg = _upload_raw(gpu, b"", b1, b"", b2, max_reads=n_all)
    assert rc == 0 and n == n_all
    rc, n, tails, nu, msg = _upload_raw(gpu, b"", b1, flags=2)
    assert rc == ARG and "flag" in msg
    rc, n, tails, nu, msg = _upload_raw(gpu, b"", b"", last=False)
    assert rc == 0 and n == 0 and tails == (0, 0)
    # only heads: plain text goes through the same call
    n, tail1, tail2, _ = gpu.upload_fastq_bgzf(t1, b"", t2, b"", rc_odd_reads=True, last=True)
    assert n == n_all
    # a tail buffer that is too small
    n, tail1, tail2, _ = gpu.upload_fastq_bgzf(b"", b"".join(_members(b1)[:2]))
    assert tail1
    out = np.zeros(len(tail1), np.uint8)
    assert gpu.lib.dg_batch_download_fastq_tail(gpu.ctx, out.ctypes.data, len(tail1) - 1, None, 0) == CAPACITY and not out.any()


def test_a_batch_uploaded_through_bgzf_maps_and_prints_as_the_plain_upload(case, workdir):
    import os
    from dart_amd import synth
    c, gpu = case
    d = os.path.join(workdir, "gzdev"); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"][:300], 1); synth.write_fastq(os.path.join(d, "2.fq"), c["m2"][:300], 2)
    t1 = open(os.path.join(d, "1.fq"), "rb").read(); t2 = open(os.path.join(d, "2.fq"), "rb").read()
    p, h = common.parse_flags(c["runs"][0]["flags"])
    gpu.set_params(host.default_params(paired=1, **p))
    assert gpu.upload_fastq(t1, t2, rc_odd_reads=True) == 600
    gpu.run()
    want = gpu.download(); want_sam = gpu.format_sam_resident(600, unique_only=h["unique"]); want_bam = gpu.format_bam_resident(600, unique_only=h["unique"], raw=True)
    n, tail1, tail2, unlike = gpu.upload_fastq_bgzf(b"", gpu.bgzf_compress(t1, dynamic=True), b"", gz.bgzf(t2, block=5000), rc_odd_reads=True, last=True)
    assert n == 600 and unlike == 0
    gpu.run()
    common.assert_same(gpu.download(), (want.reads, want.reports, want.cigar, want.sj))
    assert gpu.format_sam_resident(600, unique_only=h["unique"]) == want_sam
    assert gpu.format_bam_resident(600, unique_only=h["unique"], raw=True) == want_bam
