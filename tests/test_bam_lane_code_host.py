"""CPU suite: the per-read code of the device's BAM writer (dart_amd/csrc/dg_bamfmt.h) and the serial pieces of its deflate kernel (dg_bgzf.h) compiled
for the host (tests/native/bam_lane_checks.hip).  A record is defined by the host writer: the expected bytes are BamWriter::sam_line_to_bam
(tests/native/bam_raw_checks.cpp) over the text sam.format_records gives for the same records; the chain is pinned on the reference's own output by
decoding the bytes (tests/bam_decode.py) against the golden SAM."""
import gzip, os, subprocess, zlib
import numpy as np
import pytest
import common, oracle_py, bam_decode
import sam_device_inputs as sdi
import bam_device_inputs as bdi
from dart_amd import host

CASES = sorted(common.MANIFEST["cases"])


def _check(workdir, tag, res, so, rl, flat, headers, quals, names, n_pair_mode, unique, multi, seqs):
    reads, rep, cig, _ = res
    exe = bdi.build_lane_program(workdir)
    path = os.path.join(workdir, "bam_batch_%s.bin" % tag)
    sdi.write_batch(path, reads, rep, cig, so, rl, flat, headers, quals, names, n_pair_mode, unique, multi)
    lens, ct, rec = bdi.run_lane_program(exe, path)
    assert int(lens.sum()) == len(rec)
    twin, st = sdi.twin_text(headers, seqs, quals, reads, rep, cig, names, n_pair_mode, multi=multi, unique=unique)
    want, n_rec, n_refused = bdi.host_writer_bytes(workdir, tag, names, twin)
    assert ct == [st.unmapped, st.unique, st.paired, n_rec, n_refused], (ct, n_rec, n_refused)
    if rec != want:
        k = next(i for i in range(min(len(rec), len(want))) if rec[i] != want[i]) if rec[:len(want)] != want[:len(rec)] else min(len(rec), len(want))
        raise AssertionError("%s: %d bytes against the host writer's %d, first difference at byte %d" % (tag, len(rec), len(want), k))
    # which rules of the record definition occurred (the callers assert them)
    lines = [l for l in twin.decode("latin1").split("\n") if l]
    stored = set(sdi.as_bytes(s).decode("latin1") for s in seqs)
    recs = bdi.records_of(rec)
    seen = dict(records=n_rec, refused=n_refused, bin=sum(1 for f, _ in recs if f[4] != 4680), odd=sum(1 for f, _ in recs if f[7] % 2),
                flag4=sum(1 for l in lines if l.split("\t")[5] == "" and not int(l.split("\t")[1]) & 4),
                revcomp=sum(1 for l in lines if l.split("\t")[2] != "*" and l.split("\t")[9] not in stored))
    return rec, seen


def _decodes_to(rec, names, lens, golden_text):
    _, refs, lines, bins = bam_decode.decode(bdi.bam_file(names, lens, bdi.stored_bgzf(rec)))
    want = bdi.golden_as_bam_stores_it(golden_text)
    assert refs == list(zip(names, [int(x) for x in lens]))
    assert len(lines) == len(want)
    for a, b in zip(lines, want):
        assert a == b, (a, b)


@pytest.mark.parametrize("name", CASES)
def test_lane_code_writes_the_host_writers_records_of_every_golden_run(name, workdir):
    c = common.build_case(name, workdir)
    orc, ix = oracle_py.Oracle(c["prefix"]), host.Index(c["prefix"])
    so, rl, flat = host.pack_reads(c["reads"])
    paired = bool(c["spec"]["paired"])
    for run in c["runs"]:
        p, h = common.parse_flags(run["flags"])
        res = orc.map_batch(orc.params(paired=int(paired), **p), so, rl, flat, threads=4)
        rec, seen = _check(workdir, run["base"], res, so, rl, flat, c["headers"], c["quals"], ix.names, len(c["reads"]) if paired else 0, h["unique"], bool(p["multi_hit"]), c["seqs"])
        _decodes_to(rec, ix.names, ix.chr_len, common.golden_sam(run["base"]))
        assert seen["records"] > 0 and seen["refused"] == 0 and seen["bin"] > 0 and seen["revcomp"] > 0, seen
        assert seen["odd"] > 0 or c["reads"].shape[1] % 2 == 0, seen


def test_lane_code_writes_the_records_of_the_odd_character_reads(workdir):
    c = common.build_case("pe101_spliced", workdir)
    orc, ix = oracle_py.Oracle(c["prefix"]), host.Index(c["prefix"])
    seqs = common.odd_character_reads(c["genome"])
    so, rl, flat = host.pack_reads(seqs)
    res = orc.map_batch(orc.params(paired=0, max_mismatch=12), so, rl, flat, threads=4)
    headers = ["r%d" % i for i in range(len(seqs))]
    quals = ["I" * len(s) for s in seqs]
    rec, _ = _check(workdir, "odd", res, so, rl, flat, headers, quals, ix.names, 0, False, False, seqs)
    _decodes_to(rec, ix.names, ix.chr_len, gzip.open(os.path.join(common.GOLDEN, "odd_characters.mis12.sam.gz"), "rt").read())
    assert any(15 in (b >> 4, b & 15) for _, r in bdi.records_of(rec)[:200] for b in r[32 + r[8]:])      # a '-' or an N became code 15


def test_lane_code_writes_the_records_of_the_read_structures(workdir):
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
    rec, seen = _check(workdir, "read_structures", res, so, rl, flat, headers, quals, ix.names, len(seqs), False, True, seqs)
    _decodes_to(rec, ix.names, ix.chr_len, rsi.fixture_sam())
    assert seen["refused"] == 0 and seen["odd"] > 0


EDGE_RUNS = [(False, False, False), (True, False, False), (False, True, False), (True, True, True), (False, False, True)]


def _edge_batch(workdir, unique, multi, fasta):
    c = common.build_case("pe101_spliced", workdir)
    seqs, headers, quals = sdi.edge_reads(c["genome"])
    so, rl, flat = host.pack_reads(seqs)
    R, P, cig = bdi.edge_records()
    return (R, P, cig, None), so, rl, flat, headers, None if fasta else quals, ["chrA", "c" * 300], 12, unique, multi, seqs


@pytest.mark.parametrize("unique,multi,fasta", EDGE_RUNS)
def test_lane_code_on_an_input_the_fixtures_do_not_hold(unique, multi, fasta, workdir):
    """a negative POS, a POS beyond 32 bits, a CIGAR of 150 ops, a 5000-byte name (refused), a NUL inside a quality and a quality longer than its read (both
    refused), a 1-base and a 1000-base read, FASTA, -unique and -m -- against the host writer"""
    args = _edge_batch(workdir, unique, multi, fasta)
    rec, seen = _check(workdir, "edge_%d%d%d" % (unique, multi, fasta), *args)
    recs = bdi.records_of(rec)
    assert len(recs) == seen["records"] > 0 and seen["refused"] >= (2 if fasta else 4), seen
    assert any(f[1] == -4 for f, _ in recs)                                        # POS -3
    assert any(f[1] == (3999999000 - 1) - (1 << 32) for f, _ in recs)              # POS 3999999000: its low 32 bits
    assert any(f[1] == (4000000000 - 1) - (1 << 32) for f, _ in recs) == (multi and not unique)      # (a second report: -m shows it, MAPQ 1: -unique hides it)
    assert any(f[5] == 150 for f, _ in recs) == (not unique)                       # (MAPQ 0)
    assert not any(b"N" * 255 in r for _, r in recs)                               # the 5000-byte name wrote nothing
    quals_of = [r[32 + f[2] + 4 * f[5] + (f[7] + 1) // 2:][:f[7]] for f, r in recs]
    assert all(len(q) == f[7] for q, (f, _) in zip(quals_of, recs)) and any(f[7] == 1 for f, _ in recs) == (not unique) and any(f[7] == 1000 for f, _ in recs)
    assert all(set(q) == {0xFF} for q in quals_of) == fasta


def test_a_mapped_line_without_cigar_gets_flag_4(workdir):
    """a shown report without CIGAR ops: the formatter prints an empty column, the writer marks the read unmapped"""
    c = common.build_case("pe101_spliced", workdir)
    seqs, headers, quals = sdi.edge_reads(c["genome"])
    so, rl, flat = host.pack_reads(seqs)
    R, P, cig = bdi.edge_records()
    P = P.copy(); P["n_cigar"][int(R[8]["rep_off"])] = 0
    rec, seen = _check(workdir, "edge_nocigar", (R, P, cig, None), so, rl, flat, headers, quals, ["chrA", "c" * 300], 12, False, False, seqs)
    assert seen["flag4"] == 1
    assert any(f[6] == (73 | 4) and f[5] == 0 and f[0] == 0 for f, _ in bdi.records_of(rec))


def test_lane_code_under_the_sanitizers(workdir):
    """the same program built with AddressSanitizer and UBSan for its host side, run stand-alone on the edge batch"""
    exe = bdi.build_lane_program(workdir, sanitize=True)
    res, so, rl, flat, headers, quals, names, npm, unique, multi, seqs = _edge_batch(workdir, False, True, False)
    path = os.path.join(workdir, "bam_batch_edge_san.bin")
    sdi.write_batch(path, res[0], res[1], res[2], so, rl, flat, headers, quals, names, npm, unique, multi)
    r = subprocess.run([exe, "records", path, path + ".out"], capture_output=True, text=True)
    assert r.returncode == 0 and "bad 0" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr[-2000:]
    r = subprocess.run([exe, "tokens", path + ".tokens"], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-2000:]


def test_every_length_and_distance_code_inflates(workdir):
    """one match token per stream: every length 3..258 and every boundary of the distance codes (1, 2, 3, 4, 5, 7, 9, ... 24577, 32768, each with its
    neighbours), coded by dg_bgzf.h's token-to-bits function with the fixed Huffman codes, inflated by zlib"""
    exe = bdi.build_lane_program(workdir)
    out = os.path.join(workdir, "bam_tokens.bin")
    r = subprocess.run([exe, "tokens", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    lits = bytes((((i * 2654435761) & 0xFFFFFFFF) >> 23) & 0xFF for i in range(32768))
    p = 0; seen_len, seen_dist = set(), set()
    while p < len(raw):
        ln, dist, nb = np.frombuffer(raw, np.uint32, 3, p); p += 12
        stream = raw[p:p + int(nb)]; p += int(nb)
        want = bytearray(lits[:int(dist)])
        for _ in range(int(ln)):
            want.append(want[-int(dist)])
        got = zlib.decompress(stream, -15)
        assert got == bytes(want), (int(ln), int(dist))
        seen_len.add(int(ln)); seen_dist.add(int(dist))
    assert seen_len == set(range(3, 259))
    bounds = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577, 32768]
    assert set(bounds) <= seen_dist and {b - 1 for b in bounds[1:]} <= seen_dist


def test_crc_of_split_buffers_equals_zlib(workdir):
    exe = bdi.build_lane_program(workdir)
    rng = np.random.default_rng(5)
    for n, cuts in ((0, []), (1, []), (1, [0]), (1, [1]), (255, [100]), (256, [1, 2, 255]), (257, [256]), (0xFF00, [1, 0x8000, 0xFEFF]), (0xFF00 - 1, [0x7FFF, 0x7FFF]), (1000, [0, 0, 500, 1000])):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        path = os.path.join(workdir, "bam_crc_%d.bin" % n)
        open(path, "wb").write(data)
        r = subprocess.run([exe, "crc", path] + [str(c) for c in cuts], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        want = "%08x" % (zlib.crc32(data) & 0xFFFFFFFF)
        assert r.stdout.split() == [want, want], (n, cuts, r.stdout, want)


def _text(n, seed=1):
    rng = np.random.default_rng(seed)
    words = [b"the", b"read", b"maps", b"to", b"chromosome", b"twenty", b"with", b"a", b"junction", b"and", b"its", b"mate", b"quality", b"of", b"alignment,", b"spliced.", b"score"]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + b" "
    return bytes(out[:n])


def test_deflate_lane_functions_in_the_kernels_order(workdir):
    """k_bgzf_deflate's per-lane functions (token choice, bits into the slot, table inserts) run on the host lane after lane, phase after phase: text,
    noise (stored: input + 31 bytes), a run of one byte, a phrase at distance 32768 and 32769, repeats over the strip and segment seams, and BAM records
    -- every block inflated by zlib, CRC32 and ISIZE checked (bam_decode.bgzf_blocks)"""
    exe = bdi.build_lane_program(workdir)
    rng = np.random.default_rng(11)
    noise = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    B = bdi.BLOCK
    phrase = _text(300, seed=9)
    cases = {"t1": _text(1), "t2": _text(2), "t3": _text(3), "t258": _text(258), "tb-1": _text(B - 1), "tb": _text(B), "tb+1": _text(B + 1), "t3b+7": _text(3 * B + 7),
             "noise": np.random.default_rng(0).integers(0, 256, B, dtype=np.uint8).tobytes(), "run": b"I" * B,
             "far32768": noise(100) + phrase + noise(32768 - 300) + phrase + noise(50), "far32769": noise(100) + phrase + noise(32769 - 300) + phrase + noise(50)}
    for dist in (32768, 32769):                               # a filler that leaves the phrase's table entries alone: the far copy is the only candidate
        piece = noise(300)
        cases["zfar%d" % dist] = bytes(100) + piece + bytes(dist - 300) + piece + bytes(50)
        cases["tfar%d" % dist] = _text(100, 2) + piece + _text(dist - 300, 3) + piece + _text(50, 4)
    for k in (259, 600):
        piece = noise(k)
        cases["rep%d" % k] = noise(10000) + piece + noise(9000) + piece + noise(77) + piece + piece
    for seam in (8192, 16384, 8192 + 32, 96, 8192 - 32):
        for shift in (-1, 0, 1):
            piece = noise(40)
            a = bytearray(_text(3 * 8192 + 500, seed=seam + shift)); at = max(0, seam + shift - 20)
            a[at:at + 40] = piece; a[17000:17040] = piece; a[5:45] = piece
            cases["seam%d%+d" % (seam, shift)] = bytes(a)
    c = common.build_case("pe101_spliced", workdir)
    res, so, rl, flat, headers, quals, names, npm, unique, multi, seqs = _edge_batch(workdir, False, True, False)
    path = os.path.join(workdir, "bam_batch_for_deflate.bin")
    sdi.write_batch(path, res[0], res[1], res[2], so, rl, flat, headers, quals, names, npm, unique, multi)
    cases["records"] = bdi.run_lane_program(exe, path)[2] * 40
    for name, data in cases.items():
        src = os.path.join(workdir, "bam_deflate_in.bin"); out = os.path.join(workdir, "bam_deflate_out.bin")
        open(src, "wb").write(data)
        r = subprocess.run([exe, "deflate", src, out], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stdout, r.stderr)
        z = open(out, "rb").read()
        blocks = bam_decode.bgzf_blocks(z)
        n_blocks = (len(data) + B - 1) // B
        assert b"".join(b for b, _ in blocks) == data, name
        assert len(blocks) == n_blocks and all(sz <= 65536 for _, sz in blocks) and len(z) <= len(data) + 31 * n_blocks, name
        if name == "noise":
            assert blocks[0][1] == B + 31
        if name == "run":                                     # runs of 258: about B / 256 tokens of 18 bits (3599 bytes if no match outgrew its 32-byte segment)
            assert len(z) < 1000, len(z)
        if name in ("tb", "t3b+7", "run", "records"):
            assert len(z) < 0.8 * len(data), (name, len(z), len(data))
        print("%s: %d -> %d bytes" % (name, len(data), len(z)))
