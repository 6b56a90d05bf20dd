"""Helpers of the device BAM writer's tests: the two native programs (tests/native/bam_lane_checks.hip: the device's per-read code on the host;
tests/native/bam_raw_checks.cpp: the host writer over SAM text), the hand-made edge records, BAM files made of loose pieces for tests/bam_decode.py,
and the golden SAM as a BAM file stores it."""
from __future__ import annotations

import os, re, struct, subprocess, zlib
import numpy as np
import common
from dart_amd import host

BLOCK = 0xFF00
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _hipcc():
    import __graft_entry__ as ge
    return ge.HIPCC


def build_lane_program(workdir, sanitize=False):
    exe = os.path.join(workdir, "bam_lane_checks_san" if sanitize else "bam_lane_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([_hipcc(), "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "bam_lane_checks.hip")])
    return exe


def build_raw_program(workdir):
    exe = os.path.join(workdir, "bam_raw_checks")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(common.ROOT, "dart_amd", "csrc", "host"), "-o", exe,
                               os.path.join(common.ROOT, "tests", "native", "bam_raw_checks.cpp"), "-lz", "-ldl"])
    return exe


def run_lane_program(exe, batch_path):
    """-> (per-read lengths u64, counters [unmapped, unique, paired, records, refused], record bytes)"""
    out = batch_path + ".bam_out"
    r = subprocess.run([exe, "records", batch_path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    n = int(np.fromfile(batch_path, np.int32, 1)[0])
    lens = np.frombuffer(raw, np.uint64, n)
    tail = np.frombuffer(raw, np.uint64, 6, 8 * n)
    rec = raw[8 * n + 48:]
    assert len(rec) == int(tail[5])
    return lens, [int(x) for x in tail[:5]], rec


def host_writer_bytes(workdir, tag, chr_names, sam_body: bytes):
    """BamWriter::sam_line_to_bam over every line of a SAM body -> (concatenated records, records, refused)"""
    exe = build_raw_program(workdir)
    names = os.path.join(workdir, "bam_raw_%s.names" % tag); body = os.path.join(workdir, "bam_raw_%s.sam" % tag); out = os.path.join(workdir, "bam_raw_%s.bin" % tag)
    open(names, "w").write("".join(n + "\n" for n in chr_names))
    open(body, "wb").write(sam_body)
    r = subprocess.run([exe, names, body, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"records=(\d+) refused=(\d+)", r.stdout)
    return open(out, "rb").read(), int(m.group(1)), int(m.group(2))


def edge_records():
    """hand-made records for the edge batch of sam_device_inputs.edge_reads (6 pairs + a single tail): several reports per read, both strands, a negative
    POS and negative distances, an unmapped mate, a low MAPQ for -unique, a CIGAR of 150 ops, a POS beyond 32 bits"""
    R = np.zeros(13, host.READ_OUT); P = []; cig = []
    def report(aln, sj, flag, pidx, ch, bdir, pos, ops):
        P.append((aln, sj, flag, pidx, ch, bdir, pos, len(cig), len(ops))); cig.extend(ops)
    def read(k, score, sub, mis, mapq, best, reps):
        R[k]["score"], R[k]["sub_score"], R[k]["mis_num"], R[k]["mapq"], R[k]["best"] = score, sub, mis, mapq, best
        R[k]["rep_off"], R[k]["n_rep"] = len(P), len(reps)
        for r in reps:
            report(*r)
    M = lambda l: (l << 4)
    read(0, 101, 0, 0, 50, 0, [(101, -1, 99, 0, 0, 1, 1000, [M(101)]), (90, 0, 355, -1, 1, 0, 77, [M(50), (1200 << 4) | 3, M(51)])])
    read(1, 101, 0, 1, 50, 0, [(101, -1, 147, 0, 0, 0, 1200, [M(101)])])
    read(2, 1000, 10, 2, 50, 1, [(0, -1, 0, -1, 0, 1, 5, [M(1000)]), (1000, 1, 97, 0, 1, 1, -3, [M(400), (2 << 4) | 1, (7 << 4) | 2, M(598)])])
    read(3, 101, 0, 0, 50, 0, [(101, 2, 145, 1, 1, 1, 250, [(5 << 4) | 4, M(96)])])
    read(4, 80, 80, 3, 0, 0, [(80, 3, 65, 0, 0, 0, 500, [M(1)] * 150), (80, -1, 321, -1, 0, 1, 900, [M(101)])])
    read(5, 1, 0, 0, 2, 0, [(1, -1, 129, 0, 0, 0, 90000, [M(1)])])
    read(6, 0, 0, 0, 0, 0, [(0, -1, 77, -1, -1, 0, 0, [])])
    read(7, 0, 0, 0, 0, 0, [(0, -1, 141, -1, -1, 0, 0, [])])
    read(8, 101, 90, 0, 3, 0, [(101, -1, 73, 0, 0, 1, 10, [M(101)])])
    read(9, 0, 0, 0, 0, 0, [(0, -1, 133, -1, -1, 0, 0, [])])
    read(10, 60, 60, 1, 1, 0, [(0, -1, 0, -1, 0, 1, 1, [M(101)]), (60, 1, 99, 0, 1, 0, 4000000000, [M(101)])])
    read(11, 60, 0, 0, 50, 0, [(60, 0, 147, 1, 1, 0, 3999999000, [M(101)])])
    read(12, 101, 101, 0, 0, 0, [(50, -1, 0, -1, 0, 1, 3, [M(101)]), (101, 0, 16, -1, 1, 0, 20001, [M(101)]), (101, 1, 256, -1, 0, 1, 5, [M(101)])])
    return R, np.asarray(P, host.REPORT_OUT), np.asarray(cig, np.uint32)


def records_of(raw: bytes):
    """the uncompressed records one by one -> [(fields of struct '<iiBBHHHiiii', record bytes behind block_size)]"""
    out, p = [], 0
    while p < len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]
        rec = raw[p + 4:p + 4 + bs]
        assert len(rec) == bs and bs >= 32
        out.append((struct.unpack_from("<iiBBHHHiiii", rec, 0), rec))
        p += 4 + bs
    return out


def bam_header(header_text: str, names, lens) -> bytes:
    h = b"BAM\x01" + struct.pack("<i", len(header_text)) + header_text.encode()
    h += struct.pack("<i", len(names))
    for n, l in zip(names, lens):
        h += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", int(l))
    return h


def stored_bgzf(data: bytes) -> bytes:
    """data as BGZF blocks that hold it uncompressed (zlib level 0)"""
    out = b""
    for o in range(0, len(data), BLOCK):
        piece = data[o:o + BLOCK]
        co = zlib.compressobj(0, zlib.DEFLATED, -15)
        body = co.compress(piece) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(body) + 8 - 1) + body + struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece))
    return out


def bam_file(names, lens, record_blocks: bytes, header_text: str = "") -> bytes:
    """a BAM file around BGZF blocks of records: the header in blocks of its own in front, the end-of-file block behind"""
    return stored_bgzf(bam_header(header_text, names, lens)) + record_blocks + EOF_BLOCK


def golden_as_bam_stores_it(sam_text: str):
    """the lines of a golden SAM body the way they read back from BAM (tests/test_host_text.py): the blank-joined strand tag is lost, a base is one of
    sixteen codes (case is lost, everything but "=ACMGRSVTWYHKDBN" reads back as N)"""
    want = []
    for l in sam_text.splitlines():
        if not l or l.startswith("@"):
            continue
        f = re.sub(r" XS:A:[+-]$", "", l).split("\t")
        if len(f) > 9 and f[9] != "*":
            f[9] = "".join(ch if ch in "=ACMGRSVTWYHKDBN" else "N" for ch in f[9].upper())
        want.append("\t".join(f))
    return want


def host_deflate(workdir, data: bytes) -> bytes:
    """data as BGZF blocks through k_bgzf_deflate's lane functions on the host (bam_lane_checks deflate)"""
    exe = build_lane_program(workdir)
    src = os.path.join(workdir, "bam_host_deflate_in.bin"); out = os.path.join(workdir, "bam_host_deflate_out.bin")
    open(src, "wb").write(data)
    r = subprocess.run([exe, "deflate", src, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(out, "rb").read()
