"""Helpers of the device SAM formatter's tests: the flat name / quality arrays dg_batch_format_sam takes, the batch file tests/native/sam_checks.hip
reads, and the expected text from the Python twin (dart_amd/sam.py::format_records)."""
from __future__ import annotations

import os, subprocess
import numpy as np
import common
from dart_amd import host, sam


def as_bytes(x) -> bytes:
    return x if isinstance(x, (bytes, bytearray)) else x.encode("latin1")


def flatten(items):
    """list of bytes / str -> (u32 offsets [n + 1], u8 array)"""
    bs = [as_bytes(x) for x in items]
    off = np.zeros(len(bs) + 1, np.uint32)
    if bs:
        off[1:] = np.cumsum([len(x) for x in bs])
    flat = np.frombuffer(b"".join(bs), np.uint8).copy() if bs else np.zeros(0, np.uint8)
    return off, flat


def c_string(q) -> str:
    """a stored quality as the reference prints it: up to its first NUL byte"""
    return as_bytes(q).split(b"\0")[0].decode("latin1")


def twin_text(headers, seqs, quals, reads, reports, cigar, chr_names, n_pair_mode, multi=False, unique=False):
    """sam.format_records over reads [0, n_pair_mode) as pairs and the rest as single reads -> (bytes, Stats); quals None = FASTA"""
    st = sam.Stats()
    hs = [as_bytes(h).decode("latin1") for h in headers]
    ss = [as_bytes(s).decode("latin1") for s in seqs]
    qs = [c_string(q) for q in quals] if quals is not None else ["*"] * len(hs)
    out = []
    for lo, hi, paired in ((0, n_pair_mode, True), (n_pair_mode, len(hs), False)):
        if hi > lo:
            out.append(sam.format_records(hs[lo:hi], ss[lo:hi], qs[lo:hi], reads[lo:hi], reports, cigar, chr_names, paired=paired, multi_hit=multi,
                                          unique_only=unique, fastq=quals is not None, stats=st))
    return "".join(out).encode("latin1"), st


def write_batch(path, reads, reports, cigar, seq_off, rlen, flat, headers, quals, chr_names, n_pair_mode, unique, multi):
    n = len(reads)
    so = np.zeros(n + 1, np.uint32); so[:n] = seq_off
    so[n] = int(max((int(seq_off[i]) + int(rlen[i]) for i in range(n)), default=0))
    ho, hb = flatten(headers)
    qo, qb = flatten(quals) if quals is not None else (np.zeros(n + 1, np.uint32), np.zeros(0, np.uint8))
    co, cb = flatten(chr_names)
    head = np.asarray([n, len(reports), len(cigar), len(chr_names), n_pair_mode, int(unique), int(multi), int(quals is not None)], np.int32)
    with open(path, "wb") as f:
        for a in (head, np.ascontiguousarray(reads, host.READ_OUT), np.ascontiguousarray(reports, host.REPORT_OUT), np.ascontiguousarray(cigar, np.uint32),
                  so, np.ascontiguousarray(rlen, np.uint16), np.ascontiguousarray(flat, np.uint8)[:int(so[n])], ho, hb, qo, qb, co, cb):
            raw = a.tobytes()
            f.write(raw + b"\0" * (-len(raw) % 8))


def build_lane_program(workdir):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "sam_checks")
    if not os.path.exists(exe):
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w", "-o", exe, os.path.join(common.ROOT, "tests", "native", "sam_checks.hip")])
    return exe


def run_lane_program(exe, batch_path):
    """-> (per-read lengths u64, counters [unmapped, unique, paired], text bytes)"""
    out = batch_path + ".out"
    r = subprocess.run([exe, batch_path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    n = int(np.fromfile(batch_path, np.int32, 1)[0])
    lens = np.frombuffer(raw, np.uint64, n)
    tail = np.frombuffer(raw, np.uint64, 4, 8 * n)
    text = raw[8 * n + 32:]
    assert len(text) == int(tail[3])
    return lens, [int(x) for x in tail[:3]], text


def body_of(golden_text: str) -> bytes:
    """a golden SAM file without its header lines"""
    lines = golden_text.split("\n")
    k = 0
    while k < len(lines) and lines[k].startswith("@"):
        k += 1
    return "\n".join(lines[k:]).encode("latin1")


def edge_reads(genome, rng_seed=99):
    """the edge batch's reads, names and qualities: a 1-base and a 1000-base read, a 5000-byte name, a quality with a NUL in the middle, one longer than
    its read; 6 pairs and a seventh mate 1 left single.  Mate 2 comes stored (reverse-complemented, qualities reversed)."""
    from dart_amd import synth
    m1, m2 = synth.make_reads(genome, 6, rlen=101, seed=rng_seed, spliced_frac=0.5, indel_frac=0.2, n_frac=0.0)
    pairs = host.interleave_pairs(m1, m2)
    seqs = [pairs[i].tobytes() for i in range(12)]
    codes = np.asarray(genome.codes[:300000])
    long_read = bytes(b"ACGT"[int(c) & 3] for c in codes[5000:6000])
    seqs[2] = long_read                                   # a 1000-base mate 1
    seqs[5] = b"A"                                        # a 1-base mate 2
    seqs.append(bytes(b"ACGT"[int(c) & 3] for c in codes[20000:20101]))      # the single tail
    headers = [b"p%d" % (i // 2) for i in range(12)] + [b"tail"]
    headers[6] = headers[7] = b"N" * 5000
    quals = [bytes(33 + (7 * i + j) % 40 for j in range(len(s))) for i, s in enumerate(seqs)]
    quals[0] = quals[0][:40] + b"\0" + quals[0][41:]      # ends at the NUL
    quals[1] = quals[1] + b"JJJJJJJ"                      # longer than the read
    quals[3] = b"\0" + quals[3][1:]                       # empty as a C string
    return seqs, headers, quals
