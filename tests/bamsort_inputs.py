"""Helpers of the coordinate-sorted BAM tests: hand-made BAM records, the Python twin of the order dart_amd/csrc/dg_bamsort.h defines (the key, the
checked walk, sorted() -- which is stable -- over segments in ordinal order), the native program tests/native/bamsort_checks.hip, and the read set
both GPU suites sort.  The order is the definition in dg_bamsort.h's header comment: no samtools exists where these tests run."""
from __future__ import annotations

import os, struct, subprocess
import numpy as np
import common

BLOCK = 0xFF00
OK, TRUNCATED, SIZE, NAME, REFID, POS = 0, 1, 2, 3, 4, 5       # dg_bamsort.h: BS_REC_*


def record(refid, pos, flag, name=b"r", n_cigar=0, l_seq=0, mapq=0, tags=b"", fill=0):
    """one uncompressed BAM record with its block_size; CIGAR ops are 1M each, bases and qualities are `fill`"""
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(name) + 1, mapq, 4680, n_cigar, flag, l_seq, -1, -1, 0)
    body += name + b"\0" + struct.pack("<%dI" % n_cigar, *([1 << 4] * n_cigar)) + bytes([fill]) * ((l_seq + 1) // 2) + bytes([fill]) * l_seq + tags
    return struct.pack("<i", len(body)) + body


def key(rec: bytes, n_chr: int, at: int = 0) -> int:
    refid, pos = struct.unpack_from("<ii", rec, at + 4)
    flag = struct.unpack_from("<H", rec, at + 18)[0]
    tid = refid if 0 <= refid < n_chr else n_chr
    return tid << 33 | ((pos + 1) & 0xFFFFFFFF) << 1 | (flag >> 4 & 1)


def key_bits(n_chr: int) -> int:
    return 33 + int(n_chr).bit_length()


def walk_checked(data: bytes, n_chr: int):
    """-> (why, index of the first bad record, offsets of the records before it)"""
    at, offs = 0, []
    while at < len(data):
        left = len(data) - at
        if left < 4:
            return TRUNCATED, len(offs), offs
        bs = struct.unpack_from("<I", data, at)[0]
        if bs < 32:
            return SIZE, len(offs), offs
        if bs > left - 4:
            return TRUNCATED, len(offs), offs
        l_name = data[at + 12]; n_cigar = struct.unpack_from("<H", data, at + 16)[0]; l_seq = struct.unpack_from("<I", data, at + 20)[0]
        if bs < 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq:
            return SIZE, len(offs), offs
        if l_name == 0:
            return NAME, len(offs), offs
        refid, pos = struct.unpack_from("<ii", data, at + 4)
        if refid >= n_chr:
            return REFID, len(offs), offs
        if pos < -1:
            return POS, len(offs), offs
        offs.append(at)
        at += 4 + bs
    return OK, 0, offs


def split(raw: bytes):
    """whole records the library wrote itself -> [record bytes]"""
    out, p = [], 0
    while p < len(raw):
        bs = struct.unpack_from("<I", raw, p)[0]
        assert bs >= 32 and p + 4 + bs <= len(raw)
        out.append(raw[p:p + 4 + bs]); p += 4 + bs
    return out


def expected_sorted(segments, n_chr: int):
    """segments = [(ordinal, record bytes)] in call order -> the records of all of them: ascending ordinal (equal ordinals in call order), then stable by key"""
    recs = []
    for _, data in sorted(segments, key=lambda s: s[0]):
        recs += split(data)
    return sorted(recs, key=lambda r: key(r, n_chr))


def crafted_segments(n_chr: int):
    """[(ordinal, bytes)] in call order, ordinals not ascending: every corner of the key and of a record's layout"""
    last = n_chr - 1
    a = [record(last, 2 ** 31 - 2, 16, b"far_rev"), record(last, 2 ** 31 - 2, 0, b"far_fwd"), record(-1, -1, 4, b"unplaced"), record(0, -1, 0, b"pos_m1"),
         record(0, 0, 0, b"pos0"), record(0, 0, 16, b"pos0_rev"), record(0, 0, 0, b"pos0_again"), record(-1, 77, 4, b"unplaced_with_pos"),
         record(0, 500, 16, b"x"), record(0, 500, 0, b"n" * 254), record(0, 500, 0, b"cig300", n_cigar=300, l_seq=10), record(0, 500, 0, b"seq1000", l_seq=1000, fill=0x11),
         record(0, 500, 0, b"odd_seq", l_seq=7, tags=b"NMC\x01")]
    tie = lambda tag: record(last, 1234, 0, b"tie_" + tag, l_seq=5)
    b = [tie(b"b0"), record(0, 1, 0, b"early"), tie(b"b1"), tie(b"b2")]       # three identical keys inside one ordinal
    c = [tie(b"c0"), record(-1, -1, 4, b"unplaced_c")]                         # and the same key under other ordinals
    d = [tie(b"d0")]
    e = [record(-5, 3, 0, b"negative_refid_is_unplaced")]
    return [(7, b"".join(a)), (3, b"".join(b)), (9, b"".join(c)), (1, b"".join(d)), (3, b"".join(e))]


def malformed_cases(n_chr: int):
    """name -> (bytes, why, index of the bad record): each with two good records in front"""
    good = record(0, 5, 0, b"g0") + record(0, 4, 16, b"g1", l_seq=3)
    r = record(0, 9, 0, b"victim", n_cigar=2, l_seq=8)
    small = bytearray(r); struct.pack_into("<I", small, 0, len(r) - 4 - 1); small = bytes(small[:-1])      # block_size one short of its fields
    noname = bytearray(record(0, 9, 0, b"")); assert noname[12] == 1; noname[12] = 0
    return {
        "truncated": (good + r[:-3], TRUNCATED, 2),
        "truncated_in_block_size": (good + r[:2], TRUNCATED, 2),
        "block_size_too_small": (good + small + record(0, 1, 0), SIZE, 2),
        "block_size_below_32": (good + struct.pack("<I", 31) + bytes(31), SIZE, 2),
        "refid_is_n_chr": (good + record(n_chr, 9, 0), REFID, 2),
        "pos_minus_2": (good + record(0, -2, 0), POS, 2),
        "no_name": (good + bytes(noname), NAME, 2),
        "bad_first": (record(0, -2, 0) + good, POS, 0),
    }


# ---- the native program ----
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "bamsort_checks_san" if sanitize else "bamsort_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "bamsort_checks.hip")])
    return exe


def run_program(exe, workdir, tag, n_chr, segments):
    """-> (per segment dict(why, bad, n, range), [per accepted segment [(key, offset)]], order, bits, sorted bytes)"""
    pad = lambda b: b + bytes(-len(b) % 8)
    src = os.path.join(workdir, "bamsort_%s.in" % tag); txt = os.path.join(workdir, "bamsort_%s.txt" % tag); out = os.path.join(workdir, "bamsort_%s.bin" % tag)
    with open(src, "wb") as f:
        f.write(struct.pack("<qq", n_chr, len(segments)))
        for ordinal, data in segments:
            f.write(struct.pack("<qq", ordinal, len(data)) + pad(data))
    r = subprocess.run([exe, src, txt, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    segs, recs, order, bits, tail = [], [], None, None, None
    for line in open(txt).read().splitlines():
        w = line.split()
        if w[0] == "seg":
            segs.append(dict(why=int(w[3]), bad=int(w[5]), n=int(w[7]), range=int(w[9])))
            if int(w[3]) == OK:
                recs.append([])
        elif w[0] == "rec":
            recs[-1].append((int(w[1]), int(w[2])))
        elif w[0] == "order":
            order = [int(x) for x in w[1:]]
        elif w[0] == "bits":
            bits = int(w[1])
        elif w[0] == "sorted":
            tail = (int(w[1]), int(w[2]))
    data = open(out, "rb").read()
    assert tail == (sum(len(x) for x in recs), len(data))
    return segs, recs, order, bits, data


# ---- the reads both GPU suites sort: a golden case plus what makes the order non-trivial ----
def sort_reads(case, n_random: int = 6, seed: int = 11):
    """-> (reads array, headers, quals): the case's pairs, then pair 0 three more times under other names (tie groups of four), a few pairs of random
    sequence (unmapped: refID -1), and a pair whose second mate is random (its mate is unmapped)"""
    rng = np.random.default_rng(seed)
    reads = case["reads"]; L = reads.shape[1]
    rows = [reads]; headers = list(case["headers"])
    for k in range(3):
        rows.append(reads[0:2]); headers += ["copy%d" % k] * 2
    noise = lambda: np.frombuffer(bytes(rng.choice(list(b"ACGT"), L).tolist()), np.uint8)
    for k in range(n_random):
        rows.append(np.stack([noise(), noise()])); headers += ["noise%d" % k] * 2
    rows.append(np.stack([reads[2], noise()])); headers += ["half"] * 2
    arr = np.ascontiguousarray(np.concatenate(rows))
    return arr, headers, ["I" * L] * len(arr)
