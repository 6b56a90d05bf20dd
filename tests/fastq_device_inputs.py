"""Helpers of the device FASTQ parser's tests: an awkward FASTQ text, a Python restatement of the reference's reader (GetNextEntry / GetNextChunk,
GetData.cpp:55-179) that says what the batch must hold, and the driver of tests/native/fastq_checks.hip."""
from __future__ import annotations

import os, subprocess
import numpy as np
import common


# ---- the text -------------------------------------------------------------------------------------------------------------------------------
def rec(i, seq, tag):
    """one record of tests/test_gpu_cli.py::test_dart_cli_awkward_fastq (a copy of its generator): headers with blanks / slashes / tabs and repeated
    '@', quality lines that start with '@' or '+', qualities longer than the read, lower-case and IUPAC bases"""
    s = seq.tobytes().decode()
    if i % 7 == 1: s = s[:40].lower() + s[40:]
    if i % 11 == 2: s = s[:10] + "R" + s[11:]
    q = "".join(chr(33 + (i * 7 + k * 3) % 41) for k in range(len(s)))
    if i % 5 == 0: q = "@" + q[1:]
    if i % 13 == 3: q = "+" + q[1:]
    if i % 19 == 5: q = q + "IIII"
    h = ["@r%d/%s" % (i, tag), "@@r%d extra words" % i, "@r%d\tx" % i, "@r%d" % i][i % 4]
    return "%s\n%s\n+%s\n%s\n" % (h, s, "" if i % 3 else h[1:], q)


def random_reads(n, rlen=101, seed=5):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n, rlen))]


def extra_records(tag):
    """a 1-base read, a 1000-base read, a 5000-byte name, a name that trims to empty, a quality shorter than its read, a quality with a NUL, CRLF line ends"""
    long_seq = "".join("ACGT"[(k * k + 3 * k) % 4] for k in range(1000))
    return [
        "@one/%s\nG\n+\nI\n" % tag,
        "@thousand/%s\n%s\n+\n%s\n" % (tag, long_seq, "F" * 1000),
        "@%s %s\n%s\n+\n%s\n" % ("N" * 5000, tag, "ACGTTGCAAC" * 6, "5" * 60),
        "@@@\n%s\n+\n%s\n" % ("TTGACCAGTA" * 5, "6" * 50),
        "@shortq/%s\n%s\n+\n%s\n" % (tag, "GATTACAGAT" * 5, "7" * 20),
        "@nulq/%s\n%s\n+\n%s\n" % (tag, "CCATGGTTAA" * 4, "8" * 15 + "\0" + "9" * 24),
        "@crlf%s\r\n%s\r\n+\r\n%s\r\n" % (tag, "ACGGTCATGC" * 3, "A" * 30),
    ]


def awkward_texts(m1, m2):
    """-> (file 1, file 2, both interleaved) as bytes: rec() records with the extra ones spread between them; file 1 and the interleaved text end
    without a newline"""
    n = m1.shape[0]
    def file_of(m, tag):
        out, ex = [], extra_records(tag)
        for i in range(n):
            out.append(rec(i, m[i], tag))
            if i % 5 == 2 and ex:
                out.append(ex.pop(0))
        return out + ex
    r1, r2 = file_of(m1, "1"), file_of(m2, "2")
    inter = "".join(a + b for a, b in zip(r1, r2))
    return "".join(r1)[:-1].encode("latin1"), "".join(r2).encode("latin1"), inter[:-1].encode("latin1")


# ---- the reference's reader, restated ----------------------------------------------------------------------------------------------------------
class _File:
    """FILE* with getline: the line up to and including its newline, or what is left; None at the end"""
    def __init__(self, data: bytes):
        self.d, self.p = data, 0

    def getline(self):
        if self.p >= len(self.d):
            return None
        e = self.d.find(b"\n", self.p)
        e = len(self.d) if e < 0 else e + 1
        line, self.p = self.d[self.p:e], e
        return line


def identify_header_beg_pos(s: bytes, n: int) -> int:        # GetData.cpp:55-64
    for i in range(1, n):
        if s[i] not in b">@":
            return i
    return n - 1


def identify_header_end_pos(s: bytes, n: int) -> int:        # GetData.cpp:66-75
    for i in range(1, n):
        if s[i] in b" /\t":
            return i
    return n - 1


def get_next_entry(f: _File):
    """GetNextEntry (GetData.cpp:77-132), FASTQ branch -> (header, seq, qual, rlen); rlen 0: no entry.  Where the reference's C strings and ours part:
    the name is empty when its end does not lie behind its begin (:89-90 would pass a negative length to new[]); the stored quality keeps the file's
    bytes behind a NUL (strncpy, :100, pads with NUL there; they are never printed)."""
    buf = f.getline()
    if buf is None:
        return None, None, None, 0
    p1, p2 = identify_header_beg_pos(buf, len(buf)), identify_header_end_pos(buf, len(buf))
    header = buf[p1:p2] if p2 > p1 else b""
    buf = f.getline()
    if buf is None:
        return header, None, None, 0
    rlen = len(buf)                                           # :95 the line's length, newline included
    seq = buf[:rlen]
    f.getline()                                               # :99 the '+' line is not looked at
    q = f.getline()
    q = b"" if q is None else q
    rlen -= 1                                                 # :101
    return header, seq[:rlen], q[:rlen], rlen


COMP = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")


def get_complementary_seq(s: bytes) -> bytes:                # tools.cpp:3-17,19-27: the reverse, every base through comp_base
    return bytes(COMP[c] if c in b"ACGTacgt" else ord("N") for c in reversed(s))


def reference_reads(text1: bytes, text2, pair_end: bool):
    """GetNextChunk (GetData.cpp:134-179) over the whole input -- its chunk limits (:176) only decide where a chunk ends -- -> [(name, stored read,
    stored quality)]; the stream ends at the first entry without bases.  text2 None: one file.  A stored quality shorter than its read is reversed as the
    bytes it has (the reference reverses a C string and copies rlen bytes out of it, :165-166: undefined behind its end)."""
    f1 = _File(text1); f2 = _File(text2) if text2 is not None else f1
    out = []
    while True:
        h, s, q, rlen = get_next_entry(f1)
        if rlen <= 0:
            break
        out.append((h, s, q))
        h, s, q, rlen = get_next_entry(f2)
        if rlen <= 0:
            break
        if pair_end:
            s, q = get_complementary_seq(s), q[::-1]
        out.append((h, s, q))
    return out


# ---- the lane code on the host ---------------------------------------------------------------------------------------------------------------------
def build_checks_program(workdir):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "fastq_checks")
    if not os.path.exists(exe):
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w", "-o", exe, os.path.join(common.ROOT, "tests", "native", "fastq_checks.hip")])
    return exe


def run_checks_program(exe, path, text1: bytes, text2, rc_odd: bool):
    """-> (status, [(name, stored read, stored quality)]); status: 0, or -1 when the record counts of two texts do not fit"""
    t2 = text2 if text2 is not None else b""
    with open(path, "wb") as f:
        f.write(np.asarray([int(text2 is not None), int(rc_odd), len(text1), len(t2)], np.int64).tobytes())
        for t in (text1, t2):
            f.write(t + b"\0" * (-len(t) % 8))
    r = subprocess.run([exe, path, path + ".out"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(path + ".out", "rb").read()
    n = int(np.frombuffer(raw, np.int64, 1)[0])
    if n < 0:
        return -1, []
    rl = np.frombuffer(raw, np.int64, n, 8); hl = np.frombuffer(raw, np.uint32, n, 8 + 8 * n); ql = np.frombuffer(raw, np.uint32, n, 8 + 12 * n)
    at = 8 + 16 * n
    out = []
    for k in range(n):
        r_ = max(int(rl[k]), 0)
        s = raw[at:at + r_]; at += r_
        h = raw[at:at + int(hl[k])]; at += int(hl[k])
        q = raw[at:at + int(ql[k])]; at += int(ql[k])
        out.append((h, s, q) if rl[k] > 0 else (h, None, None))
    assert at == len(raw)
    return 0, out


def seam_texts(tile: int):
    """texts of about three tiles of the device's line kernels: a newline as the last byte of a tile, as the first byte of the next, a record header
    starting exactly at a tile start, a text whose length is an exact multiple of the tile; the record in front of the seam is stretched by its
    name to put the seam where it is wanted -> [(label, text)]"""
    m = random_reads(400, rlen=75, seed=11)
    def build(target, what, total=None):
        # records until the next one would cross `target`; then one whose name is padded so that `what` falls on the seam
        out, size, i = [], 0, 0
        def plain(i):
            return "@s%d\n%s\n+\n%s\n" % (i, m[i % 400].tobytes().decode(), "H" * 75)
        while True:
            r = plain(i)
            if size + len(r) + 160 > target:
                break
            out.append(r); size += len(r); i += 1
        # the padded record: "@" + pad + "\n" + seq + "\n+\n" + qual + "\n"; offsets of its four line ends from its start: L0 = len(pad) + 1 (the newline
        # is byte L0), ...
        if what == "nl_last":            # the header's newline is the last byte of the tile: size + 1 + pad == target - 1
            pad = target - 1 - size - 1
        elif what == "nl_first":         # the header's newline is the first byte of the next tile
            pad = target - size - 1
        else:                            # "header_at_start": the record behind the padded one begins at the tile start
            pad = target - size - (1 + 1 + 75 + 3 + 75 + 1)
        assert pad > 0
        out.append("@%s\n%s\n+\n%s\n" % ("p" * pad, m[i % 400].tobytes().decode(), "H" * 75)); i += 1
        text = "".join(out)
        while len(text) < 3 * tile - 400:
            text += plain(i); i += 1
        if total is not None:            # a last record stretched to the exact length
            base = "@\n%s\n+\n%s\n" % (m[i % 400].tobytes().decode(), "H" * 75)
            pad = total - len(text) - len(base)
            assert pad > 0
            text += "@%s\n%s\n+\n%s\n" % ("e" * pad, m[i % 400].tobytes().decode(), "H" * 75)
            assert len(text) == total
        return text.encode("latin1")
    out = []
    for seam in (tile, 2 * tile):
        t = build(seam, "nl_last"); assert t[seam - 1:seam] == b"\n"; out.append(("nl_last_%d" % seam, t))
        t = build(seam, "nl_first"); assert t[seam:seam + 1] == b"\n" and t[seam - 1:seam] != b"\n"; out.append(("nl_first_%d" % seam, t))
        t = build(seam, "header_at_start"); assert t[seam - 1:seam + 2] == b"\n@s"; out.append(("header_at_start_%d" % seam, t))
    t = build(tile, "nl_last", total=3 * tile); assert len(t) == 3 * tile and t.endswith(b"\n"); out.append(("exact_multiple", t))
    t = build(tile, "nl_first", total=3 * tile + 5)[:-1]; out.append(("multiple_plus_4_no_newline", t))
    t = build(2 * tile, "header_at_start", total=3 * tile - 3); out.append(("multiple_minus_3", t))
    return out
