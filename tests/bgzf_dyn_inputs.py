"""Helpers of the dynamic-Huffman BGZF coder's tests: the native program (tests/native/bgzf_dyn_checks.hip: the kernel's lane functions on the host), the
inputs both suites use, the histograms of the length builder's tests, and the record bytes of the golden SAM files."""
from __future__ import annotations

import gzip, os, re, subprocess
import numpy as np
import common
import bam_device_inputs as bdi

BLOCK = bdi.BLOCK
STRIP = 8192
COUNTERS = ("dynamic", "fixed", "stored", "repairs", "nodist", "onedist", "blocks")


def build_program(workdir, sanitize=False):
    exe = os.path.join(workdir, "bgzf_dyn_checks_san" if sanitize else "bgzf_dyn_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([bdi._hipcc(), "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "bgzf_dyn_checks.hip")])
    return exe


def host_deflate_dyn(workdir, data: bytes, sanitize=False):
    """data as BGZF blocks through k_bgzf_deflate_dyn's lane functions on the host -> (bytes, {counter: how often the fork ran})"""
    exe = build_program(workdir, sanitize)
    src = os.path.join(workdir, "bgzf_dyn_in.bin"); out = os.path.join(workdir, "bgzf_dyn_out.bin")
    open(src, "wb").write(data)
    r = subprocess.run([exe, "deflate", src, out], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
    w = r.stdout.split()
    ct = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
    assert tuple(ct) == COUNTERS, r.stdout
    return open(out, "rb").read(), ct


def host_lengths(workdir, freq, limit, sanitize=False):
    """the length builder on a histogram -> (lengths, 1 when lengths were cut to the limit)"""
    exe = build_program(workdir, sanitize)
    r = subprocess.run([exe, "lengths", str(limit)] + [str(int(f)) for f in freq], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])
    first, second = r.stdout.splitlines()
    return [int(x) for x in second.split()], int(first.split()[1])


def text(n, seed=1):
    """English-like text: words of a small vocabulary in random order (the _text of the fixed coder's tests)"""
    rng = np.random.default_rng(seed)
    words = [b"the", b"read", b"maps", b"to", b"chromosome", b"twenty", b"with", b"a", b"junction", b"and", b"its", b"mate", b"quality", b"of", b"alignment,", b"spliced.", b"score"]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + b" "
    return bytes(out[:n])


TEXT_SIZES = [1, 2, 3, 258, STRIP - 1, STRIP, STRIP + 1, STRIP + 5, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7]


def edge_alphabets():
    """one block each -> {name: bytes}"""
    rng = np.random.default_rng(21)
    noise = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    four = bytearray()
    while len(four) < STRIP:                                  # four values, never one of them three times in a row: the first strip's only candidate is distance 1
        v = int(rng.integers(0, 4)) + 65
        if len(four) < 2 or not (four[-1] == v and four[-2] == v):
            four.append(v)
    return {"one_value": b"I" * STRIP, "four_values": bytes(four), "all_256": bytes(range(256)) * 4 + text(STRIP - 1024, 3), "noise": noise(BLOCK),
            # the dynamic code writes noise at a little over 8 bits a byte, so a strip of text in front keeps the whole block coded ...
            "text_then_noise": text(STRIP) + noise(BLOCK - STRIP),
            # ... and a few words in front do not: their gain is spent on the first headers, the block is coded first and stored in the end
            "words_then_noise": text(200) + noise(BLOCK - 200)}


def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def histograms():
    """-> [(name, limit, frequencies)] of the length builder's tests"""
    eob_only = [0] * 286; eob_only[256] = 1
    two = [0] * 30; two[3] = 7; two[17] = 2
    one = [0] * 30; one[5] = 4
    # Fibonacci weights give the deepest tree there is; among zeros and in a scrambled order the sort and the symbol indices take part
    spread = [0] * 286
    for k, f in enumerate(fibonacci(30)):
        spread[(k * 37 + 5) % 286] = f
    return [("fib17", 15, fibonacci(17)), ("fib20", 15, fibonacci(20)), ("fib30", 15, fibonacci(30)), ("fib9", 7, fibonacci(9)), ("fib19", 7, fibonacci(19)),
            ("fib30_spread", 15, spread), ("one", 15, one), ("two", 15, two), ("equal286", 15, [5] * 286), ("eob_only", 15, eob_only)]


GOLDEN_SETS = ["pe101_spliced.run0", "pe151_spliced.run0", "odd_characters.mis12", "se100.run0"]


def golden_records(workdir, base):
    """the BAM records of a golden SAM file: the host writer over its body, the chromosome names from its @SQ lines"""
    t = gzip.open(os.path.join(common.GOLDEN, base + ".sam.gz"), "rb").read()
    lines = t.split(b"\n")
    names = [re.match(rb"@SQ\tSN:(\S+)", l).group(1).decode() for l in lines if l.startswith(b"@SQ")]
    body = b"".join(l + b"\n" for l in lines if l and not l.startswith(b"@"))
    rec, n_rec, refused = bdi.host_writer_bytes(workdir, "dyn_" + base, names, body)
    assert n_rec > 0 and refused == 0
    return rec
