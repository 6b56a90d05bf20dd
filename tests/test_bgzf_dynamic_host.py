"""CPU suite: the dynamic-Huffman mode of the device's BGZF coder (dart_amd/csrc/dg_bgzf_dyn.h), its lane functions compiled for the host and run in
the kernel's order with scrambled lanes (tests/native/bgzf_dyn_checks.hip).  Every block is inflated by zlib (tests/bam_decode.py checks CRC32 and
ISIZE); the program itself compares the exact cost each choice was made with against the bits written, and watches the slot behind the block."""
from collections import Counter
from fractions import Fraction
import numpy as np
import pytest
import bam_decode
import bam_device_inputs as bdi
import bgzf_dyn_inputs as dyn

B = dyn.BLOCK


def _check(workdir, data):
    """dynamic mode on the host: inflates to the input, within the stored bound, and per block at most 9 bytes above the fixed mode's block (the tokens are
    the same; at most 8 strips, each 3 + 7 bits more than its share of the one fixed block: 70 bits) -> (stream, counters, fixed stream)"""
    z, ct = dyn.host_deflate_dyn(workdir, data)
    blocks = bam_decode.bgzf_blocks(z)
    n_blocks = (len(data) + B - 1) // B
    assert b"".join(b for b, _ in blocks) == data
    assert len(blocks) == n_blocks == ct["blocks"] and [len(b) for b, _ in blocks] == [min(B, len(data) - i * B) for i in range(n_blocks)]
    assert all(sz <= 65536 for _, sz in blocks) and len(z) <= len(data) + 31 * n_blocks
    fixed = bdi.host_deflate(workdir, data)
    for (_, sz), (_, sz_fixed) in zip(blocks, bam_decode.bgzf_blocks(fixed)):
        assert sz <= sz_fixed + 9, (sz, sz_fixed)
    return z, ct, fixed


@pytest.mark.parametrize("n", dyn.TEXT_SIZES)
def test_blocks_of_text_inflate_to_their_input(n, workdir):
    z, ct, fixed = _check(workdir, dyn.text(n))
    print("text %d: dynamic mode %d bytes, fixed mode %d, %s" % (n, len(z), len(fixed), ct))
    strips = sum((min(B, n - o) + dyn.STRIP - 1) // dyn.STRIP for o in range(0, n, B))
    assert ct["dynamic"] + ct["fixed"] <= strips and ct["repairs"] == 0
    if n <= 3:                                                # 3 + 8 + 7 bits are three bytes: not smaller than the input
        assert ct == dict(ct, dynamic=0, fixed=0, stored=1)
    if n >= 258:                                              # every full strip, and a last strip of text long enough to pay its header
        assert ct["dynamic"] == sum(min(B, n - o) // dyn.STRIP + (min(B, n - o) % dyn.STRIP >= 258) for o in range(0, n, B))
    if n in (dyn.STRIP + 1, dyn.STRIP + 5):                   # a strip of 1 or 5 bytes behind a full one: the fixed code, BFINAL on it
        assert ct == dict(ct, dynamic=1, fixed=1, stored=0)
    if n in (B + 1, 3 * B + 7):                               # a block of 1 or 7 bytes of its own: stored (7 bytes of text are 3 + 7 * 8 + 7 bits in the fixed code)
        assert ct["stored"] == 1 and ct["fixed"] == 0
    if n >= dyn.STRIP - 1:
        assert len(z) < 0.8 * len(fixed)


def test_edge_alphabets_take_their_forks(workdir):
    cases = dyn.edge_alphabets()
    got = {}
    for name, data in cases.items():
        assert len(data) <= B
        z, ct, fixed = _check(workdir, data)
        got[name] = (len(z), ct)
        print("%s: %d -> dynamic mode %d bytes, fixed mode %d, %s" % (name, len(data), len(z), len(fixed), ct))
    one = dict(dynamic=1, fixed=0, stored=0, repairs=0, blocks=1)
    assert got["one_value"][1] == dict(one, nodist=0, onedist=1) and got["one_value"][0] < 100          # a literal, then lengths 258 and the rest at distance 1
    # five symbols with the end of the block: no worse than two bits for three values and three for the rarest (at most a quarter of the bytes) and the end,
    # 18435 bits, behind a header of at most 14 + 19 * 3 + 20 * 14 bits, in 26 bytes of BGZF
    assert got["four_values"][1] == dict(one, nodist=1, onedist=0) and got["four_values"][0] <= (3 + 351 + 18435 + 7) // 8 + 26
    assert got["all_256"][1] == dict(one, nodist=1, onedist=0)
    assert got["noise"][0] == B + 31 and got["noise"][1]["stored"] == 1
    # a strip of text saves more than the headers of seven strips of noise cost: the dynamic mode keeps this block coded (the fixed mode stores it)
    n, ct = got["text_then_noise"]
    assert ct["stored"] == 0 and ct["dynamic"] == 8 and n < B
    # coded first, stored in the end; _check's program saw nothing left behind the block
    n, ct = got["words_then_noise"]
    assert n == B + 31 and ct["stored"] == 1 and ct["dynamic"] + ct["fixed"] >= 1


def _optimal_cost(freq, limit):
    """the cost of an optimal code with lengths <= limit, by package-merge (Larmore and Hirschberg) in exact integers"""
    leaves = sorted((f, (i,)) for i, f in enumerate(freq) if f)
    n = len(leaves)
    if n == 1:
        return leaves[0][0]
    level = []
    for _ in range(limit):
        packages = [(level[2 * k][0] + level[2 * k + 1][0], level[2 * k][1] + level[2 * k + 1][1]) for k in range(len(level) // 2)]
        level = sorted(leaves + packages, key=lambda t: t[0])
    depth = Counter(i for _, ids in level[:2 * n - 2] for i in ids)
    assert sum(Fraction(1, 2 ** l) for l in depth.values()) == 1
    return sum(freq[i] * l for i, l in depth.items())


def _check_lengths(name, freq, limit, lens):
    used = [i for i, f in enumerate(freq) if f]
    assert len(lens) == len(freq) and max(lens) <= limit, name
    assert all((l > 0) == (f > 0) for l, f in zip(lens, freq)), name
    kraft = sum(Fraction(1, 2 ** l) for l in lens if l)
    assert kraft == 1 if len(used) >= 2 else kraft <= 1, (name, kraft)
    cost, best = sum(f * l for f, l in zip(freq, lens)), _optimal_cost(freq, limit)
    print("%s: limit %d, %d used symbols, the builder's cost %d, the optimal length-limited cost %d (%+.3f %%)" % (name, limit, len(used), cost, best, 100.0 * (cost - best) / best))
    assert cost >= best, (name, cost, best)                   # below the optimum: not a prefix code
    return cost, best


def test_length_builder_against_package_merge(workdir):
    repaired = {}
    for name, limit, freq in dyn.histograms():
        lens, rep = dyn.host_lengths(workdir, freq, limit)
        cost, best = _check_lengths(name, freq, limit, lens)
        repaired[name] = rep
        if not rep:                                           # no length was cut: the code is Huffman's, and optimal
            assert cost == best, name
    # a Fibonacci histogram of k symbols makes a tree of depth k - 1
    assert repaired == dict(fib17=1, fib20=1, fib30=1, fib9=1, fib19=1, fib30_spread=1, one=0, two=0, equal286=0, eob_only=0), repaired
    assert dyn.host_lengths(workdir, dyn.fibonacci(16), 15) == ([15, 15] + list(range(14, 0, -1)), 0)      # depth 15: nothing to cut
    # histograms the cases above do not hold: random ones of every shape, at both limits
    rng = np.random.default_rng(8)
    for k in range(40):
        n_sym = int(rng.integers(2, 287)) if k % 2 else int(rng.integers(2, 20))
        limit = 15 if k % 2 else 7
        freq = (rng.integers(0, 3, n_sym) * rng.integers(1, 1 << int(rng.integers(1, 20)), n_sym)).tolist()
        if not any(freq):
            freq[0] = 1
        lens, _ = dyn.host_lengths(workdir, freq, limit)
        _check_lengths("random%d" % k, freq, limit, lens)


@pytest.mark.parametrize("base", dyn.GOLDEN_SETS)
def test_golden_record_sets_are_smaller_than_in_the_fixed_mode(base, workdir):
    rec = dyn.golden_records(workdir, base)
    z, ct, fixed = _check(workdir, rec)
    print("%s: %d bytes of records, fixed mode %d, dynamic mode %d (%.3f of the fixed mode's), %s" % (base, len(rec), len(fixed), len(z), len(z) / len(fixed), ct))
    assert len(z) < len(fixed)
    assert ct["dynamic"] > 0 and ct["stored"] == 0


def test_lane_functions_under_the_sanitizers(workdir):
    """the same program built with AddressSanitizer and UBSan for its host side, run stand-alone"""
    data = dyn.text(70000)
    z, ct = dyn.host_deflate_dyn(workdir, data, sanitize=True)
    assert z == dyn.host_deflate_dyn(workdir, data)[0] and ct["dynamic"] >= 8
    for name, limit, freq in dyn.histograms():
        if name.startswith("fib"):
            assert dyn.host_lengths(workdir, freq, limit, sanitize=True) == dyn.host_lengths(workdir, freq, limit)
