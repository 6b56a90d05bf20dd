"""Helpers of the device junction table's tests: the input file tests/native/sj_checks.hip reads, the synthetic keys both suites use, and the expected
entries and text from the Python twin (dart_amd/sam.py::junction_twin)."""
from __future__ import annotations

import os, subprocess
import numpy as np
import common
from dart_amd import host, sam

INT_MAX = (1 << 31) - 1


def entries_of(tuples) -> np.ndarray:
    """(g1, g2) or (g1, g2, count) rows -> SJ_ENTRY array"""
    rows = list(tuples)
    a = np.zeros(len(rows), host.SJ_ENTRY)
    for k, t in enumerate(rows):
        a[k]["g1"], a[k]["g2"], a[k]["count"] = int(t[0]), int(t[1]), int(t[2]) if len(t) > 2 else 1
    return a


def twin(tuples, ix: host.Index):
    """-> (SJ_ENTRY array, text bytes, lines) of sam.junction_twin"""
    ent, text, lines = sam.junction_twin(tuples, ix.names, ix.chr_off, ix.chr_len, ix.l_pac)
    a = np.zeros(len(ent), host.SJ_ENTRY)
    for k, (g1, g2, cnt, c) in enumerate(ent):
        a[k]["g1"], a[k]["g2"], a[k]["count"], a[k]["chr"] = g1, g2, cnt, c
    return a, text, lines


def boundary_keys(ix: host.Index):
    n = len(ix.names)
    return [int(ix.chr_off[i]) + int(ix.chr_len[i]) - 1 for i in range(n)] + [2 * int(ix.l_pac) - int(ix.chr_off[i]) - 1 for i in reversed(range(n))]


def synthetic_keys(ix: host.Index):
    """(g1, g2, count) rows the mapper would never emit: g1 exactly on a boundary key, one past it, on the last key and one past the last key (no line),
    g1 = -1, g1 in the mirrored half [l_pac, 2 l_pac), keys above 2^33, counts and positions at every decimal width change up to 2^31 - 1"""
    keys = boundary_keys(ix)
    L = int(ix.l_pac)
    rows = []
    for k in keys[:3] + keys[-2:]:
        rows += [(k, k + 7, 3), (k + 1, k + 9, 2)]          # on a boundary key and one past it (the last: past every key, no line)
    rows += [(-1, 5, 4), (-1, -1, 1), (L, L + 10, 1), (2 * L - 1, 2 * L - 1, 6), (L + 17, 3, 2)]
    rows += [((1 << 33) + 5, (1 << 33) + 900, 1), ((1 << 33) + 5, (1 << 40) + 1, 2), ((1 << 62), -(1 << 62), 1), (-(1 << 62), (1 << 62), 5)]
    w = 10
    while w <= INT_MAX:
        for c in (w - 1, w):
            rows.append((7, 1000 + len(rows), c))              # the count at the width change (9 / 10, 99 / 100, ...)
            rows.append((3, c - 1, 1))                         # g2's position printed as c
            rows.append((c - 1, 5, 1))                         # g1's position printed as c (while it lies on a chromosome)
        w *= 10
    rows.append((1, 2, INT_MAX))
    rows.append((2, INT_MAX - 1, 1))
    # (two rows with one key add up: the twin sums them too)
    rows.append((keys[0], keys[0] + 7, 5))
    return rows


def write_input(path, tuples, ix: host.Index, slots: int):
    ent = entries_of(tuples)
    no, nb = host.flatten_strings(ix.names)
    nb = nb[:int(no[-1])]                                      # (without the terminating NUL flatten_strings appends)
    head = np.asarray([len(ent), len(ix.names), int(ix.l_pac), int(slots)], np.int64)
    with open(path, "wb") as f:
        for a in (head, np.ascontiguousarray(ix.chr_off, np.int64), np.ascontiguousarray(ix.chr_len, np.int64), np.ascontiguousarray(no, np.uint32), nb, ent):
            raw = a.tobytes()
            f.write(raw + b"\0" * (-len(raw) % 8))


def build_lane_program(workdir):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "sj_checks")
    if not os.path.exists(exe):
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w", "-o", exe, os.path.join(common.ROOT, "tests", "native", "sj_checks.hip")])
    return exe


def run_lane_program(exe, in_path):
    """-> (SJ_ENTRY array, text bytes, lines, growths)"""
    out = in_path + ".out"
    r = subprocess.run([exe, in_path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    ne, nl, nb, grown = (int(x) for x in np.frombuffer(raw, np.uint64, 4))
    ent = np.frombuffer(raw, host.SJ_ENTRY, ne, 32).copy()
    text = raw[32 + 24 * ne:]
    assert len(text) == nb
    return ent, text, nl, grown
