"""Helpers of the inline-UMI tests: the sequential twin of the definition of dg_set_umi in include/dartgpu.h on top of the trimming twin (tests/trim_inputs.py:
the cut comes first, then the four steps on the remainder), reads on the rule's seams, and the driver of tests/native/umi_extract_checks.hip."""
from __future__ import annotations

import os, struct, subprocess
import numpy as np
import common
import fastq_device_inputs as fdi
import trim_inputs as ti

UMI_PAIRS = 1
STAT_KEYS = ti.STAT_KEYS[:14] + ["umi_bases", "umi_dropped_reads"]


def umi(len1=0, len2=0, skip1=0, skip2=0, sep=b"_", flags=0):
    return dict(len=(len1, len2), skip=(skip1, skip2), sep=sep, flags=flags)


def slot_of(k, f, two, u):
    return f if two else ((k & 1) if u["flags"] & UMI_PAIRS else 0)


def letters(s: bytes, n: int) -> bytes:
    return bytes(ti._up(c) if ti._up(c) in b"ACGT" else ord("N") for c in s[:n])


BLANK = dict(cut5=0, cut3=0, adapter=False, ad_cut=0, poly=False, poly_cut=0, qskip=False)


def batch(recs, p, u, two: bool, rc_odd: bool):
    """trim_inputs.trim_batch with the UMI rule u (None: off) in front -> (kept [(name, stored read, stored quality)], stats [16], kept indices)"""
    pairs = bool(p["flags"] & ti.PAIRS)
    n = len(recs)
    cut, fail, wins = [], [], []
    for k, (h, s, q, f) in enumerate(recs):
        m = slot_of(k, f, two, u) if u else 0
        c = u["len"][m] + u["skip"][m] if u else 0
        ad = f if two else ((k & 1) if pairs else 0)
        bad = len(s) < c + 1
        cut.append(c); fail.append(bad)
        wins.append(((0, 0, BLANK) if bad else ti.window(s[c:], q[c:], p, p["adapter"][ad])) + (ad, m))
    own = [not fail[k] and wins[k][1] - wins[k][0] >= p["min_len"] for k in range(n)]
    st = [0] * 16
    kept, idx = [], []
    for k, (h, s, q, f) in enumerate(recs):
        a, b, w, ad, m = wins[k]
        partnered = bool(u) and (two or bool(u["flags"] & UMI_PAIRS)) and (k ^ 1) < n
        drop = fail[k] or (partnered and fail[k ^ 1])
        mate = own[k ^ 1] if pairs and (k ^ 1) < n else True
        keep = own[k] and mate and not drop
        st[0] += 1; st[2] += len(s); st[4] += w["cut5"]; st[5] += w["cut3"]
        if w["adapter"]:
            st[6 + ad] += 1; st[8] += w["ad_cut"]
        if w["poly"]:
            st[9] += 1; st[10] += w["poly_cut"]
        st[11] += not drop and not own[k]; st[12] += not drop and own[k] and not mate; st[13] += w["qskip"]
        if u:
            st[14] += 0 if fail[k] else cut[k]; st[15] += drop
        if keep:
            c = cut[k]
            st[1] += 1; st[3] += b - a
            ts, tq = s[c + a:c + b], q[c + a:min(c + b, len(q))] if c + a < len(q) else b""
            if u:
                e = k & ~1
                h = h + u["sep"] + (letters(recs[e][1], u["len"][wins[e][4]]) + letters(recs[e + 1][1], u["len"][wins[e + 1][4]]) if partnered else letters(s, u["len"][m]))
            idx.append(k)
            if rc_odd and (k & 1):
                ts, tq = fdi.get_complementary_seq(ts), tq[::-1]
            kept.append((h, ts, tq))
    return kept, st, idx


def seam_reads(u_cut: int, seed=3, n_fill=40, drop_at=()):
    """[(label, read, quality)]: reads of u - 1, u and u + 1 bases, remainders of 63, 64 and 65 bases, N and lower case inside the first bases, a quality shorter
    than the read, then n_fill reads of 30..90 bases of which those at drop_at are u bases long (they fail the rule)"""
    rng = np.random.default_rng(seed)
    rnd = lambda n: ti._rand(rng, n, b"ACGT")
    out = []
    for L in (max(u_cut - 1, 1), max(u_cut, 1), u_cut + 1, u_cut + 63, u_cut + 64, u_cut + 65):
        out.append(("len%d" % L, rnd(L), b"I" * L))
    out.append(("n_and_lower", b"aNcgtRn." + rnd(50), b"I" * 58))
    out.append(("ql_short", rnd(60), b"I" * 40))
    for k in range(n_fill):
        L = max(u_cut, 1) if k in drop_at else int(rng.integers(30, 91))
        s = rnd(L)
        if k % 3 == 0 and L > 40:
            s = s[:L - 12] + ti.ADAPTER[:12]
        out.append(("m%d" % k, s, bytes(int(x) for x in rng.integers(35, 74, L))))
    return out


# ---- the native program ----
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "umi_extract_checks_san" if sanitize else "umi_extract_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w", "-I", os.path.join(common.ROOT, "include")] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "umi_extract_checks.hip")])
    return exe


def run_program(exe, workdir, tag, recs, u, two, n_min_len=1):
    """the rules of the cut over the reads (in file orientation) -> per read (slot, cut, fails, dropped, partnered, suffix bytes)"""
    src = os.path.join(workdir, "ux_%s.in" % tag)
    with open(src, "wb") as f:
        f.write(struct.pack("<8q", len(recs), 1 if two else 0, u["flags"], u["len"][0], u["len"][1], u["skip"][0], u["skip"][1], u["sep"][0]))
        for h, s, q, fl in recs:
            f.write(struct.pack("<2q", fl, len(s)) + s)
    r = subprocess.run([exe, src], capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        w = line.split(b" ")
        out.append((int(w[0]), int(w[1]), int(w[2]), int(w[3]), int(w[4]), w[5] if len(w) > 5 else b""))
    return out
