"""Helpers of the UMI-aware duplicate-marking tests: the sequential Python twin of the definition of dg_bam_markdup_umi_finish in include/dartgpu.h (dictionaries
keyed by family and by UMI -- record by record, not as the kernels' sorts), a second, independent verdict (brute force: roots by recursion over the definition's
sentences on decoded letters, verdicts by loops over all pairs of pairs and of fragments), hand-made records that each hold what they are named for, and the
native program tests/native/umidup_checks.hip.  What a record is, which records pair up and which are fragments is markdup_inputs' (the plain marking's twin)."""
from __future__ import annotations

import os, struct, subprocess
import common
import bamsort_inputs as bsi
import markdup_inputs as mdi
from bamidx_inputs import offsets, M

HASH_BITS = mdi.HASH_BITS
FAMILY = 64
MAX_LEN = 21
LETTERS = b"ACGTN+-"
STATS = mdi.STATS[:7] + ("largest_cluster", "records_with_umi", "pair_families_of_several_groups", "absorbed_groups", "crowded_families")


def umi_of(name: bytes, sep: bytes = b"_") -> int:
    k = name.rfind(sep)
    if k < 0:
        return 0
    suffix = name[k + 1:]
    if not 1 <= len(suffix) <= MAX_LEN or any(b not in LETTERS for b in suffix):
        return 0
    u = 0
    for b in suffix:
        u = u * 8 + LETTERS.index(b) + 1
    return u


def letters_of(u: int) -> bytes:
    out = b""
    while u:
        out = LETTERS[(u & 7) - 1:(u & 7)] + out
        u >>= 3
    return out


def n_letters(u: int) -> int:
    n = 0
    while u:
        n, u = n + 1, u >> 3
    return n


def joins(ur, cr, ug, cg) -> bool:
    if not ur or not ug or n_letters(ur) != n_letters(ug) or cr < 2 * cg - 1:
        return False
    x, d = ur ^ ug, 0
    while x:
        d, x = d + (1 if x & 7 else 0), x >> 3
    return d <= 1


def cluster(counts: dict, max_edit: int):
    """counts = {U: count} of one family -> ({U: root U}, absorbed groups, crowded)"""
    if len(counts) > FAMILY:
        return {u: u for u in counts}, 0, True
    root = {}
    if max_edit:
        for g in sorted(counts, key=lambda u: (-counts[u], u)):
            root[g] = next((r for r in root if root[r] == r and joins(r, counts[r], g, counts[g])), g)       # (a dict keeps the order of the walk)
    else:
        root = {u: u for u in counts}
    return root, sum(1 for u in root if root[u] != u), False


def _examined(raw, n_chr, sep):
    offs = offsets(raw)
    recs = {}
    for i, at in enumerate(offs):
        r = mdi.examine(raw, at, n_chr, i)
        if r is not None:
            r["U"] = umi_of(r["name"], sep)
            recs[i] = r
    return offs, recs


def twin(raw: bytes, n_chr: int, max_edit: int = 0, sep: bytes = b"_", hash_bits: int = HASH_BITS):
    """-> (the marked array's bytes, the twelve stats, {index: verdict} of the examined records); raises mdi.RangeError"""
    offs, recs = _examined(raw, n_chr, sep)
    pairs, frags, crowded_cand = mdi.classify(recs, hash_bits)
    E = lambda i: recs[i]["E"]
    verdict, absorbed, crowded, multi, largest = {}, 0, 0, 0, 0
    fams = {}
    for a, b in pairs:
        fams.setdefault((min(E(a), E(b)), max(E(a), E(b))), {}).setdefault(recs[a]["U"], []).append((a, b))
    for groups in fams.values():
        root, ab, cr = cluster({u: len(p) for u, p in groups.items()}, max_edit)
        absorbed += ab; crowded += cr; multi += len(groups) > 1
        clusters = {}
        for u, p in groups.items():
            clusters.setdefault(root[u], []).extend(p)
        for members in clusters.values():
            largest = max(largest, len(members))
            best = min(members, key=lambda p: (-(recs[p[0]]["score"] + recs[p[1]]["score"]), p[0]))
            for p in members:
                verdict[p[0]] = verdict[p[1]] = p != best
    efams = {}
    for a, b in pairs:
        for i in (a, b):
            efams.setdefault(E(i), {}).setdefault(recs[i]["U"], []).append(("pair end", i))
    for i in frags:
        efams.setdefault(E(i), {}).setdefault(recs[i]["U"], []).append(("fragment", i))
    for groups in efams.values():
        root, ab, cr = cluster({u: len(e) for u, e in groups.items()}, max_edit)
        absorbed += ab; crowded += cr
        clusters = {}
        for u, e in groups.items():
            clusters.setdefault(root[u], []).extend(e)
        for members in clusters.values():
            has_pair = any(kind == "pair end" for kind, _ in members)
            fr = [i for kind, i in members if kind == "fragment"]
            best = min(fr, key=lambda i: (-recs[i]["score"], i), default=None)
            for i in fr:
                verdict[i] = has_pair or i != best
    out = bytearray(raw)
    for i, dup in verdict.items():
        out[offs[i] + 19] = out[offs[i] + 19] | 4 if dup else out[offs[i] + 19] & ~4
    dp = sum(1 for a, _ in pairs if verdict[a]); df = sum(1 for i in frags if verdict[i])
    stats = (len(recs), len(pairs), len(frags), dp, df, crowded_cand, 2 * dp + df, largest, sum(1 for r in recs.values() if r["U"]), multi, absorbed, crowded)
    return bytes(out), stats, verdict


def brute(raw: bytes, n_chr: int, max_edit: int = 0, sep: bytes = b"_", hash_bits: int = HASH_BITS):
    """the independent verdict, straight from the sentences, on letters instead of codes and without any ordering of the groups -> {index: verdict}"""
    _, recs = _examined(raw, n_chr, sep)
    pairs, frags, _ = mdi.classify(recs, hash_bits)
    text = {i: letters_of(r["U"]) for i, r in recs.items()}

    def near(a: bytes, b: bytes):
        return bool(a) and bool(b) and len(a) == len(b) and sum(x != y for x, y in zip(a, b)) <= 1

    def roots(members):
        """members = the UMI text of every pair / end of one family, with repeats -> {text: its root's text}"""
        cnt = {}
        for t in members:
            cnt[t] = cnt.get(t, 0) + 1
        if not max_edit or len(cnt) > FAMILY:
            return {t: t for t in cnt}
        code = lambda t: [LETTERS.index(b) + 1 for b in t]
        earlier = lambda a, b: cnt[a] > cnt[b] or (cnt[a] == cnt[b] and (len(a), code(a)) < (len(b), code(b)))      # U ascending: shorter first, then the codes
        memo = {}

        def root(g):
            if g not in memo:
                takers = [r for r in cnt if earlier(r, g) and root(r) == r and near(r, g) and cnt[r] >= 2 * cnt[g] - 1]
                memo[g] = next((r for r in takers if not any(earlier(x, r) for x in takers)), g)
            return memo[g]
        return {t: root(t) for t in cnt}

    sig = lambda a, b: (min(recs[a]["E"], recs[b]["E"]), max(recs[a]["E"], recs[b]["E"]))
    verdict = {}
    pair_roots = {}
    for a, b in pairs:
        if sig(a, b) not in pair_roots:
            pair_roots[sig(a, b)] = roots([text[x] for x, y in pairs if sig(x, y) == sig(a, b)])
    P = [(sig(a, b), pair_roots[sig(a, b)][text[a]], recs[a]["score"] + recs[b]["score"], a, b) for a, b in pairs]
    for s, r, sc, a, b in P:
        verdict[a] = verdict[b] = any(s2 == s and r2 == r and (sc2 > sc or (sc2 == sc and a2 < a)) for s2, r2, sc2, a2, _ in P)
    ends = [(recs[i]["E"], i, True) for p in pairs for i in p] + [(recs[i]["E"], i, False) for i in frags]
    end_roots = {}
    for e, _, _ in ends:
        if e not in end_roots:
            end_roots[e] = roots([text[i] for e2, i, _ in ends if e2 == e])
    for i in frags:
        e, sc, r = recs[i]["E"], recs[i]["score"], end_roots[recs[i]["E"]][text[i]]
        verdict[i] = any(e2 == e and end_roots[e][text[j]] == r and j != i and (paired or recs[j]["score"] > sc or (recs[j]["score"] == sc and j < i)) for e2, j, paired in ends)
    return verdict


# ---- the crafted cases ----
def rename(rec: bytes, name: bytes) -> bytes:
    """the record under another name"""
    body = rec[4:36] + name + b"\0" + rec[36 + rec[12]:]
    out = bytearray(struct.pack("<i", len(body) - 0) + body)
    out[12] = len(name) + 1
    struct.pack_into("<i", out, 0, len(out) - 4)
    return bytes(out)


def with_umis(rng, recs, values, bare=0.1, sep=b"_"):
    """every name gains sep and one of `values` (mates share it); a share `bare` of the names stays as it is"""
    chosen = {}
    out = []
    for r in recs:
        nm = r[36:36 + r[12] - 1]
        if nm not in chosen:
            chosen[nm] = None if rng.random() < bare else rng.choice(values)
        out.append(r if chosen[nm] is None else rename(r, nm + sep + chosen[nm]))
    return out


def umi_values(rng, n=30, length=6):
    """n UMIs in neighbourhoods: a third drawn at random, the rest one letter away from one of those"""
    base = [bytes(rng.choice(b"ACGT") for _ in range(length)) for _ in range(n // 3)]
    out = list(base)
    while len(out) < n:
        b = bytearray(rng.choice(base)); k = rng.randrange(length)
        b[k] = rng.choice([x for x in b"ACGTN" if x != b[k]])
        if bytes(b) not in out:
            out.append(bytes(b))
    return out


def random_records(rng, n, n_chr, distinct_scores=False):
    return with_umis(rng, mdi.random_records(rng, n, n_chr, distinct_scores), umi_values(rng))


def doubled(k: int) -> bytes:
    """six letters, the three base-4 digits of k twice each: two different k are two letters apart or more"""
    return b"".join(b"ACGT"[k >> s & 3:(k >> s & 3) + 1] * 2 for s in (4, 2, 0))


def crafted_cases():
    """name -> (n_chr, records in coordinate order)"""
    serial = [0]

    def pairs(umi, count, pos=1000, q=60, tid=0, stem=b"p"):
        out = []
        for _ in range(count):
            serial[0] += 1
            out += mdi.pair(stem + b"%d" % serial[0] + (b"_" + umi if umi is not None else b""), tid, pos, 0, tid, pos + 200, 1, q1=q)
        return out

    frag = lambda pos, name, score=100, flag=0: mdi.mrec(0, pos, flag, name, [(50, M)], mdi.quals_of(score))
    suffix = [frag(100, b"nosep"), frag(100, b"empty_", 101), frag(100, b"u21_" + b"ACGTN+-" * 3, 102), frag(100, b"u22_" + b"ACGTN+-" * 3 + b"A", 103), frag(100, b"lower_acgt", 104),
              frag(100, b"pm_A+-", 105), frag(100, b"in_side_ACG", 106), frag(100, b"x_AC_GT", 107), frag(100, b"digit_AC1T", 108), frag(100, b"_T", 109), frag(100, b"one_N", 110)]
    family = lambda k: pairs(doubled(0), 3, q=70) + [r for j in range(1, k - 1) for r in pairs(doubled(j), 1)] + pairs(b"AAAAAN", 1)
    cases = {
        "suffix": suffix,
        "different_umis": pairs(b"AAAAAA", 1) + pairs(b"CCCCCC", 1) + pairs(b"GGGGGG", 1),
        "same_umi": pairs(b"ACGTAC", 1, q=61) + pairs(b"ACGTAC", 1, q=90) + pairs(b"ACGTAC", 1),
        "join_3_1": pairs(b"ACGTAC", 3) + pairs(b"ACGTAA", 1, q=99),
        "apart_2_2": pairs(b"ACGTAC", 2) + pairs(b"ACGTAA", 2),
        "distance_2": pairs(b"ACGTAC", 3) + pairs(b"ACGTTT", 1),
        "lengths": pairs(b"ACGTAC", 3) + pairs(b"ACGTA", 1) + pairs(b"ACGTACA", 1),
        "zero_never_joins": pairs(None, 3) + pairs(b"A", 1) + pairs(b"bad", 1),
        "one_hop_chain": pairs(b"ACGTAC", 10) + pairs(b"ACGTAA", 4) + pairs(b"ACGTTA", 1),
        "count_ties": pairs(b"AAAAAA", 1, q=60) + pairs(b"AAAAAC", 1, q=90) + pairs(b"AAAACC", 1, q=70),
        "fragment_and_pair_end": pairs(b"AAAAAA", 1, pos=1000) + [frag(1000, b"f_same_AAAAAA", 5000), frag(1000, b"f_other_CCCCCC", 90), frag(1000, b"f_other_worse_CCCCCC", 80),
                                                                  frag(1000, b"f_near_AAAAAC", 70)],
        "family_of_64": family(64), "family_of_65": family(65),
        "empty": [],
    }
    return {k: (2, sorted(v, key=lambda r: bsi.key(r, 2))) for k, v in cases.items()}


def names_of(recs):
    return [r[36:36 + r[12] - 1] for r in recs]


# ---- the native program ----
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "umidup_checks_san" if sanitize else "umidup_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "umidup_checks.hip")])
    return exe


def run_program(exe, workdir, tag, n_chr, raw, max_edit=0, sep=b"_", hash_bits=HASH_BITS):
    """-> dict(recs = [(examined, candidate, E, score, h, U)], bad = index of the first record out of range or None, dup = {index: verdict}, stats = the twelve,
    marked = the bytes)"""
    src = os.path.join(workdir, "ud_%s.in" % tag); txt = os.path.join(workdir, "ud_%s.txt" % tag); out = os.path.join(workdir, "ud_%s.bin" % tag)
    with open(src, "wb") as f:
        f.write(struct.pack("<5q", n_chr, hash_bits, len(raw), max_edit, sep[0]) + raw)
    r = subprocess.run([exe, src, txt, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    res = dict(recs=[], bad=None, dup={}, stats=None, marked=open(out, "rb").read())
    for line in open(txt).read().splitlines():
        w = line.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "rec":
            res["recs"].append(tuple(v[1:]))
        elif w[0] == "bad":
            res["bad"] = v[0]
        elif w[0] == "dup":
            res["dup"][v[0]] = bool(v[1])
        elif w[0] == "stats":
            res["stats"] = tuple(v)
    return res
