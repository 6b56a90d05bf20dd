"""Helpers of the duplicate-marking tests: the sequential Python twin of the definition in dart_amd/csrc/dg_markdup.h (dictionaries keyed by hash, by name, by
signature and by end key -- record by record, not as the kernels' sorts), a second, independent verdict (brute force over all pairs of pairs and of fragments,
written from the definition's sentences), hand-made records that each hold what they are named for, and the native program tests/native/markdup_checks.hip.
The definition is the header's comment: no samtools or Picard exists where these tests run."""
from __future__ import annotations

import os, struct, subprocess
import common
import bamsort_inputs as bsi
from bamidx_inputs import offsets, M, I, D, N, S, H, P, EQ, X

HASH_BITS = 48
CROWD = 64
SCORE_MAX = (1 << 20) - 1
DUP = 0x400
STATS = ("examined", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "crowded_candidates", "flagged_records", "largest_family")


class RangeError(Exception):
    """an examined record's unclipped 5' end does not fit the end key (args[0] = its index)"""


def mrec(refid, pos, flag, name, cigar=(), quals=b"", mapq=30, tags=b""):
    """one uncompressed BAM record with its block_size: cigar = [(len, op)], quals = the quality bytes (l_seq of them)"""
    quals = bytes(quals)
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(name) + 1, mapq, 4680, len(cigar), flag, len(quals), -1, -1, 0)
    body += name + b"\0" + b"".join(struct.pack("<I", l << 4 | op) for l, op in cigar) + bytes((len(quals) + 1) // 2) + quals + tags
    return struct.pack("<i", len(body)) + body


def quals_of(total: int) -> bytes:
    """quality bytes whose score is `total` (>= 50)"""
    n, rem = divmod(total, 50)
    q = [50] * n
    if rem >= 15:
        q.append(rem)
    elif rem:
        q[0] += rem
    return bytes(q)


def name_hash(name: bytes, hash_bits: int = HASH_BITS) -> int:
    h = 0xcbf29ce484222325
    for b in name:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return (h ^ h >> 48) & ((1 << hash_bits) - 1)


def examine(raw: bytes, at: int, n_chr: int, index: int):
    """-> dict(E, score, cand, name, flag) of an examined record, else None; raises RangeError(index)"""
    avail = len(raw) - at
    if avail < 36:
        return None
    bs, refid, pos = struct.unpack_from("<Iii", raw, at)
    l_name = raw[at + 12]
    n_cig, flag = struct.unpack_from("<HH", raw, at + 16)
    l_seq = struct.unpack_from("<I", raw, at + 20)[0]
    if not (0 <= refid < n_chr and pos >= 0 and not flag & 4 and not flag & 0x900 and n_cig > 0):
        return None
    qual_at = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
    if qual_at + l_seq > min(4 + bs, avail):
        return None
    s = flag >> 4 & 1
    rlen = lead = trail = 0
    seen = False
    for c in struct.unpack_from("<%dI" % n_cig, raw, at + 36 + l_name):
        op, ln = c & 15, c >> 4
        if op in (S, H):
            if seen:
                trail += ln
            else:
                lead += ln
        else:
            seen, trail = True, 0
            if op in (M, D, N, EQ, X):
                rlen += ln
    u5 = pos + rlen - 1 + trail if s else pos - lead
    if not 0 <= u5 + (1 << 31) < 1 << 33:
        raise RangeError(index)
    score = min(sum(q for q in raw[at + qual_at:at + qual_at + l_seq] if 15 <= q <= 93), SCORE_MAX)
    cand = bool(flag & 1) and not flag & 8 and bool(flag & 0x40) != bool(flag & 0x80)
    return dict(E=refid << 34 | (u5 + (1 << 31)) << 1 | s, score=score, cand=cand, name=raw[at + 36:at + 36 + max(l_name - 1, 0)], flag=flag)


def classify(recs, hash_bits):
    """recs = {index: examined dict} -> (pairs [(rep, other)], fragments [index], candidates in crowded runs)"""
    runs = {}
    for i in sorted(recs):
        if recs[i]["cand"]:
            runs.setdefault(name_hash(recs[i]["name"], hash_bits), []).append(i)
    pairs, paired, crowded = [], set(), 0
    for members in runs.values():
        if len(members) > CROWD:
            crowded += len(members)
            continue
        groups = {}
        for i in members:
            groups.setdefault(recs[i]["name"], []).append(i)
        for g in groups.values():
            if len(g) == 2 and {recs[g[0]]["flag"] & 0xC0, recs[g[1]]["flag"] & 0xC0} == {0x40, 0x80}:
                pairs.append((min(g), max(g))); paired.update(g)
    return sorted(pairs), [i for i in sorted(recs) if i not in paired], crowded


def twin(raw: bytes, n_chr: int, hash_bits: int = HASH_BITS):
    """-> (the marked array's bytes, the eight stats, {index: verdict} of the examined records); raises RangeError(index of the first record out of range)"""
    offs = offsets(raw)
    recs = {}
    for i, at in enumerate(offs):
        r = examine(raw, at, n_chr, i)
        if r is not None:
            recs[i] = r
    pairs, frags, crowded = classify(recs, hash_bits)
    best, family = {}, {}
    sig = lambda a, b: (min(recs[a]["E"], recs[b]["E"]), max(recs[a]["E"], recs[b]["E"]))
    rank = lambda a, b: (-(recs[a]["score"] + recs[b]["score"]), a)
    for a, b in pairs:
        k = sig(a, b)
        family[k] = family.get(k, 0) + 1
        if k not in best or rank(a, b) < rank(*best[k]):
            best[k] = (a, b)
    verdict = {}
    for a, b in pairs:
        verdict[a] = verdict[b] = best[sig(a, b)] != (a, b)
    pair_ends = {e for k in best for e in k}
    best_frag = {}
    for i in frags:
        e = recs[i]["E"]
        if e not in best_frag or (-recs[i]["score"], i) < (-recs[best_frag[e]]["score"], best_frag[e]):
            best_frag[e] = i
    for i in frags:
        verdict[i] = recs[i]["E"] in pair_ends or best_frag[recs[i]["E"]] != i
    out = bytearray(raw)
    for i, dup in verdict.items():
        out[offs[i] + 19] = out[offs[i] + 19] | 4 if dup else out[offs[i] + 19] & ~4
    dp = sum(1 for a, _ in pairs if verdict[a]); df = sum(1 for i in frags if verdict[i])
    return bytes(out), (len(recs), len(pairs), len(frags), dp, df, crowded, 2 * dp + df, max(family.values(), default=0)), verdict


def brute(raw: bytes, n_chr: int, hash_bits: int = HASH_BITS):
    """the independent verdict, straight from the sentences: a pair is a duplicate iff a better pair has its signature; a fragment is a duplicate iff a pair has
    its end, or a better fragment has it.  Its own grouping too: loops, no dictionary -> {index: verdict}"""
    offs = offsets(raw)
    recs = [examine(raw, at, n_chr, i) for i, at in enumerate(offs)]
    cands = [i for i, r in enumerate(recs) if r and r["cand"]]
    hashes = {i: name_hash(recs[i]["name"], hash_bits) for i in cands}
    partner = {}
    for i in cands:
        run = [j for j in cands if hashes[j] == hashes[i]]
        if len(run) > CROWD:
            continue
        same = [j for j in run if j != i and recs[j]["name"] == recs[i]["name"]]
        if len(same) == 1 and (recs[i]["flag"] ^ recs[same[0]]["flag"]) & 0xC0 == 0xC0:
            partner[i] = same[0]
    pairs = [(i, j) for i, j in partner.items() if i < j]
    frags = [i for i, r in enumerate(recs) if r and i not in partner]
    P = [(min(recs[a]["E"], recs[b]["E"]), max(recs[a]["E"], recs[b]["E"]), recs[a]["score"] + recs[b]["score"], a, b) for a, b in pairs]
    verdict = {}
    for lo, hi, sc, a, b in P:
        verdict[a] = verdict[b] = any((l2, h2) == (lo, hi) and (s2 > sc or (s2 == sc and a2 < a)) for l2, h2, s2, a2, _ in P)
    for i in frags:
        e, sc = recs[i]["E"], recs[i]["score"]
        verdict[i] = any(e in (lo, hi) for lo, hi, _, _, _ in P) or any(j != i and recs[j]["E"] == e and (recs[j]["score"] > sc or (recs[j]["score"] == sc and j < i)) for j in frags)
    return verdict


def flags_by_name(raw: bytes):
    """{(name, flag)} of the array's records"""
    return {(raw[at + 36:at + 36 + raw[at + 12] - 1], struct.unpack_from("<H", raw, at + 18)[0]) for at in offsets(raw)}


def collide(hash_bits: int, bucket: int, prefix: bytes, count: int):
    """`count` different names whose hash of `hash_bits` bits is `bucket`"""
    out, k = [], 0
    while len(out) < count:
        nm = prefix + b"%d" % k
        if name_hash(nm, hash_bits) == bucket:
            out.append(nm)
        k += 1
    return out


# ---- the crafted cases ----
ALL_OPS = [(5, S), (10, M), (2, I), (3, D), (700, N), (4, EQ), (1, X), (6, P), (7, H)]         # rlen 718; lead 5, trail 7
FAR = [((1 << 28) - 1, N)]


def pair(name, tid1, pos1, rev1, tid2, pos2, rev2, q1=60, q2=60, cig1=None, cig2=None, extra1=0, extra2=0):
    """a proper pair: mate 1 and mate 2 under one name"""
    f1 = 0x41 | (16 if rev1 else 0) | (32 if rev2 else 0) | extra1; f2 = 0x81 | (16 if rev2 else 0) | (32 if rev1 else 0) | extra2
    return [mrec(tid1, pos1, f1, name, cig1 or [(50, M)], quals_of(q1)), mrec(tid2, pos2, f2, name, cig2 or [(50, M)], quals_of(q2))]


def liars():
    """block_size holds one op and ten bases; the counts say otherwise: such a record is not examined (dg_bam_sort_add refuses it: only the lane code's tests see it)"""
    a = bytearray(mrec(0, 50, 0, b"liar_cigar", [(10, M)], quals_of(500))); struct.pack_into("<H", a, 16, 60000)
    b = bytearray(mrec(0, 60, 0, b"liar_seq", [(10, M)], quals_of(500))); struct.pack_into("<I", b, 20, 0xFFFFFFF0)
    c = bytearray(mrec(0, 70, 0, b"liar_seq_by_one", [(10, M)], quals_of(500))); struct.pack_into("<I", c, 20, 11)
    return [bytes(a), bytes(b), bytes(c)]


def crafted_cases():
    """name -> (n_chr, records in coordinate order, hash_bits, fits the store: dg_bam_sort_add takes every record)"""
    frag = lambda tid, pos, flag, name, cigar, score=100: mrec(tid, pos, flag, name, cigar, quals_of(score))
    cigar = [
        frag(0, 1000, 0, b"all_ops_fwd", ALL_OPS, 300), frag(0, 995, 0, b"same_u5_no_clip", [(30, M)], 200),             # u5 = 995 both
        frag(0, 1000, 16, b"all_ops_rev", ALL_OPS, 300), frag(0, 1700, 16, b"same_end_no_clip", [(25, M)], 400),            # u5 = 1000 + 718 - 1 + 7 = 1724 both
        frag(0, 2000, 0, b"h_then_s", [(3, H), (4, S), (20, M), (2, S), (1, H)], 100), frag(0, 1993, 0, b"plain_1993", [(20, M)], 90),
        frag(0, 2000, 16, b"rev_trailing_clip", [(50, M), (5, S)], 100), frag(0, 2004, 16, b"rev_plain_2054", [(51, M)], 101),  # u5 = 2054 both
        frag(0, 2, 0, b"u5_negative", [(10, S), (20, M)], 100), frag(0, 4, 0, b"u5_negative_too", [(12, H), (20, M)], 120),      # u5 = -8 both
        frag(0, 3000, 0, b"clip_in_the_middle_of_clips", [(2, S), (10, M), (3, S), (10, M), (4, S)], 100), frag(0, 2998, 0, b"plain_2998", [(5, M)], 50),
    ]
    rng_bad = [frag(0, 10, 0, b"fine", [(5, M)]), frag(0, 0, 0, b"too_far_left", [((1 << 28) - 1, H)] * 9 + [(5, M)]), frag(1, (1 << 31) - 1, 16, b"too_far_right", FAR * 17 + [(8, M)])]
    edge = [frag(0, 0, 0, b"leftmost", [((1 << 28) - 1, H)] * 8 + [(8, S), (5, M)]), frag(1, (1 << 31) - 1, 16, b"rightmost", FAR * 16 + [(17, H)])]   # u5 = -2^31, 3 * 2^31 - 1
    quals = [mrec(0, 500, 0, b"q%d" % q, [(4, M)], bytes([q] * 4)) for q in (14, 15, 93, 94, 0xff)] + \
            [mrec(0, 600, 0, b"saturated_a", [(4, M)], bytes([93] * 11500)), mrec(0, 600, 0, b"saturated_b", [(4, M)], bytes([93] * 12000)),
             mrec(0, 600, 0, b"just_below", [(4, M)], bytes([93] * 11274) + bytes([92]))]                                                                      # 2^20 - 2
    ties = [frag(0, 700, 0, b"tie_a", [(9, M)], 77), frag(0, 700, 0, b"tie_b", [(9, M)], 77), frag(0, 700, 0, b"tie_c", [(9, M)], 77)] + \
           pair(b"ptie_a", 0, 800, 0, 0, 900, 1) + pair(b"ptie_b", 0, 800, 0, 0, 900, 1) + pair(b"ptie_c", 0, 800, 0, 0, 900, 1, q1=50, q2=70) + pair(b"pbest", 1, 800, 0, 1, 900, 1, q1=61) + \
           pair(b"pworse", 1, 800, 0, 1, 900, 1)
    sigs = pair(b"lo_is_hi_a", 0, 100, 0, 0, 100, 0) + pair(b"lo_is_hi_b", 0, 100, 0, 0, 100, 0, q1=70) + \
           pair(b"fr", 0, 300, 0, 0, 451, 1) + pair(b"rf", 0, 251, 1, 0, 500, 0) + pair(b"fr_again", 0, 300, 0, 0, 451, 1, q2=55) + \
           pair(b"mate2_first", 0, 451, 1, 0, 300, 0, q1=90) + \
           pair(b"two_chr_a", 0, 1000, 0, 1, 50, 1) + pair(b"two_chr_b", 0, 1000, 0, 1, 50, 1, q1=99) + pair(b"two_chr_other", 0, 1000, 0, 1, 51, 1)
    frags = pair(b"the_pair", 0, 100, 0, 0, 300, 1) + [
        frag(0, 100, 0, b"on_the_pairs_lo", [(50, M)], 5000), frag(0, 320, 16, b"on_the_pairs_hi", [(30, M)], 5000), frag(0, 100, 16, b"other_strand", [(50, M)]),
        frag(0, 400, 0x49, b"mate_unmapped", [(50, M)]), frag(0, 400, 0x49, b"mate_unmapped_too", [(50, M)], 101), mrec(0, 400, 0x85, b"mate_unmapped", (), quals_of(100)),
        frag(0, 500, 0, b"unpaired", [(50, M)]), frag(0, 500, 0, b"unpaired_better", [(50, M)], 101),
        frag(0, 600, 0x41, b"partner_not_in_store", [(50, M)]), frag(0, 600, 0x41, b"partner_not_in_store_too", [(50, M)], 99),
        frag(0, 700, 0x41, b"both_first", [(50, M)]), frag(0, 800, 0x51, b"both_first", [(50, M)]), frag(0, 700, 0xC1, b"first_and_last", [(50, M)], 120),
        frag(0, 100, 0x141 | DUP, b"the_pair", [(50, M)]), frag(0, 100, 0x841, b"the_pair", [(50, M)]), frag(0, 500, 0x100, b"secondary", [(50, M)], 9000),
        frag(0, 500, 0x800 | DUP, b"supplementary", [(50, M)], 9000),
        mrec(-1, -1, 0x4D | DUP, b"unplaced", (), quals_of(100)), frag(-1, 500, 0, b"unplaced_with_cigar", [(50, M)]), frag(0, -1, 0, b"pos_m1", [(50, M)]),
        mrec(0, 500, 0, b"no_cigar", (), quals_of(9000)), frag(0, 500, 4, b"placed_unmapped", [(50, M)], 9000), frag(0, 900, 0x200, b"qc_fail_is_examined", [(50, M)], 102),
    ]
    in_flag = [frag(0, 100, DUP, b"survivor_marked_on_input", [(50, M)], 200), frag(0, 100, 0, b"loser", [(50, M)], 100), frag(0, 100, DUP, b"loser_marked_on_input", [(50, M)], 50)] + \
              pair(b"pair_marked_on_input", 0, 300, 0, 0, 400, 1, extra1=DUP, extra2=DUP) + [frag(0, 300, 0x100 | DUP, b"secondary_stays_marked", [(50, M)])]
    collisions = {}
    for bits in (4, 8):
        recs = []
        for k, nm in enumerate(collide(bits, 3, b"c%d_" % bits, 12) + collide(bits, 5, b"d%d_" % bits, 12)):
            recs += pair(nm, 0, 100 + 7 * (k % 4), 0, 0, 400 + 7 * (k % 4), 1, q1=60 + k)      # four signatures of six pairs each, drawn from two runs
        recs += [frag(0, 100, 0x41, collide(bits, 3, b"lone%d_" % bits, 1)[0], [(50, M)], 300)]                                   # a candidate without a partner inside a run
        collisions["collide%d" % bits] = recs
    x64, x65 = collide(4, 2, b"x", 1)[0], collide(4, 9, b"y", 1)[0]
    crowd = [mrec(0, 1000 + k, 0x41, x64, [(20, M)], quals_of(60)) for k in range(62)] + pair(collide(4, 2, b"in_the_run_of_64_", 1)[0], 0, 5000, 0, 0, 5200, 1) + \
            [mrec(0, 2000 + k, 0x41, x65, [(20, M)], quals_of(60)) for k in range(63)] + pair(collide(4, 9, b"in_the_run_of_65_", 1)[0], 0, 6000, 0, 0, 6200, 1) + \
            pair(collide(4, 7, b"dup_of_the_64_", 1)[0], 0, 5000, 0, 0, 5200, 1, q1=50) + pair(collide(4, 7, b"dup_of_the_65_", 1)[0], 0, 6000, 0, 0, 6200, 1, q1=50)
    srt = lambda recs, n: sorted(recs, key=lambda r: bsi.key(r, n))
    cases = {
        "cigar": (2, srt(cigar, 2), HASH_BITS, True), "range": (2, srt(rng_bad, 2), HASH_BITS, True), "edge": (2, srt(edge, 2), HASH_BITS, True),
        "quals": (2, srt(quals, 2), HASH_BITS, True), "ties": (2, srt(ties, 2), HASH_BITS, True), "signatures": (2, srt(sigs, 2), HASH_BITS, True),
        "fragments": (2, srt(frags, 2), HASH_BITS, True), "input_flag": (2, srt(in_flag, 2), HASH_BITS, True),
        "malformed": (2, srt(frags[:6] + liars(), 2), HASH_BITS, False), "malformed_last": (2, srt(frags[:6], 2) + liars()[1:2], HASH_BITS, False),
        "malformed_last_cigar": (2, srt(frags[:6], 2) + liars()[:1], HASH_BITS, False),
        "crowd": (2, srt(crowd, 2), 4, True), "empty": (3, [], HASH_BITS, True),
    }
    for k, recs in collisions.items():
        cases[k] = (2, srt(recs, 2), int(k[7:]), True)
    return cases


def random_records(rng, n, n_chr, distinct_scores=False):
    """about n records: families of 2 to 12 pairs on one signature, fragment piles, fragments on pairs' ends, clipped variants that share an unclipped end, and
    a few records that are not examined.  distinct_scores: no two pairs and no two fragments have the same score (the verdict then ignores the input order)"""
    out, serial = [], [0]

    def sc():
        serial[0] += 1
        return 100 + serial[0] if distinct_scores else rng.choice([60, 60, 75, 100, 100, 140])

    def clipped(pos, rev, length=50):
        c = rng.randrange(0, 4)
        if not c:
            return pos, [(length, M)]
        op = rng.choice([S, H])
        return (pos, [(length - c, M), (c, op)]) if rev else (pos + c, [(c, op), (length - c, M)])       # the unclipped 5' end stays

    while len(out) < n:
        kind = rng.randrange(10)
        tid = rng.randrange(n_chr)
        if kind < 5:                                           # a family of pairs
            p1, gap, r1 = rng.randrange(0, 3000), rng.randrange(0, 400), rng.randrange(2)
            t2 = tid if rng.randrange(8) else rng.randrange(n_chr)
            for _ in range(rng.randrange(2, 13)):
                serial[0] += 1
                a, ca = clipped(p1, r1); b, cb = clipped(p1 + gap, 1 - r1)
                out += pair(b"p%d" % serial[0], tid, a, r1, t2, b, 1 - r1, q1=sc(), q2=100 if distinct_scores else sc(), cig1=ca, cig2=cb,
                            extra1=rng.choice([0, 0, DUP]), extra2=0)
                if not rng.randrange(6):                       # a fragment on one of its ends
                    serial[0] += 1
                    out.append(mrec(tid, a, (16 if r1 else 0) | rng.choice([0, 0x49]), b"f%d" % serial[0], ca, quals_of(sc())))
        elif kind < 8:                                         # a pile of fragments
            p, r = rng.randrange(0, 3000), rng.randrange(2)
            for _ in range(rng.randrange(2, 13)):
                serial[0] += 1
                a, ca = clipped(p, r)
                out.append(mrec(tid, a, (16 if r else 0) | rng.choice([0, 0, DUP]), b"f%d" % serial[0], ca, quals_of(sc())))
        else:
            serial[0] += 1
            flag = rng.choice([4, 0x100, 0x800, 0x900 | DUP, 0x41])
            out.append(mrec(rng.choice([-1, tid]), rng.choice([-1, rng.randrange(0, 3000)]), flag, b"n%d" % serial[0], [(50, M)], quals_of(sc())))
    return out


# ---- the native program ----
def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "markdup_checks_san" if sanitize else "markdup_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra +
                              ["-o", exe, os.path.join(common.ROOT, "tests", "native", "markdup_checks.hip")])
    return exe


def run_program(exe, workdir, tag, n_chr, raw, hash_bits=HASH_BITS):
    """-> dict(recs = [(examined, candidate, E, score, h)], bad = index of the first record out of range or None, mate = {index: partner or -1}, dup = {index:
    verdict}, stats = the eight, marked = the bytes)"""
    src = os.path.join(workdir, "md_%s.in" % tag); txt = os.path.join(workdir, "md_%s.txt" % tag); out = os.path.join(workdir, "md_%s.bin" % tag)
    with open(src, "wb") as f:
        f.write(struct.pack("<3q", n_chr, hash_bits, len(raw)) + raw)
    r = subprocess.run([exe, src, txt, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    res = dict(recs=[], bad=None, mate={}, dup={}, stats=None, marked=open(out, "rb").read())
    for line in open(txt).read().splitlines():
        w = line.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "rec":
            res["recs"].append(tuple(v[1:]))
        elif w[0] == "bad":
            res["bad"] = v[0]
        elif w[0] == "mate":
            res["mate"][v[0]] = v[1]
        elif w[0] == "dup":
            res["dup"][v[0]] = bool(v[1])
        elif w[0] == "stats":
            res["stats"] = tuple(v)
    return res
