"""Helpers of the trimming tests: the sequential twin of the definition in include/dartgpu.h (dg_set_trim: quality ends, adapter, poly tails, length; the kept
reads compacted), the crafted reads that sit on the kernels' seams -- with the assertions that each case occurs --, adapter read-through laid over golden
reads, and the driver of tests/native/trim_checks.hip."""
from __future__ import annotations

import os, subprocess
import numpy as np
import common
import fastq_device_inputs as fdi

PAIRS = 1
ADAPTERS = {"illumina": b"AGATCGGAAGAGC", "nextera": b"CTGTCTCTTATA", "smallrna": b"TGGAATTCTCGG"}
STAT_KEYS = ["reads_in", "reads_kept", "bases_in", "bases_kept", "qual5_bases", "qual3_bases", "adapter0_reads", "adapter1_reads", "adapter_bases", "poly_reads",
             "poly_bases", "too_short_reads", "mate_dropped_reads", "qual_skipped_reads", "reserved14", "reserved15"]


def params(**kw):
    p = dict(flags=0, qual3=0, qual5=0, qual_base=33, min_overlap=3, max_err_permille=100, poly_mask=0, poly_min=10, min_len=1, adapter=(b"", b""))
    p.update(kw)
    return p


def poly_mask(letters: str) -> int:
    return sum(1 << "ACGT".index(c) for c in letters)


# ---- the definition, one read ----------------------------------------------------------------------------------------------------------------
def _up(c: int) -> int:
    return c - 32 if 97 <= c <= 122 else c


def _eq(c: int, a: int) -> bool:
    return _up(c) == a and a in b"ACGT"


def qual_walk(v, cutoff):
    """the walk over v in walking order -> the step at which the sum first reached its strict maximum > 0, or None"""
    s, mx, at = 0, 0, None
    for t, x in enumerate(v):
        s += cutoff - x
        if s < 0:
            break
        if s > mx:
            mx, at = s, t
    return at


def window(s: bytes, q: bytes, p, adapter: bytes):
    """-> (a, b, what): the window of one read in file orientation; what: cut5, cut3, adapter (bool), ad_cut, poly (bool), poly_cut, qskip"""
    L = len(s)
    a, b = 0, L
    w = dict(cut5=0, cut3=0, adapter=False, ad_cut=0, poly=False, poly_cut=0, qskip=False, early_stop=False, tie=False)
    if p["qual3"] or p["qual5"]:
        if len(q) == L:
            v = [c - p["qual_base"] for c in q]
            if p["qual3"]:
                t = qual_walk(v[::-1], p["qual3"])
                b = L if t is None else L - 1 - t
                # (for the crafted cases: would the walk without the early stop, or with "last maximum", have said something else?)
                sums = np.cumsum([p["qual3"] - x for x in v[::-1]])
                t_all = int(np.argmax(sums)) if sums.max() > 0 else None
                w["early_stop"] = t_all != t
                neg = np.nonzero(sums < 0)[0]
                seen = sums[:neg[0]] if len(neg) else sums
                w["tie"] = len(seen) > 0 and seen.max() > 0 and int((seen == seen.max()).sum()) > 1
            if p["qual5"]:
                t = qual_walk(v, p["qual5"])
                a = 0 if t is None else t + 1
            if a >= b:
                w["cut5"], w["cut3"] = a, L - a
                a = b = 0
            else:
                w["cut5"], w["cut3"] = a, L - b
        else:
            w["qskip"] = True
    if len(adapter):
        for pos in range(a, b - p["min_overlap"] + 1):
            n = min(b - pos, len(adapter))
            m = sum(1 for i in range(n) if not _eq(s[pos + i], adapter[i]))
            if m * 1000 <= n * p["max_err_permille"]:
                w["adapter"], w["ad_cut"], w["ad_n"], w["ad_m"] = True, b - pos, n, m
                b = pos
                break
    if p["poly_mask"] and b > a:
        nb = b
        for ci in range(4):
            if not (p["poly_mask"] >> ci) & 1:
                continue
            c = b"ACGT"[ci]
            best, at, run = None, None, 0
            for i in range(b - 1, a - 1, -1):
                run += 1 if _up(s[i]) == c else -2
                if best is None or run >= best:
                    best, at = run, i
            if best is not None and best > 0 and b - at >= p["poly_min"]:
                nb = min(nb, at)
        if nb < b:
            w["poly"], w["poly_cut"] = True, b - nb
            b = nb
    return a, b, w


# ---- the batch -----------------------------------------------------------------------------------------------------------------------------------
def records(text1: bytes, text2=None):
    """the records of one or two texts in batch order, in file orientation -> [(name, read, quality cut to the read, file)] (the plain reader's rules,
    fastq_device_inputs.get_next_entry; the stream ends at the first record without bases)"""
    f1 = fdi._File(text1); f2 = fdi._File(text2) if text2 is not None else f1
    out = []
    while True:
        h, s, q, rlen = fdi.get_next_entry(f1)
        if rlen <= 0:
            break
        out.append((h, s, q, 0))
        h, s, q, rlen = fdi.get_next_entry(f2)
        if rlen <= 0:
            break
        out.append((h, s, q, 1 if text2 is not None else 0))
    return out


def trim_batch(recs, p, two: bool, rc_odd: bool):
    """-> (kept [(name, stored read, stored quality)], stats [16], windows [(a, b, what)], kept indices, file-orientation kept [(name, read, quality, file)])"""
    pairs = bool(p["flags"] & PAIRS)
    wins = []
    for k, (h, s, q, f) in enumerate(recs):
        ad = f if two else ((k & 1) if pairs else 0)
        wins.append(window(s, q, p, p["adapter"][ad]) + (ad,))
    own = [b - a >= p["min_len"] for a, b, w, ad in wins]
    st = [0] * 16
    kept, idx, plain = [], [], []
    for k, (h, s, q, f) in enumerate(recs):
        a, b, w, ad = wins[k]
        mate = own[k ^ 1] if pairs and (k ^ 1) < len(recs) else True
        keep = own[k] and mate
        st[0] += 1; st[2] += len(s); st[4] += w["cut5"]; st[5] += w["cut3"]
        if w["adapter"]:
            st[6 + ad] += 1; st[8] += w["ad_cut"]
        if w["poly"]:
            st[9] += 1; st[10] += w["poly_cut"]
        st[11] += not own[k]; st[12] += own[k] and not mate; st[13] += w["qskip"]
        if keep:
            st[1] += 1; st[3] += b - a
            ts, tq = s[a:b], q[a:min(b, len(q))] if a < len(q) else b""
            plain.append((h, ts, tq, f)); idx.append(k)
            if rc_odd and (k & 1):
                ts, tq = fdi.get_complementary_seq(ts), tq[::-1]
            kept.append((h, ts, tq))
    return kept, st, [(a, b, w) for a, b, w, ad in wins], idx, plain


def fastq_of(plain, two: bool):
    """the FASTQ text(s) of file-orientation reads, as a trimming tool would write them back -> (text1, text2 or None)"""
    out = [[], []]
    for h, s, q, f in plain:
        out[f if two else 0].append(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n")
    return b"".join(out[0]), (b"".join(out[1]) if two else None)


# ---- crafted reads -------------------------------------------------------------------------------------------------------------------------------
ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCACGGCTACATCTCGTATGCCGTCTTCTGCTTG"      # 64 bases
assert len(ADAPTER) == 64
CRAFT = params(qual3=20, qual5=15, min_overlap=5, max_err_permille=100, poly_mask=poly_mask("GA"), poly_min=10, min_len=8, adapter=(ADAPTER, ADAPTER[:20]))


def _rand(rng, n, alphabet=b"ACT"):
    """random bases without G (no accidental poly-G) that do not start like the adapter"""
    return bytes(alphabet[i] for i in rng.integers(0, len(alphabet), size=n))


def _mutate(a: bytes, at):
    """a with the bases at `at` replaced by another ACGT base"""
    out = bytearray(a)
    for i in at:
        out[i] = b"CATG"[b"ACGT".index(out[i])]
    return bytes(out)


def crafted_reads(seed=17):
    """-> [(label, read, quality)]: single reads, each built for one rule of CRAFT; their labels are asserted on in crafted_cases()"""
    rng = np.random.default_rng(seed)
    hi = lambda n: b"I" * n
    out = []
    for L in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000):                 # the packed-word and wave-round seams: the adapter's first bases end the read
        body = _rand(rng, max(L - 7, 0))
        out.append(("len%d" % L, (body + ADAPTER[:7])[:L] if L >= 7 else _rand(rng, L), hi(L)))
        out.append(("len%d_plain" % L, _rand(rng, L), hi(L)))
    out.append(("all_adapter", ADAPTER[:40], hi(40)))
    out.append(("overlap_min", _rand(rng, 50) + ADAPTER[:5], hi(55)))
    out.append(("overlap_min_less_1", _rand(rng, 50) + ADAPTER[:4], hi(54)))
    for n in (9, 10, 19, 20, 64):                                               # mismatches at floor(n / 10) and one above
        k = n // 10
        spread = lambda cnt: [1 + (i * (n - 2)) // max(cnt, 1) for i in range(cnt)]
        tail = lambda cnt: _rand(rng, 40) + _mutate(ADAPTER[:n], spread(cnt)) + (_rand(rng, 30) if n == 64 else b"")
        t = tail(k); out.append(("mm%d_at" % n, t, hi(len(t))))
        t = tail(k + 1); out.append(("mm%d_above" % n, t, hi(len(t))))
    out.append(("adapter_longer_than_rest", _rand(rng, 60) + ADAPTER[:30], hi(90)))
    t = _rand(rng, 30) + ADAPTER[:8] + b"N" + ADAPTER[9:30]; out.append(("n_inside", t, hi(len(t))))
    t = _rand(rng, 30) + ADAPTER[:30].lower(); out.append(("lower_inside", t, hi(len(t))))
    t = _rand(rng, 30) + ADAPTER[:8] + b"R" + ADAPTER[9:30]; out.append(("iupac_inside", t, hi(len(t))))
    t = _rand(rng, 30) + ADAPTER[:4] + b"N" + ADAPTER[5:9]; out.append(("n_breaks_short_match", t, hi(len(t))))
    # quality walks: '#' = 2, '5' = 20, 'I' = 40 (base 33)
    out.append(("q_early_stop", _rand(rng, 60), hi(15) + b"#" * 40 + hi(3) + b"##"))        # the walk stops in the good stretch; without the stop it would cut 40 bases more
    out.append(("q_tie", _rand(rng, 60), hi(40) + b"5" * 10 + b"#" * 10))                    # quality 20 adds 0: the maximum is met again ten times, the first one counts
    out.append(("q_both_ends", _rand(rng, 80), b"#" * 7 + hi(60) + b"#" * 13))
    out.append(("q_all_bad", _rand(rng, 40), b"#" * 40))
    out.append(("q_crosses_round", _rand(rng, 200), hi(100) + b"#" * 100))
    out.append(("ql_short", _rand(rng, 50) + ADAPTER[:20], hi(40) + b"#" * 5))
    out.append(("poly_min", _rand(rng, 50) + b"G" * 10, hi(60)))
    out.append(("poly_min_less_1", _rand(rng, 50) + b"G" * 9, hi(59)))
    out.append(("poly_interrupted", _rand(rng, 50) + b"G" * 8 + b"T" + b"G" * 12, hi(71)))
    out.append(("poly_two_bases", _rand(rng, 50, b"CT") + b"A" * 30 + b"G" * 10, hi(90)))      # both tails count: G's is 10 long, A's (score -20 + 30) reaches 40 bases in
    out.append(("poly_long", _rand(rng, 20, b"CT") + b"G" * 150, hi(170)))
    out.append(("poly_lower", _rand(rng, 40) + b"g" * 15, hi(55)))
    return out


def crafted_cases():
    """the crafted reads under CRAFT: asserts from the twin that every case they are built for occurs -> the reads"""
    reads = crafted_reads()
    got = {label: window(s, q if label != "ql_short" else q, CRAFT, ADAPTER) for label, s, q in reads}
    L = {label: len(s) for label, s, q in reads}
    for n in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000):
        a, b, w = got["len%d" % n]
        assert (w["adapter"] and b == n - 7) if n >= 7 else not w["adapter"], (n, a, b, w)
        assert not got["len%d_plain" % n][2]["adapter"]
    a, b, w = got["all_adapter"]; assert w["adapter"] and a == b == 0
    assert got["overlap_min"][2]["adapter"] and got["overlap_min"][2]["ad_n"] == CRAFT["min_overlap"] and not got["overlap_min_less_1"][2]["adapter"]
    for n in (9, 10, 19, 20, 64):
        w = got["mm%d_at" % n][2]; assert w["adapter"] and w["ad_n"] == n and w["ad_m"] == n // 10 and got["mm%d_at" % n][1] == 40, (n, w)
        a, b, w = got["mm%d_above" % n]; assert not (w["adapter"] and b == 40), (n, w)
    w = got["adapter_longer_than_rest"][2]; assert w["adapter"] and w["ad_n"] == 30 < len(ADAPTER)
    for label in ("n_inside", "lower_inside", "iupac_inside"):
        a, b, w = got[label]; assert w["adapter"] and b == 30 and w["ad_m"] == (0 if label == "lower_inside" else 1), (label, w)
    assert not got["n_breaks_short_match"][2]["adapter"]
    a, b, w = got["q_early_stop"]; assert w["early_stop"] and b == 58, (a, b, w)
    a, b, w = got["q_tie"]; assert w["tie"] and b == 50, (a, b, w)
    a, b, w = got["q_both_ends"]; assert (a, b) == (7, 67)
    a, b, w = got["q_all_bad"]; assert a == b == 0 and w["cut5"] + w["cut3"] == 40
    a, b, w = got["q_crosses_round"]; assert b == 100
    a, b, w = got["ql_short"]; assert w["qskip"] and w["adapter"] and b == 50
    a, b, w = got["poly_min"]; assert w["poly"] and b == 50
    assert not got["poly_min_less_1"][2]["poly"]
    a, b, w = got["poly_interrupted"]; assert w["poly"] and b == 50
    a, b, w = got["poly_two_bases"]; assert w["poly"] and b == 50 and w["poly_cut"] == 40
    a, b, w = got["poly_long"]; assert w["poly"] and b == 20
    a, b, w = got["poly_lower"]; assert w["poly"] and b == 40
    return reads


def text_of(reads, tag=""):
    """[(label, read, quality)] -> FASTQ text; "ql_short" style reads (a quality shorter than the read) keep their short line"""
    return b"".join(b"@" + label.encode() + tag.encode() + b"\n" + s + b"\n+\n" + q + b"\n" for label, s, q in reads)


def many_reads(n, seed, drop_at):
    """n reads of 30..90 bases; those at drop_at are 5 bases long (they fail CRAFT's min_len of 8)"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = 5 if k in drop_at else int(rng.integers(30, 91))
        s = _rand(rng, L)
        if k % 3 == 0 and L > 20:
            s = s[:L - 12] + ADAPTER[:12]
        out.append(("m%d" % k, s, b"I" * L))
    return out


def pair_texts():
    """-> (text 1, text 2, both interleaved, the interleaved text with an unpaired last read): the crafted reads as mates 1, as mates 2 reads of their own whose
    adapter is CRAFT's second; in pair 4 only mate 2 fails the length, in pair 6 only mate 1; text 1 holds one record more (the stream's unpaired last read)"""
    m1 = crafted_cases()
    rng = np.random.default_rng(23)
    m2 = []
    for k in range(len(m1)):
        L = 5 if k == 4 else int(rng.integers(20, 120))
        s = _rand(rng, L)
        if k % 2 == 1 and L > 30:
            s = s[:L - 15] + ADAPTER[:15]
        m2.append(("mate%d" % k, s, b"I" * L))
    m1 = list(m1); m1[6] = ("short1", b"ACTCA", b"IIIII")
    last = ("unpaired", _rand(rng, 70) + ADAPTER[:9], b"I" * 79)
    r1 = [text_of([r], "/1") for r in m1]; r2 = [text_of([r], "/2") for r in m2]
    inter = b"".join(a + b for a, b in zip(r1, r2))
    return b"".join(r1) + text_of([last], "/1"), b"".join(r2), inter, inter + text_of([last], "/1")


# ---- adapter read-through over golden reads -----------------------------------------------------------------------------------------------------
def spoil(m, seed, adapter: bytes, frac=3):
    """rows of reads (uint8 [n, rlen]) -> [(read bytes, quality bytes)]: every `frac`-th read gets, from a random insert size on, the adapter, then random
    bases, under low qualities; a few get a poly-G tail in front of nothing else"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(m.shape[0]):
        s = bytearray(m[i].tobytes()); L = len(s)
        q = bytearray(33 + 30 + int(x) for x in rng.integers(0, 11, size=L))
        if i % frac == 0:
            ins = int(rng.integers(0, L - 4))                       # a short insert leaves a read that fails the length
            t = (adapter + _rand(rng, L, b"ACGT"))[:L - ins]
            s[ins:] = t
            for j in range(max(ins, L - 15), L):
                q[j] = 33 + 2
        elif i % 17 == 1:
            n = int(rng.integers(12, 30))
            s[L - n:] = b"G" * n
        out.append((bytes(s), bytes(q)))
    return out


# ---- the lane code on the host ---------------------------------------------------------------------------------------------------------------------
def build_checks_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "trim_checks" + ("_asan" if sanitize else ""))
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra + ["-o", exe, os.path.join(common.ROOT, "tests", "native", "trim_checks.hip")])
    return exe


def run_checks_program(exe, path, text1: bytes, text2, rc_odd: bool, p):
    """-> (status, windows [(a, b, cut5, cut3, ad_cut, poly_cut, flags)], stats [16], kept [(name, stored read, stored quality)]); status -1: the counts do not fit"""
    t2 = text2 if text2 is not None else b""
    ad = [bytes(x) for x in p["adapter"]]
    with open(path, "wb") as f:
        f.write(np.asarray([int(text2 is not None), int(rc_odd), len(text1), len(t2)], np.int64).tobytes())
        f.write(np.asarray([p["flags"], p["qual3"], p["qual5"], p["qual_base"], p["min_overlap"], p["max_err_permille"], p["poly_mask"], p["poly_min"], p["min_len"],
                            len(ad[0]), len(ad[1]), 0], np.uint32).tobytes())
        for a in ad:
            f.write(a + b"\0" * (64 - len(a)))
        for t in (text1, t2):
            f.write(t + b"\0" * (-len(t) % 8))
    r = subprocess.run([exe, path, path + ".out"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(path + ".out", "rb").read()
    n_in, n_kept = (int(x) for x in np.frombuffer(raw, np.int64, 2))
    if n_in < 0:
        return -1, [], [], []
    stats = [int(x) for x in np.frombuffer(raw, np.uint64, 16, 16)]
    w = np.frombuffer(raw, np.uint16, 8 * n_in, 16 + 128).reshape(n_in, 8)
    at = 16 + 128 + 16 * n_in
    lens = np.frombuffer(raw, np.uint32, 3 * n_kept, at).reshape(n_kept, 3); at += 12 * n_kept
    kept = []
    for k in range(n_kept):
        rl, hl, ql = (int(x) for x in lens[k])
        s = raw[at:at + rl]; at += rl
        h = raw[at:at + hl]; at += hl
        q = raw[at:at + ql]; at += ql
        kept.append((h, s, q))
    assert at == len(raw)
    return 0, [tuple(int(x) for x in row[:7]) for row in w], stats, kept


F_ADAPTER, F_ADAPTER1, F_POLY, F_QSKIP, F_KEEP = 1, 2, 4, 8, 16


def window_row(a, b, w, ad, keep):
    """a twin window as the row the native program and the kernel leave"""
    return (a, b, w["cut5"], w["cut3"], w["ad_cut"], w["poly_cut"],
            (F_ADAPTER if w["adapter"] else 0) | (F_ADAPTER1 if w["adapter"] and ad else 0) | (F_POLY if w["poly"] else 0) | (F_QSKIP if w["qskip"] else 0) | (F_KEEP if keep else 0))
