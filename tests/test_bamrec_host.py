"""CPU suite: the one BAM record reader under every stage on the sorted array (dart_amd/csrc/dg_bamrec.h) through tests/native/bamrec_checks.hip -- bam_head and
the CIGAR walk over crafted records, each at every `avail` from 0 to its length + 4, against the sequential restatement below; and each stage's own policy over
the same bytes (which records it counts, what it does with one it does not) against one line of Python per stage.  The stages disagree on damaged records on
purpose; the restatements here are written from the stage headers' definitions, not from the reader."""
import os
import struct
import subprocess
import pytest
import common

N_CHR, CHR_LEN = 3, 1000
M, I, D, N, S, H, P, EQ, X = range(9)
FILL = b"\xee" * 4
U64 = (1 << 64) - 1


def record(refid, pos, flag, name=b"r", cigar=(), seq_len=0, mapq=30, nxt=(-1, -1, 0), aux=b"", n_cigar=None, l_seq=None, l_name=None, block_size=None, qual=40):
    """a record's bytes; n_cigar, l_seq, l_name and block_size overwrite the stored fields, not the bytes that follow"""
    nm = name + b"\0" if name is not None else b""
    body = nm + b"".join(struct.pack("<I", ln << 4 | op) for op, ln in cigar) + bytes([0x12] * ((seq_len + 1) // 2)) + bytes([qual] * seq_len) + aux
    fixed = struct.pack("<iiBBHHHIiii", refid, pos, len(nm) if l_name is None else l_name, mapq, 4680, len(cigar) if n_cigar is None else n_cigar, flag,
                        seq_len if l_seq is None else l_seq, *nxt)
    return struct.pack("<I", 32 + len(body) if block_size is None else block_size) + fixed + body


ALL_OPS = ((S, 5), (M, 10), (I, 2), (D, 3), (N, 20), (EQ, 4), (X, 1), (P, 2), (H, 3))
RECORDS = {
    "all_nine_ops": record(0, 100, 0x63, b"pair", ALL_OPS, 22, nxt=(0, 300, 250), aux=b"NMC\x01MDZ10^ACG5\0XSi\x05\0\0\0"),
    "n_cigar_0": record(0, 50, 0x0, b"nocigar", (), 10),
    "l_seq_0": record(1, 60, 0x10, b"noseq", ((M, 10),), 0),
    "name_of_1": record(0, 70, 0x0, b"", ((M, 8),), 8),
    "l_name_0": record(0, 70, 0x0, None, ((M, 8),), 8),
    "unplaced": record(-1, -1, 0x4, b"u", (), 6),
    "refid_n_chr": record(N_CHR, 10, 0x0, b"behind", ((M, 4),), 4),
    "pos_minus_1": record(0, -1, 0x0, b"neg", ((M, 4),), 4),
    "pos_minus_2": record(0, -2, 0x0, b"neg2", ((M, 4),), 4),
    "n_cigar_overruns": record(2, 200, 0x0, b"liar", ((M, 6),), 6, n_cigar=60000),
    "l_seq_overruns": record(2, 210, 0x0, b"long", ((M, 6),), 6, l_seq=0x7fffffff),
    "block_size_20": record(0, 5, 0x0, b"tiny", ((M, 2),), 2, block_size=20),
    "block_size_behind": record(0, 5, 0x0, b"over", ((M, 2),), 2, block_size=200),
    "clips_at_the_end": record(1, CHR_LEN - 15, 0x93, b"rev", ((H, 3), (S, 4), (M, 20), (S, 5), (H, 2)), 29, nxt=(1, 700, -300)),
    "ends_behind_2_32": record(0, (1 << 31) - 1, 0x10, b"far", ((N, (1 << 28) - 1),) * 9 + ((M, 10),), 10),
}


def build_program(workdir, sanitize=False):
    import __graft_entry__ as ge
    exe = os.path.join(workdir, "bamrec_checks_san" if sanitize else "bamrec_checks")
    if not os.path.exists(exe):
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([ge.HIPCC, "-O2", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra + ["-o", exe, os.path.join(common.ROOT, "tests", "native", "bamrec_checks.hip")])
    return exe


def run_program(exe, workdir, tag):
    """-> {(record index, avail): {line tag: [ints]}}"""
    src = os.path.join(workdir, "bamrec_%s.in" % tag); out = os.path.join(workdir, "bamrec_%s.txt" % tag)
    with open(src, "wb") as f:
        f.write(struct.pack("<3q", N_CHR, CHR_LEN, len(RECORDS)))
        for rec in RECORDS.values():
            f.write(struct.pack("<q", len(rec)) + rec + bytes(-len(rec) % 8))
    r = subprocess.run([exe, src, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cases, cur = {}, None
    for line in open(out):
        w = line.split()
        if w[0] == "case":
            cur = cases.setdefault((int(w[1]), int(w[2])), {})
        else:
            cur[w[0]] = [int(x) for x in w[1:]]
    return cases


# ---- the restatement: the layout of SAM specification 4.2, read with struct ----
def head(buf):
    avail = len(buf)
    if avail < 36:
        return dict(ok=0, refid=-1, pos=-1, l_name=0, mapq=0, n_cigar=0, flag=0, l_seq=0, next_refid=-1, next_pos=-1, tlen=0, block=0, size=0, cigar_at=0, seq_at=0, qual_at=0, aux_at=0)
    bs, refid, pos, l_name, mapq, _bin, n_cigar, flag, l_seq, nr, np_, tlen = struct.unpack_from("<IiiBBHHHIiii", buf)
    h = dict(ok=1, refid=refid, pos=pos, l_name=l_name, mapq=mapq, n_cigar=n_cigar, flag=flag, l_seq=l_seq, next_refid=nr, next_pos=np_, tlen=tlen, block=4 + bs, size=min(4 + bs, avail))
    h["cigar_at"] = 36 + l_name; h["seq_at"] = h["cigar_at"] + 4 * n_cigar; h["qual_at"] = h["seq_at"] + (l_seq + 1) // 2; h["aux_at"] = h["qual_at"] + l_seq
    return h


HEAD_ORDER = ("ok", "refid", "pos", "l_name", "mapq", "n_cigar", "flag", "l_seq", "next_refid", "next_pos", "tlen", "block", "size", "cigar_at", "seq_at", "qual_at", "aux_at")


def ops_that_fit(buf, h):
    n = min(h["n_cigar"], (h["size"] - h["cigar_at"]) // 4 if h["cigar_at"] <= h["size"] else 0)
    return [(w & 15, w >> 4) for w in struct.unpack_from("<%dI" % n, buf, h["cigar_at"])] if n else []


def walk(ops, pos):
    out, p, q = [], pos & U64, 0
    for op, ln in ops:
        out += [op, ln, p, q]
        if op in (M, D, N, EQ, X):
            p = (p + ln) & U64
        if op in (M, I, S, EQ, X):
            q += ln
    return out, p, q


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return (first + (beg >> shift)) & 0xffffffff
    return 0


def placed(h):
    return 0 <= h["refid"] < N_CHR


def twin_key(h):
    return (h["refid"] if placed(h) else N_CHR) << 33 | ((h["pos"] + 1) & 0xffffffff) << 1 | (h["flag"] >> 4 & 1)


def twin_chk(buf):
    """bs_record_check: the first rule the record breaks (dg_bamsort.h's order), and its size when it breaks none"""
    if len(buf) < 4:
        return [1, 0]
    bs = struct.unpack_from("<I", buf)[0]
    if bs < 32:
        return [2, 0]
    if bs > len(buf) - 4:
        return [1, 0]
    h = head(buf)
    if bs + 4 < h["aux_at"]:
        return [2, 0]
    if h["l_name"] == 0:
        return [3, 0]
    if h["refid"] >= N_CHR:
        return [4, 0]
    if h["pos"] < -1:
        return [5, 0]
    return [0, bs + 4]


def twin_bi(buf, h):
    """the index cuts the ops to what fits and refuses nothing; a short record keeps bin 4680 and end = beg + 1"""
    if not h["ok"]:
        return [-1, -1, 0, 1, 0, 4680, 0, 0]
    mapped = not h["flag"] & 4
    rlen = sum(ln for op, ln in ops_that_fit(buf, h) if op in (M, D, N, EQ, X)) if mapped and h["n_cigar"] else 0
    beg = max(h["pos"], 0); end = max(h["pos"] + (rlen or 1), beg + 1)
    return [h["refid"], h["pos"], beg, end, rlen, reg2bin(beg, end), int(placed(h)), int(mapped)]


def cv_counts(h, exclude):
    """coverage counts a record only when its whole CIGAR lies inside the clamped size"""
    return bool(h["ok"] and placed(h) and h["pos"] >= 0 and not h["flag"] & 4 and h["n_cigar"] > 0 and not h["flag"] & exclude and h["seq_at"] <= h["size"])


def twin_cv(buf, h):
    out = [int(cv_counts(h, 0x704)), h["refid"], h["pos"], h["cigar_at"], h["n_cigar"]]
    if out[0]:
        w, _, _ = walk(ops_that_fit(buf, h), h["pos"])
        for k in range(0, len(w), 4):
            if w[k] in (M, EQ, X) and w[k + 1]:
                out += [w[k + 2], w[k + 2] + w[k + 1]]
    return out


def md_examines(h):
    """the marking examines a record only when its qualities end inside the clamped size, and never a secondary or supplementary one"""
    return bool(h["ok"] and placed(h) and h["pos"] >= 0 and not h["flag"] & 4 and not h["flag"] & 0x900 and h["n_cigar"] > 0 and h["aux_at"] <= h["size"])


def twin_pu_state(buf, h):
    """0 skip, 1 counted, 2 left out, 3 range: the range test comes before the packed bases and l_seq are looked at, left out behind them"""
    if not cv_counts(h, 0):
        return 0, 0
    w, p, q = walk(ops_that_fit(buf, h), h["pos"])
    rlen = p - h["pos"]
    if any(w[k] in (M, EQ, X) and w[k + 1] and w[k + 2] + w[k + 1] > 0xffffffff for k in range(0, len(w), 4)):
        return 3, rlen
    if h["qual_at"] > h["size"] or h["l_seq"] == 0:
        return 0, rlen
    return (1 if q == h["l_seq"] and p <= CHR_LEN else 2), rlen


def twin_qc_whole(h, avail):
    return int(bool(h["ok"] and h["aux_at"] <= h["block"] and h["aux_at"] <= avail))


def twin_tg(buf, h):
    """-> (kind is a rewrite or an unreadable aux area, size): the tags refuse a record whose block_size passes the array's end; the copy's size is clamped"""
    avail = len(buf)
    whole = 4 + struct.unpack_from("<I", buf)[0] if avail >= 4 else None
    size = whole if whole is not None and whole <= avail else avail
    eligible = whole is not None and whole <= avail and twin_pu_state(buf, h)[0] == 1 and h["aux_at"] <= size
    return eligible, size


@pytest.fixture(scope="module")
def cases(workdir):
    return run_program(build_program(workdir), workdir, "plain")


def _bufs():
    for i, rec in enumerate(RECORDS.values()):
        for avail in range(len(rec) + 5):
            yield i, avail, (rec + FILL)[:avail]


def test_the_corpus_holds_what_it_is_there_for(cases):
    assert len(RECORDS) >= 12 and len(cases) == sum(len(r) + 5 for r in RECORDS.values())
    full = {name: head(rec + FILL) for name, rec in RECORDS.items()}
    assert sorted(op for op, _ in ops_that_fit(RECORDS["all_nine_ops"], full["all_nine_ops"])) == list(range(9))
    assert full["n_cigar_0"]["n_cigar"] == 0 and full["l_seq_0"]["l_seq"] == 0 and full["name_of_1"]["l_name"] == 1 and full["l_name_0"]["l_name"] == 0
    assert full["unplaced"]["refid"] == -1 and full["refid_n_chr"]["refid"] == N_CHR and full["pos_minus_1"]["pos"] == -1
    assert full["n_cigar_overruns"]["seq_at"] > full["n_cigar_overruns"]["block"] and full["l_seq_overruns"]["qual_at"] > full["l_seq_overruns"]["block"]
    assert full["block_size_20"]["block"] < 36 and full["block_size_behind"]["block"] > len(RECORDS["block_size_behind"]) + 4


def test_head_and_walk_equal_the_restatement_at_every_avail(cases):
    for i, avail, buf in _bufs():
        got, h = cases[(i, avail)], head(buf)
        assert got["head"] == [h[k] for k in HEAD_ORDER], (i, avail)
        ops = ops_that_fit(buf, h)
        w, p, q = walk(ops, h["pos"])
        assert got["walk"] == [len(ops)] + w + [p, q], (i, avail)


def test_every_stage_keeps_its_own_policy_at_every_avail(cases):
    seen = {"pu": set(), "tg": set(), "chk": set()}
    for i, avail, buf in _bufs():
        got, h, at = cases[(i, avail)], head(buf), (i, avail)
        assert ("key" in got) == (avail >= 36) and (avail < 36 or got["key"] == [twin_key(h)]), at
        assert got["chk"] == twin_chk(buf), at
        assert got["bi"] == twin_bi(buf, h), at
        assert got["cv"] == twin_cv(buf, h), at
        assert got["md"][0] == int(md_examines(h)) and (got["md"][0] or got["md"][1:6] == [0, 0, 0, 0, 0]), at
        assert got["md"][6] == (max(h["l_name"] - 1, 0) if avail >= 36 else 0), at
        state, rlen = twin_pu_state(buf, h)
        counted = cv_counts(h, 0)
        assert got["pu"] == [state, h["refid"], h["pos"], h["n_cigar"], h["l_seq"] if counted else 0, (h["flag"] >> 4 & 1) if counted else 0, h["cigar_at"], h["seq_at"] if counted else 0, rlen], at
        assert got["qc"] == [twin_qc_whole(h, avail), h["flag"], h["mapq"], h["l_seq"], h["refid"], h["pos"], h["next_refid"], h["next_pos"], h["tlen"]], at
        eligible, size = twin_tg(buf, h)
        assert (got["tg"][0] != 1) == eligible and got["tg"][1] == size and (not eligible or got["tg"][2] == h["aux_at"]), at
        seen["pu"].add(state); seen["tg"].add(got["tg"][0]); seen["chk"].add(got["chk"][0])
    assert seen["pu"] == {0, 1, 2, 3} and seen["tg"] >= {0, 1} and seen["chk"] == {0, 1, 2, 3, 4, 5}
    # the differences between the stages that must survive, each on the record that shows it (at its full length)
    full = lambda name: cases[(list(RECORDS).index(name), len(RECORDS[name]) + 4)]
    liar, long_ = full("n_cigar_overruns"), full("l_seq_overruns")
    assert liar["cv"][0] == 0 and liar["walk"][0] == 3 and liar["bi"][4] >= 6 and liar["bi"][6:] == [1, 1]      # coverage refuses the CIGAR that overruns, the index cuts it to the three words that fit
    assert long_["cv"][0] == 1 and long_["md"][0] == 0 and long_["pu"][0] == 0 and long_["qc"][0] == 0      # a CIGAR inside is enough for coverage, not for the others
    over = full("block_size_behind")
    assert over["cv"][0] == 1 and over["md"][0] == 1 and over["pu"][0] == 1 and over["qc"][0] == 1 and over["tg"][0] == 1      # block > avail: only the tags refuse
    assert full("ends_behind_2_32")["pu"][0] == 3 and full("clips_at_the_end")["pu"][0] == 2 and full("l_seq_0")["pu"][0] == 0
    assert full("all_nine_ops")["tg"][0] == 0 and full("all_nine_ops")["tg"][4] == 2             # NM and MD go, XS stays
    sec = cases[(list(RECORDS).index("all_nine_ops"), len(RECORDS["all_nine_ops"]))]
    assert sec["md"][0] == 1 and sec["md"][1] == 1


def test_the_reader_under_the_sanitizers(workdir, cases):
    """the same program with AddressSanitizer and UBSan on its host code: every case is an exact-size heap copy of its `avail` bytes, so a read behind `avail`
    leaves its allocation.  Stand-alone; never through python's process, never on the GPU."""
    assert run_program(build_program(workdir, sanitize=True), workdir, "san") == cases
