"""GPU suite: `dart -bo` with DART_UMI=8 and DART_MARK_DUPLICATES=1 DART_MARKDUP_UMI=exact|edit1 beside the sort switches -- the 8 letters in front of mate 1 are
cut inside the upload and go to the end of the read's name, where they are part of a duplicate's signature -- against the sequential twin of
tests/umidup_inputs.py computed from the unmarked file alone; the counts' files; that without DART_MARKDUP_UMI both sets of copies are marked as before; and what
the switches say when they cannot be used."""
import os, random, subprocess
import pytest
import common
import bamidx_inputs as bii
import bamsort_inputs as bsi
import markdup_inputs as mdi
import umidup_inputs as udi

pytestmark = pytest.mark.gpu
DART = os.path.join(common.ROOT, "dart_amd", "dart")
SWITCHES = ("DART_DEVICE_BAM", "DART_DEVICE_FASTQ", "DART_DEVICE_SAM", "DART_SORT_BAM", "DART_BAM_INDEX", "DART_BGZF_DYNAMIC", "DART_SORT_PIECE_MB", "DART_GPUS", "DART_COVERAGE",
            "DART_MARK_DUPLICATES", "DART_MARKDUP_UMI", "DART_MARKDUP_UMI_SEP", "DG_MARKDUP_HASH_BITS", "DART_UMI", "DART_UMI_SKIP", "DART_UMI_SEP", "DART_TRIM_QUAL")
SORTED = {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1", "DART_DEVICE_FASTQ": "1", "DART_UMI": "8"}
N_COPIES = 100
N_PAIRS = 600


def _spawn(d, args, extra):
    env = dict(os.environ, DART_TIMING="1", DART_BATCH="400", **extra)
    for k in SWITCHES:
        if k not in extra:
            env.pop(k, None)
    return subprocess.run([DART] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def _run(d, args, extra):
    r = _spawn(d, args, extra)
    assert r.returncode == 0, r.stderr[-600:]
    return r


def _read(d, name):
    return open(os.path.join(d, name), "rb").read()


def _umis(n):
    """per pair an 8-letter UMI, and one three letters away from it"""
    rng = random.Random(8)
    own = [bytes(rng.choice(b"ACGT") for _ in range(8)) for _ in range(n)]
    far = [bytes(b"CGTA"[b"ACGT".index(c)] for c in u[:3]) + u[3:] for u in own]
    return own, far


def _write_fastq(path, seqs, mate):
    """the case's first pairs with their UMI in front of mate 1; the first N_COPIES twice more, every quality one lower: once with the original's UMI, once with
    one at distance 3"""
    own, far = _umis(len(seqs))
    with open(path, "wb") as f:
        for stem, umis, q, n in ((b"r", own, b"I", len(seqs)), (b"same", own, b"H", N_COPIES), (b"other", far, b"H", N_COPIES)):
            for i, s in enumerate(seqs[:n]):
                s = (umis[i] if mate == 1 else b"") + s.tobytes()
                f.write(b"@" + stem + b"%d/%d\n" % (i, mate) + s + b"\n+\n" + q * len(s) + b"\n")


def _marked(raw):
    return {nm for nm, flag in mdi.flags_by_name(raw) if flag & mdi.DUP}


def test_dart_cli_marks_duplicates_by_position_and_umi(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("pe101_spliced", workdir)
    d = os.path.join(workdir, "umi_cli"); os.makedirs(d, exist_ok=True)
    _write_fastq(os.path.join(d, "1.fq"), c["m1"][:N_PAIRS], 1); _write_fastq(os.path.join(d, "2.fq"), c["m2"][:N_PAIRS], 2)
    args = ["-i", c["prefix"], "-f", "1.fq", "-f2", "2.fq", "-j", "o.j", "-t", "4"] + c["runs"][0]["flags"]
    own, far = _umis(N_PAIRS)
    _run(d, args + ["-bo", "plain.bam"], SORTED)
    first, _, raw, n_chr = bii.split_file(_read(d, "plain.bam"))
    names = {nm for nm, _ in mdi.flags_by_name(raw)}
    assert b"r0_" + own[0] in names and b"same0_" + own[0] in names and b"other0_" + far[0] in names          # names end in _<UMI>: the upload cut it off mate 1
    n_in = 2 * (N_PAIRS + 2 * N_COPIES)
    assert _read(d, "plain.bam.trim.txt").splitlines()[-2:] == [b"umi_bases\t%d" % (8 * n_in // 2), b"umi_dropped_reads\t0"] and len(_read(d, "plain.bam.trim.txt").splitlines()) == 16
    assert all(rec[20:24] == (101).to_bytes(4, "little") for rec in bsi.split(raw))                         # every read is back at its 101 bases
    # without DART_MARKDUP_UMI: position alone, both sets of copies are marked
    _run(d, args + ["-bo", "position.bam"], dict(SORTED, DART_MARK_DUPLICATES="1"))
    by_position = _marked(bii.split_file(_read(d, "position.bam"))[2])
    same = {i for i in range(N_COPIES) if b"same%d_" % i + own[i] in by_position}
    assert len(same) >= 10 and same == {i for i in range(N_COPIES) if b"other%d_" % i + far[i] in by_position}
    assert len(_read(d, "position.bam.markdup.txt").splitlines()) == 8
    # with it: the file the twin predicts; the copies under the original's UMI carry 0x400, those under another do not
    for mode, max_edit in (("exact", 0), ("edit1", 1)):
        want, stats, _ = udi.twin(raw, n_chr, max_edit)
        _run(d, args + ["-bo", mode + ".bam"], dict(SORTED, DART_MARK_DUPLICATES="1", DART_MARKDUP_UMI=mode))
        first2, _, raw2, n_chr2 = bii.split_file(_read(d, mode + ".bam"))
        assert (first2, n_chr2) == (first, n_chr) and raw2 == want and raw2 != raw
        marked = _marked(raw2)
        assert {i for i in range(N_COPIES) if b"same%d_" % i + own[i] in marked} == same and not any(nm.startswith(b"other") for nm in marked)
        assert _read(d, mode + ".bam.markdup.txt") == b"".join(b"%s\t%d\n" % (k, v) for k, v in zip(
            (b"examined_records", b"pairs", b"fragments", b"duplicate_pairs", b"duplicate_fragments", b"candidates_in_crowded_runs", b"records_marked_duplicate", b"largest_family",
             b"records_with_umi", b"pair_families_of_several_umis", b"umi_groups_absorbed", b"crowded_umi_families"), stats))
        assert stats[8] == stats[0] and stats[9] >= 10 and stats[10] == 0
    # another separator: no name holds a UMI, the marking by position again
    _run(d, args + ["-bo", "colon.bam"], dict(SORTED, DART_MARK_DUPLICATES="1", DART_MARKDUP_UMI="exact", DART_MARKDUP_UMI_SEP=":"))
    assert _read(d, "colon.bam") == _read(d, "position.bam") and _read(d, "colon.bam.markdup.txt").splitlines()[8] == b"records_with_umi\t0"


def test_dart_cli_umi_switches_say_what_is_wrong(workdir):
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("se100", workdir)
    d = os.path.join(workdir, "umi_missing"); os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "1.fq"), "wb") as f:
        for i, s in enumerate(c["m1"][:50]):
            f.write(b"@r%d/1\n" % i + s.tobytes() + b"\n+\n" + b"I" * len(s) + b"\n")
    args = ["-i", c["prefix"], "-f", "1.fq", "-j", "o.j", "-t", "4"] + c["runs"][0]["flags"]
    sorted_only = {"DART_DEVICE_BAM": "1", "DART_SORT_BAM": "1"}
    marked = dict(sorted_only, DART_MARK_DUPLICATES="1")
    for out, extra, text in ((["-bo", "a.bam"], dict(sorted_only, DART_MARKDUP_UMI="exact"), "Error! DART_MARKDUP_UMI=exact needs DART_MARK_DUPLICATES=1"),
                             (["-o", "b.sam"], {"DART_MARKDUP_UMI": "edit1"}, "Error! DART_MARKDUP_UMI=edit1 needs DART_MARK_DUPLICATES=1"),
                             (["-bo", "c.bam"], dict(marked, DART_MARKDUP_UMI="1"), "Error! DART_MARKDUP_UMI=1: exact or edit1"),
                             (["-bo", "e.bam"], dict(marked, DART_MARKDUP_UMI="exact", DART_MARKDUP_UMI_SEP="__"), "Error! DART_MARKDUP_UMI_SEP=__: one byte"),
                             (["-bo", "f.bam"], {"DART_UMI": "8", "DART_DEVICE_BAM": "1"}, "Error! DART_UMI needs the device parser and a device formatter"),
                             (["-o", "g.sam"], {"DART_UMI": "8", "DART_DEVICE_FASTQ": "1"}, "Error! DART_UMI needs the device parser and a device formatter"),
                             (["-o", "h.sam"], {"DART_UMI": "12,12", "DART_DEVICE_FASTQ": "1", "DART_DEVICE_SAM": "1"}, "Error! DART_UMI=12,12: "),
                             (["-o", "i.sam"], {"DART_UMI": "8", "DART_UMI_SEP": "A", "DART_DEVICE_FASTQ": "1", "DART_DEVICE_SAM": "1"}, "Error! DART_UMI_SEP=A: ")):
        r = _spawn(d, args + out, extra)
        err = r.stderr.decode("latin1").splitlines()
        assert r.returncode == 1 and len(err) == 1 and err[0].startswith(text), (r.returncode, err)
        assert not os.path.exists(os.path.join(d, out[1])) and not os.path.exists(os.path.join(d, out[1] + ".markdup.txt"))
