"""CPU suite: from a GTF file to the expression stage's tables, the way `dart` goes under DART_TX_QUANT (gtf_parse_transcripts of dart_amd/csrc/host/gtf.h, then
tx_flatten of dart_amd/csrc/dg_txquant.h) through tests/native/gtf_tx_checks.hip: transcripts in the order of their first line, exons merged whatever the order
of their lines, lengths, prefix lengths and the segment table against tests/txquant_inputs.py; a line the reader refuses is named.  Built plain and with the
address and undefined-behaviour sanitizers on its host code; the program stands alone."""
import os, random, subprocess
import pytest
import common
import txquant_inputs as txi

NAMES = ["chr1", "chrTwo", "3"]


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan+ubsan"])
def exe(request, workdir):
    import __graft_entry__ as ge
    out = os.path.join(workdir, "gtf_tx_checks_san" if request.param else "gtf_tx_checks")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param else []
    subprocess.check_call([ge.HIPCC, "-O1", "--offload-arch=gfx950", "-std=c++17", "-w"] + extra + ["-o", out, os.path.join(common.ROOT, "tests", "native", "gtf_tx_checks.hip")])
    return out


def _run(exe, path, names=NAMES):
    r = subprocess.run([exe, path] + list(names), capture_output=True, text=True)
    assert r.returncode in (0, 1), r.stdout + r.stderr
    tx, mex, segs, skipped, err = [], {}, [[] for _ in names], None, None
    for line in r.stdout.splitlines():
        w = line.split(" ", 1)
        if w[0] == "error":
            err = w[1]
        elif w[0] == "tx":
            f = w[1].split(" ", 5)
            tx.append(tuple(int(x) for x in f[1:5]) + (f[5],))
        elif w[0] == "mex":
            v = [int(x) for x in w[1].split()]
            mex.setdefault(v[0], []).append(tuple(v[1:]))
        elif w[0] == "seg":
            v = [int(x) for x in w[1].split()]
            segs[v[0]].append((v[1], tuple(v[2:])))
        elif w[0] == "skipped":
            skipped = tuple(int(x) for x in w[1].split())
    assert (r.returncode == 0) == (err is None)
    return tx, mex, segs, skipped, err


def test_a_written_annotation_comes_back_merged_and_segmented(exe, workdir):
    rng = random.Random(6)
    tr = txi.random_annotation(rng, [6000, 3000, 2500]) + [(2, 1, [(0, 10)]), (0, 0, [((1 << 32) - 11, (1 << 32) - 1), (5, 9)])]
    path = os.path.join(workdir, "tx_written.gtf")
    names = txi.write_gtf(path, tr, NAMES, rng=rng)
    tx, mex, segs, skipped, err = _run(exe, path)
    assert err is None and skipped == (1, 1)
    L = txi.lengths(tr)
    assert tx == [(c, st, L[t], len(txi.merged(ex)), names[t]) for t, (c, st, ex) in enumerate(tr)]
    for t, (_, _, ex) in enumerate(tr):
        m = txi.merged(ex)
        assert mex[t] == [(s, e, sum(b - a for a, b in m[:k])) for k, (s, e) in enumerate(m)]
    assert segs == txi.segments_twin(tr, 3)


def test_a_refused_line_is_named_and_no_transcript_is_an_error(exe, workdir):
    path = os.path.join(workdir, "tx_bad.gtf")
    good = 'chr1\tt\texon\t101\t200\t.\t+\t.\ttranscript_id "a";\n'
    open(path, "w").write("# head\n" + good + 'chr1\tt\texon\t300\t299\t.\t+\t.\ttranscript_id "a";\n')
    assert _run(exe, path)[4].startswith("line 3: ")
    open(path, "w").write(good + 'chr1\tt\texon\t300\t400\t.\t+\t.\tgene_id "g";\n')
    err = _run(exe, path)[4]
    assert err.startswith("line 2: ") and "transcript_id" in err
    open(path, "w").write("# nothing\nchrUn\tt\texon\t1\t5\t.\t+\t.\ttranscript_id \"a\";\n")
    assert "no transcript" in _run(exe, path)[4]
    assert "cannot read" in _run(exe, os.path.join(workdir, "tx_missing.gtf"))[4]
