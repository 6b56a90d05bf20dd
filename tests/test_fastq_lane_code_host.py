"""CPU suite: the record rules of the device's FASTQ parser (dart_amd/csrc/dg_fastq.h: newlines 16 bytes at a time, a record's name, read and quality from
the lengths of its four lines, the stored form of an odd read) compiled for the host (tests/native/fastq_checks.hip) and walked over an awkward FASTQ text:
names, stored bases and stored qualities must be those of a Python restatement of the reference's reader (GetNextEntry / GetNextChunk, GetData.cpp:55-179;
tests/fastq_device_inputs.py)."""
import os
import pytest
import fastq_device_inputs as fdi


@pytest.fixture(scope="module")
def texts():
    m1, m2 = fdi.random_reads(23, seed=5), fdi.random_reads(23, seed=6)
    return fdi.awkward_texts(m1, m2)


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)


@pytest.mark.parametrize("layout", ["two_files_paired", "interleaved_paired", "one_file_single", "two_files_single"])
def test_lane_code_parses_the_awkward_text_as_the_reference_reader(layout, texts, workdir):
    t1, t2, inter = texts
    exe = fdi.build_checks_program(workdir)
    a, b = (inter, None) if layout == "interleaved_paired" else (t1, None) if layout == "one_file_single" else (t1, t2)
    paired = layout.endswith("paired")
    st, got = fdi.run_checks_program(exe, os.path.join(workdir, "fq_%s.bin" % layout), a, b, paired)
    want = fdi.reference_reads(a, b, paired)
    assert st == 0
    _same(got, want)
    # what the text is there for occurs (asserted, not assumed)
    names = [h for h, s, q in got]; lens = [len(s) for h, s, q in got]
    assert 1 in lens and 1000 in lens and any(len(h) == 5000 for h in names) and b"" in names
    assert any(len(q) < len(s) for h, s, q in got) and any(b"\0" in q for h, s, q in got) and any(len(q) == len(s) and len(s) == 101 for h, s, q in got)
    assert any(h.endswith(b"\r") and s.endswith(b"\r") and q.endswith(b"\r") for h, s, q in (got[0::2] if paired else got))      # CRLF: the '\r' belongs to the name, the read and the quality
    assert any(s[:1].islower() for h, s, q in got) and any(b"R" in s for h, s, q in got) and any(q[:1] in b"@+" for h, s, q in got)
    assert not a.endswith(b"\n")
    if paired:      # an odd read is the reverse complement of its line, lower case and IUPAC through comp_base
        assert any(b"N" in s for k, (h, s, q) in enumerate(got) if k & 1) and not any(c in s for k, (h, s, q) in enumerate(got) if k & 1 for c in (b"a", b"c", b"g", b"t"))


def test_lane_code_counts_of_two_texts_and_partial_records(workdir):
    """two texts: equal record counts or one more in the first, else an error; a record whose lines are missing has no bases; no text, no reads"""
    exe = fdi.build_checks_program(workdir)
    r = lambda i: ("@x%d\nACGT\n+\nIIII\n" % i).encode()
    p = os.path.join(workdir, "fq_counts.bin")
    assert fdi.run_checks_program(exe, p, r(0) + r(1), r(2) + r(3), True)[0] == 0
    st, got = fdi.run_checks_program(exe, p, r(0) + r(1) + r(4), r(2) + r(3), True)
    assert st == 0 and [h for h, s, q in got] == [b"x0", b"x2", b"x1", b"x3", b"x4"] and got[1][1] == b"ACGT" and got[3][2] == b"IIII"
    assert fdi.run_checks_program(exe, p, r(0), r(2) + r(3), True)[0] == -1
    assert fdi.run_checks_program(exe, p, r(0) + r(1) + r(4), r(2), True)[0] == -1
    st, got = fdi.run_checks_program(exe, p, r(0) + b"@cut\nAC", None, False)            # the last line without newline loses its last byte, as getline - 1 does
    assert st == 0 and got[1] == (b"cut", b"A", b"")
    st, got = fdi.run_checks_program(exe, p, r(0) + b"@gone\n", None, False)
    assert st == 0 and len(got) == 2 and got[1][1] is None
    st, got = fdi.run_checks_program(exe, p, r(0) + b"@empty\n\n+\n\n" + r(1), None, False)
    assert st == 0 and len(got) == 3 and got[1][1] is None and got[2][0] == b"x1"
    assert fdi.run_checks_program(exe, p, b"", None, False) == (0, [])
    # a newline at every place of a 16-byte group, and text lengths around it
    for n in range(1, 40):
        t = b"@h\n" + b"A" * n + b"\n+\n" + b"I" * n + b"\n"
        for cut in (0, 1):
            st, got = fdi.run_checks_program(exe, p, t[:len(t) - cut], None, False)
            assert st == 0 and got == [(b"h", b"A" * n, b"I" * n)], (n, cut)
