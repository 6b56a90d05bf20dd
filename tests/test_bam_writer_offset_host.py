"""CPU suite: the host BAM writer's first_block_offset (what `dart` hands to dg_bam_index_finish) is the number of bytes the header's blocks took, on a
regular file and on a pipe alike -- the writer never seeks, so `-bo /dev/stdout | ...` keeps working."""
import os, subprocess
import pytest
import common, bam_decode


@pytest.fixture(scope="module")
def exe(workdir):
    out = os.path.join(workdir, "bam_writer_offset_checks")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(common.ROOT, "dart_amd", "csrc", "host"), "-o", out,
                           os.path.join(common.ROOT, "tests", "native", "bam_writer_offset_checks.cpp"), "-lz", "-ldl"])
    return out


def _header_bytes(bam):
    """the compressed bytes of the blocks in front of the first record's block, from the file alone"""
    blocks = bam_decode.bgzf_blocks(bam)
    hdr, refs, lines, _ = bam_decode.decode(bam)             # (asserts that the header ends on a block boundary)
    assert len(lines) == 1 and len(refs) == 2
    n_records_blocks = 1
    return sum(s for _, s in blocks[:-1 - n_records_blocks]), len(blocks)


def test_offset_on_a_regular_file_and_on_a_pipe(exe, workdir):
    path = os.path.join(workdir, "writer_offset.bam")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want, n_blocks = _header_bytes(open(path, "rb").read())
    assert n_blocks >= 4 and r.stderr.split() == ["ok", "1", "first", str(want)]
    # the same through a pipe: nothing can be sought there
    p = subprocess.run([exe, "/dev/stdout"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr
    assert p.stdout == open(path, "rb").read() and p.stderr.decode().split() == ["ok", "1", "first", str(want)]
