"""CPU suite: the readers of the device's 2-bit text in their two forms -- pac holding both strands (what every kernel is launched with: the reverse complement is
built once, by k_pac_both's per-byte rule) against pac holding the forward half only (the form that computes the reverse complement per access) -- compiled for the
host and run as a stand-alone program (tests/native/pac_both_checks.hip): d_refchar, d_ref8, d_ref_codes, both mismatches8 and the seeding stage's 64-symbol window,
for every position from 70 in front of the text to 70 behind it, every window length, and texts of every length modulo 4."""
import os
import re
import shutil
import subprocess

import pytest

import common


def _counts(stdout, name):
    line = [l for l in stdout.splitlines() if l.startswith(name + ":")][0]
    return {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", line.split(":", 1)[1])}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_text_readers_agree_with_and_without_the_second_strand(workdir):
    """both forms give the same characters, codes, mismatch counts and windows; the second half built by the library's rule is the text's definition; and the windows that
    matter occurred: across the strand boundary, over either end of the text, wholly inside each half"""
    src = os.path.join(common.ROOT, "tests", "native", "pac_both_checks.hip")
    exe = os.path.join(workdir, "pac_both_checks")
    subprocess.run(["hipcc", "-O2", "--offload-arch=gfx950", "-std=c++17", "-w", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("bad=0"), r.stdout[-3000:] + r.stderr[-3000:]
    for name in ("windows8", "windows1to28", "windows64"):
        c = _counts(r.stdout, name)
        for k in ("straddle_L", "at_begin", "at_end", "first_half", "second_half", "outside"):
            assert c[k] > 0, (name, c)
    first = r.stdout.splitlines()[0]
    n_new = int(first.rsplit(" ", 1)[1])
    assert n_new > 0, first            # windows d_ref_codes fetches at once only now: those across the strand boundary
