"""CPU suite: the DART_MARKDUP_UMI and DART_UMI switches as `dart` reads them once into Config (dart_amd/csrc/host/dart_config.h) -- exact and edit1, the separator and its
default, the values that end the run and are named, the refusal without DART_MARK_DUPLICATES=1; the inline cut's lengths, linker and separator, and its refusal without the device parser or a device formatter (tests/native/dart_config_umi_checks.cpp).  The program stands alone (its own main, no libdartgpu, no Python in the process), so
the second build runs under the address and undefined-behaviour sanitizers as it is."""
import os, subprocess
import pytest
import common


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_dart_config_markdup_umi_switches(sanitize, workdir):
    src = os.path.join(common.ROOT, "tests", "native", "dart_config_umi_checks.cpp")
    d = os.path.join(workdir, "dart_config_umi_san" if sanitize else "dart_config_umi"); os.makedirs(d, exist_ok=True)
    exe = os.path.join(d, "dart_config_umi_checks")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run(["g++"] + flags + ["-std=c++17", "-I", os.path.join(common.ROOT, "include"), "-I", os.path.join(common.ROOT, "dart_amd", "csrc", "host"),
                    "-o", exe, src, "-lz"], check=True)
    out = subprocess.run([exe, d], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("bad=0"), out.stdout[-3000:] + out.stderr[-3000:]
