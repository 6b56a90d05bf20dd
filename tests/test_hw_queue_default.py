"""The hardware queues libdartgpu.so asks the HIP runtime for (GPU_MAX_HW_QUEUES, decided by the library's load-time constructor:
dart_amd/csrc/dg_api.hip, dg_default_hw_queues).  A value that is missing, unparsable or lower than the library's need (16) becomes
16; a higher one stays.  Every case runs in a fresh child process that only loads the library (no dg_init, no device needed) and
asks the C library -- not os.environ, which Python fills once at start-up -- what the variable holds afterwards."""
import os
import re
import subprocess
import sys
import pytest
import common
from dart_amd import host

CHILD = r"""
import ctypes, sys
try:
    ctypes.CDLL(sys.argv[1])
except OSError as e:
    print("LOADFAIL", e); sys.exit(0)
libc = ctypes.CDLL(None)
libc.getenv.restype = ctypes.c_char_p
libc.getenv.argtypes = [ctypes.c_char_p]
v = libc.getenv(b"GPU_MAX_HW_QUEUES")
print("VALUE", v.decode() if v is not None else "unset")
"""


def value_after_load(preset):
    import __graft_entry__ as ge
    ge.build()
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    if preset is not None:
        env["GPU_MAX_HW_QUEUES"] = preset
    r = subprocess.run([sys.executable, "-c", CHILD, host.LIB_PATH], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    if "LOADFAIL" in r.stdout:
        pytest.skip("libdartgpu.so does not load here: " + r.stdout.strip())
    return r.stdout.split("VALUE", 1)[1].strip()


@pytest.mark.parametrize("preset, want", [(None, "16"), ("4", "16"), ("24", "24"), ("abc", "16")])
def test_constructor_raises_a_low_queue_count_and_keeps_a_higher_one(preset, want):
    assert value_after_load(preset) == want


@pytest.mark.parametrize("preset, want", [("", "16"), ("0", "16"), ("15", "16"), ("16", "16"), ("17", "17"), ("16x", "16"), ("-3", "16")])
def test_constructor_edge_values(preset, want):
    assert value_after_load(preset) == want


def test_sources_never_ask_for_more_than_32_queues():
    """the named constants of the library and of `dart`: one value, 16, within the 32 the runtime is ever asked for"""
    lib_src = open(os.path.join(common.ROOT, "dart_amd", "csrc", "dg_api.hip")).read()
    main_src = open(os.path.join(common.ROOT, "dart_amd", "csrc", "host", "dart_main.cpp")).read()
    a = re.search(r"#define DG_HW_QUEUES_NEED (\d+)", lib_src)
    b = re.search(r"HW_QUEUES_NEED = (\d+);", main_src)
    assert a and b and int(a.group(1)) == int(b.group(1)) == 16
    for src in (lib_src, main_src):
        assert not re.search(r'setenv\("GPU_MAX_HW_QUEUES", "\d+"', src)          # (only through the constant)


@pytest.mark.gpu
def test_gpu_init_report_ends_with_the_queue_fields(workdir):
    """dg_init_report: the start-up split, then what the constructor found and what it left -- always the last two fields"""
    c = common.build_case("se100", workdir)
    gpu = host.DartGPU(host.Index(c["prefix"]))
    try:
        rep = gpu.init_report()
    finally:
        gpu.close()
    m = re.search(r"; hw_queues_env_found=(\S+) hw_queues_env_set=(\d+)$", rep)
    assert m and "k_build_ktab" in rep[:m.start()], rep
    assert int(m.group(2)) >= 16 and (m.group(1) == "unset" or not m.group(1).isdigit() or int(m.group(2)) == max(16, int(m.group(1)))), rep


@pytest.mark.gpu
@pytest.mark.parametrize("preset, want", [("4", 16), ("24", 24)])
def test_gpu_dart_start_up_line_reports_the_queue_count(preset, want, workdir):
    """`dart` under DART_TIMING=1: its start-up line carries dg_init_report, so the queue count the run really asked for"""
    from dart_amd import synth
    import __graft_entry__ as ge
    ge.build()
    c = common.build_case("se100", workdir)
    d = os.path.join(workdir, "hwq_" + preset); os.makedirs(d, exist_ok=True)
    synth.write_fastq(os.path.join(d, "1.fq"), c["m1"], 1)
    env = dict(os.environ, GPU_MAX_HW_QUEUES=preset, DART_TIMING="1")
    r = subprocess.run([os.path.join(common.ROOT, "dart_amd", "dart"), "-i", c["prefix"], "-f", "1.fq", "-o", "o.sam", "-j", "o.j", "-t", "4"],
                       cwd=d, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-600:]
    m = re.search(r"\[dart timing\] start-up .*hw_queues_env_found=(\S+) hw_queues_env_set=(\d+)\)", r.stderr)
    assert m and m.group(1) == preset and int(m.group(2)) == want, r.stderr[-800:]
