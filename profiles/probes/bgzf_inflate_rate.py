"""Rate of the device's BGZF inflater (dg_bgzf_inflate: k_bgzf_inflate, one wave per block) against the host's inflaters on the same bytes: FASTQ-like text of
16 MiB and 128 MiB, once as zlib level 6 blocks (what bgzip writes) and once as the device's own dynamic blocks (dg_bgzf_compress_flags, DG_BGZF_DYNAMIC).
For each: device_ms of the kernel, warm, median of --runs; libdeflate on one thread where the machine has it; zlib.decompress member by member.  A tool, not a
test.  The host-to-device copy of the compressed bytes is outside the timed events.

    python profiles/probes/bgzf_inflate_rate.py [--runs 10] [--warmup 2] [--mib 16 128] [--out FILE]
"""
import argparse, ctypes as C, ctypes.util, json, os, statistics, sys, tempfile, time, zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from dart_amd import host, index_build, synth

BLOCK = 0xff00


def fastq_like(n_bytes, seed=1):
    """records of 2x101's shape: '@read<9 digits>/1', 101 bases, '+', 101 qualities"""
    rng = np.random.default_rng(seed)
    rec = 16 + 1 + 101 + 1 + 2 + 101 + 1
    n = n_bytes // rec + 1
    a = np.empty((n, rec), np.uint8)
    a[:, :5] = np.frombuffer(b"@read", np.uint8)
    idx = np.arange(n)
    for k in range(9):
        a[:, 5 + k] = 48 + (idx // 10 ** (8 - k)) % 10
    a[:, 14:16] = np.frombuffer(b"/1", np.uint8); a[:, 16] = 10
    a[:, 17:118] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, 101))]; a[:, 118] = 10
    a[:, 119] = 43; a[:, 120] = 10
    a[:, 121:222] = 33 + np.minimum(40, rng.integers(25, 60, (n, 101))); a[:, 222] = 10
    return a.tobytes()[:n_bytes]


def zlib_blocks(data, level=6):
    out = []
    for at in range(0, len(data), BLOCK):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
        raw = c.compress(data[at:at + BLOCK]) + c.flush()
        total = 18 + len(raw) + 8
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + (total - 1).to_bytes(2, "little") + raw +
                   zlib.crc32(data[at:at + BLOCK]).to_bytes(4, "little") + len(data[at:at + BLOCK]).to_bytes(4, "little"))
    return b"".join(out)


def members(blocks):
    at = 0
    while at < len(blocks):
        n = int.from_bytes(blocks[at + 16:at + 18], "little") + 1
        yield at, n
        at += n


def time_zlib(blocks, runs):
    times = []
    for _ in range(runs):
        t = time.perf_counter()
        total = 0
        for at, n in members(blocks):
            total += len(zlib.decompress(blocks[at + 18:at + n - 8], -15))
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), total


def time_libdeflate(blocks, n_out, runs):
    name = ctypes.util.find_library("deflate")
    if not name:
        return None
    ld = C.CDLL(name)
    ld.libdeflate_alloc_decompressor.restype = C.c_void_p
    ld.libdeflate_deflate_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    d = ld.libdeflate_alloc_decompressor()
    src = np.frombuffer(blocks, np.uint8); dst = np.zeros(n_out + 65536, np.uint8)
    ms = list(members(blocks))
    times = []
    for _ in range(runs):
        t = time.perf_counter()
        o = 0
        for at, n in ms:
            got = C.c_size_t(0)
            if ld.libdeflate_deflate_decompress(d, src.ctypes.data + at + 18, n - 26, dst.ctypes.data + o, 65536, C.byref(got)) != 0:
                raise RuntimeError("libdeflate refused a block")
            o += got.value
        times.append((time.perf_counter() - t) * 1e3)
    ld.libdeflate_free_decompressor.argtypes = [C.c_void_p]; ld.libdeflate_free_decompressor(d)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mib", type=int, nargs="+", default=[16, 128]); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = tempfile.mkdtemp()
    g = synth.make_genome([60000], seed=3)
    index_build.build_index_from_genome(g, d + "/idx")
    gpu = host.DartGPU(host.Index(d + "/idx"))
    rows = []
    for mib in a.mib:
        text = fastq_like(mib << 20)
        for coder, blocks in (("zlib level 6", zlib_blocks(text)), ("device dynamic", gpu.bgzf_compress(text, dynamic=True))):
            src = np.frombuffer(blocks, np.uint8)
            nb = C.c_size_t(0); nk = C.c_size_t(0); ms = C.c_float(0)
            times = []
            for k in range(a.warmup + a.runs):
                rc = gpu.lib.dg_bgzf_inflate(gpu.ctx, src.ctypes.data, len(blocks), C.byref(nb), C.byref(nk), C.byref(ms))
                if rc:
                    raise RuntimeError((gpu.lib.dg_last_error(gpu.ctx) or b"").decode())
                if k >= a.warmup:
                    times.append(float(ms.value))
            same = gpu.bgzf_inflate(blocks) == text
            med = statistics.median(times)
            z_ms, z_total = time_zlib(blocks, 3)
            ld_ms = time_libdeflate(blocks, len(text), 3)
            rows.append({"text_MiB": mib, "blocks_from": coder, "blocks": int(nk.value), "compressed_bytes": len(blocks), "runs": a.runs,
                         "device_ms_median": round(med, 3), "device_ms_min": round(min(times), 3), "device_ms_max": round(max(times), 3),
                         "device_GBps_of_text": round(len(text) / (med * 1e-3) / 1e9, 2),
                         "libdeflate_1_thread_ms": None if ld_ms is None else round(ld_ms, 1), "libdeflate_GBps_of_text": None if ld_ms is None else round(len(text) / (ld_ms * 1e-3) / 1e9, 2),
                         "zlib_decompress_ms": round(z_ms, 1), "zlib_GBps_of_text": round(len(text) / (z_ms * 1e-3) / 1e9, 2), "bytes_equal_the_text": bool(same and z_total == len(text))})
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("".join(json.dumps(r) + "\n" for r in rows))
    gpu.close()


if __name__ == "__main__":
    main()
