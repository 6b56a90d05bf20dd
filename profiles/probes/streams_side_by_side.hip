// How many streams of this process really run side by side?  The HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues, read
// when it initialises; streams that share a queue run their kernels one after the other.  N streams, on each a chain of CHAIN one-wave
// kernels that spin for SPIN_US on the wall clock and touch no memory: wall time of one chain alone x N / wall time of all N chains
// together = chains that ran side by side.  A self-check of a few hundred short, finite kernels: well under 2 s.
//   hipcc -O2 --offload-arch=gfx950 -o /tmp/streams_side_by_side profiles/probes/streams_side_by_side.hip -ldl
//   timeout -k 10 60 /tmp/streams_side_by_side [--lib dart_amd/libdartgpu.so] [N ...]        (default N: 4 8 14)
// --lib: dlopen that library before the first HIP call, as a host of libdartgpu does: its load-time constructor then decides the variable.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

enum { CHAIN = 20, SPIN_US = 200, MAX_STREAMS = 32 };

// one wave; ends after `ticks` of the constant-rate wall clock, or after `max_polls` looks at it, whichever comes first
__global__ void __launch_bounds__(64) k_spin(long long ticks, int max_polls)
{
    const long long t0 = wall_clock64();
    for (int i = 0; i < max_polls && wall_clock64() - t0 < ticks; i++) __builtin_amdgcn_s_sleep(16);
}

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char **argv)
{
    std::vector<int> ns;
    const char *env0 = getenv("GPU_MAX_HW_QUEUES");
    printf("GPU_MAX_HW_QUEUES at process start: %s\n", env0 ? env0 : "unset");
    for (int i = 1; i < argc; i++) {
        if (strcmp(argv[i], "--lib") == 0 && i + 1 < argc) {
            if (!dlopen(argv[++i], RTLD_NOW | RTLD_GLOBAL)) { fprintf(stderr, "dlopen %s: %s\n", argv[i], dlerror()); return 1; }
            const char *v = getenv("GPU_MAX_HW_QUEUES");
            printf("loaded %s before the first HIP call; GPU_MAX_HW_QUEUES now: %s\n", argv[i], v ? v : "unset");
        } else if (atoi(argv[i]) >= 1 && atoi(argv[i]) <= MAX_STREAMS) ns.push_back(atoi(argv[i]));
        else { fprintf(stderr, "usage: %s [--lib libdartgpu.so] [N <= %d ...]\n", argv[0], MAX_STREAMS); return 1; }
    }
    if (ns.empty()) ns = {4, 8, 14};
    int khz = 0;
    CHK(hipSetDevice(0));
    CHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0));
    if (khz <= 0) khz = 100000;
    const long long ticks = (long long)khz * SPIN_US / 1000;
    const int max_polls = 20000;                                   // (a poll sleeps >= 1024 cycles: a bound far above SPIN_US, there only to make the loop finite)
    const int n_max = *std::max_element(ns.begin(), ns.end());
    std::vector<hipStream_t> st(n_max);
    for (auto &s : st) CHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    auto chains = [&](int n) {                                     // n chains at once; wall seconds, best of three
        double best = 1e9;
        for (int rep = 0; rep < 4; rep++) {                        // (the first round warms up)
            CHK(hipDeviceSynchronize());
            const double t = now();
            for (int k = 0; k < CHAIN; k++) for (int i = 0; i < n; i++) k_spin<<<1, 64, 0, st[i]>>>(ticks, max_polls);
            CHK(hipGetLastError());
            for (int i = 0; i < n; i++) CHK(hipStreamSynchronize(st[i]));
            if (rep) best = std::min(best, now() - t);
        }
        return best;
    };
    const double one = chains(1);
    printf("wall clock %d kHz; a chain = %d kernels of %d us; one chain alone: %.3f ms\n", khz, (int)CHAIN, (int)SPIN_US, one * 1e3);
    for (int n : ns) {
        const double t = chains(n);
        printf("%2d streams: %.3f ms together -> %.1f chains side by side\n", n, t * 1e3, n * one / t);
    }
    for (auto &s : st) CHK(hipStreamDestroy(s));
    return 0;
}
