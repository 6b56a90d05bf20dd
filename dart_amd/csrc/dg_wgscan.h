// dg_wgscan.h -- the sums every output stage shares: a lane counts, the workgroup scans, one workgroup scans the workgroups' sums, the lanes write.
//   d_wave_sum / d_wave_max   the wave's 64 values summed / their maximum, in every lane
//   d_wg_exclusive            exclusive sum over the 256 lanes of a workgroup, and the workgroup's sum
//   d_tiles_exclusive         one workgroup: any number of workgroup sums scanned in place, 256 at a time with a carry
//   k_tiles_top<T>            the kernel that is nothing but that loop: <<<1, 256>>>, *total = the sum of all
// Sums only: a scan with another operator (a running maximum, a last-valid fill) stays with its stage.  The mapping path's single-pass look-back scan is
// dg_scan.h.  Nothing of the library is included, so the index builder (index/dg_index.hip) uses the same code.
#ifndef DG_WGSCAN_H
#define DG_WGSCAN_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef __HIPCC__
#define WG_THREADS 256

template <class T> __device__ __forceinline__ T d_wave_sum(T v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
template <class T> __device__ __forceinline__ T d_wave_max(T v) { for (int o = 32; o > 0; o >>= 1) { const T u = __shfl_xor(v, o, 64); v = u > v ? u : v; } return v; }

// Exclusive sum of `mine` over the workgroup's WG_THREADS lanes in thread order; total = the workgroup's sum, in every lane.  T is uint32_t or a 64-bit
// unsigned type; s_wave is WG_THREADS / 64 words of LDS.  The contract:
//   - ALL lanes of the workgroup call it (there are two barriers inside): a return in front of the call is taken by the whole workgroup or by no lane.
//   - It may be called any number of times running with the same s_wave.  The first barrier is the one that lets the previous call's readers of s_wave
//     finish before this call writes it: the scan owns that barrier, and no caller adds one for s_wave's sake.
//   - Whatever the workgroup wrote to LDS before the call is visible behind it.
template <class T>
__device__ __forceinline__ T d_wg_exclusive(T mine, T &total, T *s_wave)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    T incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const T up = __shfl_up(incl, o, 64); if (lane >= (uint32_t)o) incl += up; }
    __syncthreads();
    if (lane == 63u) s_wave[wv] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < WG_THREADS / 64; w++) { const T s = s_wave[w]; if (w < wv) before += s; all += s; }
    total = all;
    return before + incl - mine;
}

// One workgroup: tile_sum[i * stride], i < n_tiles, becomes the sum of the entries in front of it; returns the sum of all, in every lane.
template <class T>
__device__ __forceinline__ T d_tiles_exclusive(T *tile_sum, uint32_t n_tiles, size_t stride, T *s_wave)
{
    T carry = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += WG_THREADS) {
        const uint32_t i = t0 + threadIdx.x;
        T all;
        const T ex = d_wg_exclusive<T>(i < n_tiles ? tile_sum[i * stride] : (T)0, all, s_wave);
        if (i < n_tiles) tile_sum[i * stride] = carry + ex;
        carry += all;
    }
    return carry;
}

template <class T>
__global__ void __launch_bounds__(WG_THREADS)
k_tiles_top(T *__restrict__ tile_sum, uint32_t n_tiles, T *__restrict__ total)
{
    __shared__ T s_wave[WG_THREADS / 64];
    const T all = d_tiles_exclusive<T>(tile_sum, n_tiles, 1, s_wave);
    if (threadIdx.x == 0) *total = all;
}
#endif
#endif
