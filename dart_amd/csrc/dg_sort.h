// dart_amd/csrc/dg_sort.h -- stable LSD radix sort of (u64 key, i64 value) pairs in HBM: the sorter of the index builder.
//
// Replaces the sorting inside the reference's offline indexer (BWT_Index/bwtindex.c:77-148 -> bwt_gen.c / QSufSort.c: suffix
// sorting of the 2-bit text) for texts the GPU box has to index itself: dart_amd/index_build.py does prefix
// doubling, and every round is one sort of (rank pair, suffix) -- up to 386 M pairs per bucket of a GRCh38-sized text.
//
// 4 bits per pass, least significant digit first, tiles of 4096 pairs (256 lanes x 16):
//   k_rs_hist     per tile, how many keys fall in each of the 16 bins (bin-major table, so one scan gives every tile its bases)
//   rs_scan_u32   exclusive scan of the 16 x tiles table: k_scan_tiles, k_tiles_top (dg_wgscan.h), k_scan_add
//   k_rs_scatter  per tile: coalesced load into LDS; every lane takes 16 CONSECUTIVE pairs (stability = order by lane, then item),
//                 counts them per bin in its own LDS column; one scan over the 16 x 256 counts (bin-major) gives every lane its
//                 start in every bin; the pairs are put in tile-sorted order in LDS and leave with coalesced stores, each run of a
//                 bin going to  base[bin][tile] + (position - start of the bin in the tile)
// rs_sort_passes enqueues the five launches of every pass: the one driver of every sort, in the library (api_ctx.h's SortBufs, dg_sort_pairs) and in the
// index builder (index/dg_index.hip).
// HBM-bound: 8 + 32 bytes per pair and pass.  No MFMA anywhere (integer keys).
#pragma once
#include "dg_wgscan.h"

#define RS_TILE 4096
#define RS_PAD(i) ((i) + ((i) >> 4))            // one slot of padding per 16: a lane's 16 consecutive pairs do not all hit one bank

__global__ void __launch_bounds__(256)
k_rs_hist(const uint64_t *__restrict__ keys, uint32_t n, int shift, uint32_t n_tiles, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t lh[4][16];
    if (threadIdx.x < 64) lh[threadIdx.x >> 4][threadIdx.x & 15] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * RS_TILE, wv = threadIdx.x >> 6;
#pragma unroll 4
    for (int j = 0; j < 16; j++) {
        const uint32_t i = base + (uint32_t)j * 256u + threadIdx.x;
        if (i < n) atomicAdd(&lh[wv][(keys[i] >> shift) & 15u], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 16) hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = lh[0][threadIdx.x] + lh[1][threadIdx.x] + lh[2][threadIdx.x] + lh[3][threadIdx.x];
}

__global__ void __launch_bounds__(256)
k_rs_scatter(const uint64_t *__restrict__ keys, const int64_t *__restrict__ vals, uint64_t *__restrict__ keys_out, int64_t *__restrict__ vals_out,
             uint32_t n, int shift, uint32_t n_tiles, const uint32_t *__restrict__ bases)
{
    __shared__ uint64_t sk[RS_PAD(RS_TILE) + 1];
    __shared__ int64_t sv[RS_PAD(RS_TILE) + 1];
    __shared__ uint16_t cnt[16 * 256];
    __shared__ uint32_t s_wave[4], bstart[16], gbase[16];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * RS_TILE;
    const uint32_t n_valid = n - base < RS_TILE ? n - base : RS_TILE;
    // 1. coalesced load (pairs past the end: largest key, so they stay last in the tile's order and are never stored)
#pragma unroll 4
    for (int j = 0; j < 16; j++) {
        const uint32_t li = (uint32_t)j * 256u + tid, i = base + li;
        sk[RS_PAD(li)] = i < n ? keys[i] : ~0ull;
        sv[RS_PAD(li)] = i < n ? vals[i] : 0;
    }
    if (tid < 16) gbase[tid] = bases[(size_t)tid * n_tiles + blockIdx.x];
#pragma unroll
    for (int b = 0; b < 16; b++) cnt[b * 256 + tid] = 0;
    __syncthreads();
    // 2. this lane's 16 consecutive pairs, counted per bin in its own column
    uint64_t k[16]; int64_t v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t li = tid * 16u + (uint32_t)j;
        k[j] = sk[RS_PAD(li)]; v[j] = sv[RS_PAD(li)];
        const uint32_t d = li < n_valid ? (uint32_t)(k[j] >> shift) & 15u : 15u;
        cnt[d * 256 + tid]++;
    }
    __syncthreads();
    // 3. exclusive scan of the 4096 counts in bin-major order: lane t owns entries [16 t, 16 t + 16)
    uint32_t c[16], mine = 0;
#pragma unroll
    for (int q = 0; q < 16; q++) { c[q] = cnt[tid * 16 + q]; mine += c[q]; }
    uint32_t all;
    uint32_t run = d_wg_exclusive<uint32_t>(mine, all, s_wave);
    if ((tid & 15u) == 0) bstart[tid >> 4] = run;              // entry (bin, lane 0): where the bin starts in the sorted tile
#pragma unroll
    for (int q = 0; q < 16; q++) { cnt[tid * 16 + q] = (uint16_t)run; run += c[q]; }
    __syncthreads();
    // 4. the pairs in tile-sorted order
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t li = tid * 16u + (uint32_t)j;
        const uint32_t d = li < n_valid ? (uint32_t)(k[j] >> shift) & 15u : 15u;
        const uint32_t p = cnt[d * 256 + tid]++;
        sk[RS_PAD(p)] = k[j]; sv[RS_PAD(p)] = v[j];
    }
    __syncthreads();
    // 5. coalesced stores
#pragma unroll 4
    for (int j = 0; j < 16; j++) {
        const uint32_t p = (uint32_t)j * 256u + tid;
        if (p < n_valid) {
            const uint64_t key = sk[RS_PAD(p)];
            const uint32_t d = (uint32_t)(key >> shift) & 15u;
            const uint32_t dst = gbase[d] + (p - bstart[d]);
            keys_out[dst] = key; vals_out[dst] = sv[RS_PAD(p)];
        }
    }
}

// ------------------------------------------------------------------------------------------
// exclusive scan of n u32 in three launches: tiles of SCAN_TILE, k_tiles_top over their sums, the sums added back
// ------------------------------------------------------------------------------------------
#define SCAN_TILE 2048
__global__ void __launch_bounds__(256) k_scan_tiles(const uint32_t *in, uint32_t *out, uint32_t *tile_sums, uint32_t n)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * 8;
    uint32_t v[8], sum = 0;
    for (int i = 0; i < 8; i++) { v[i] = base + i < n ? in[base + i] : 0; sum += v[i]; }
    uint32_t all;
    uint32_t run = d_wg_exclusive<uint32_t>(sum, all, s_wave);
    for (int i = 0; i < 8; i++) { if (base + i < n) out[base + i] = run; run += v[i]; }
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = all;
}
__global__ void __launch_bounds__(256) k_scan_add(uint32_t *out, const uint32_t *tile_sums, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] += tile_sums[i / SCAN_TILE];
}
// in == out is allowed; sums holds one word per SCAN_TILE of n; *total (device memory) = the sum of all
static inline void rs_scan_u32(hipStream_t s, const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *sums, uint32_t *total)
{
    const uint32_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    k_scan_tiles<<<tiles, 256, 0, s>>>(in, out, sums, n);
    k_tiles_top<uint32_t><<<1, 256, 0, s>>>(sums, tiles, total);
    k_scan_add<<<(n + 255) / 256, 256, 0, s>>>(out, sums, n);
}

// The passes of the sort of n pairs by the low `bits` bits of the key, enqueued on stream s.  keys / vals: two buffers each; which: in = the pair that holds
// the input, out = the one that holds the result.
// hist holds rs_hist_words(n) words (16 x tiles + 1), sums rs_sums_words(n) (one per SCAN_TILE of them + 1): the caller's scratch.
static inline size_t rs_hist_words(uint32_t n) { return 16 * (size_t)((n + RS_TILE - 1) / RS_TILE) + 1; }
static inline size_t rs_sums_words(uint32_t n) { return (rs_hist_words(n) - 1 + SCAN_TILE - 1) / SCAN_TILE + 1; }
static inline hipError_t rs_sort_passes(hipStream_t s, uint64_t *const keys[2], int64_t *const vals[2], uint32_t *hist, uint32_t *sums, uint32_t n, int bits, int &which)
{
    const uint32_t tiles = (n + RS_TILE - 1) / RS_TILE, m = 16u * tiles;
    for (int shift = 0; shift < bits; shift += 4) {
        const int o = which ^ 1;
        k_rs_hist<<<tiles, 256, 0, s>>>(keys[which], n, shift, tiles, hist);
        rs_scan_u32(s, hist, hist, m, sums, hist + m);
        k_rs_scatter<<<tiles, 256, 0, s>>>(keys[which], vals[which], keys[o], vals[o], n, shift, tiles, hist);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        which = o;
    }
    return hipSuccess;
}
