// dg_bamsort.h -- coordinate-sorted BAM on the device: the uncompressed records of every batch stay in HBM (a store per context: the records' bytes, and per
// record one 64-bit key and its byte offset in the store), and at the end of the job one stable radix sort (dg_sort.h) and one gather leave all records in
// one contiguous array in coordinate order, which dg_bgzf.h then compresses piece by piece.  The reference has no such output: an opt-in extension.
//
// The order is defined by a record's own fields (bam_head of dg_bamrec.h reads them):
//   tid' = refID when 0 <= refID < n_chr, else n_chr: unplaced records come last
//   key  = tid' << 33 | (uint32)(pos + 1) << 1 | (flag >> 4 & 1)
//   ascending key; equal keys keep their input order: ascending batch ordinal, then the record's place in its batch
// That is the comparison `samtools sort` makes by default (tid as unsigned, pos, reverse strand, stable).  No samtools exists where this project is built
// and tested: the definition above -- not a run of samtools -- is what the tests pin.
//
//   k_bs_count   lane = read: walks the block_size fields inside the read's byte range of the batch's record array (k_bam_len's scanned offsets) and counts
//                its records (0 to several: a refused line left none); every workgroup leaves the exclusive scan of its 256 counts and their sum
//   (scan)       k_tiles_top over the workgroup sums
//   k_bs_emit    lane = read: the same walk; record i of the batch gets its key and its offset in the store
//   k_bs_shift   lane = record: offsets of another context's store, moved behind this one's bytes (dg_bam_sort_merge)
//   k_bs_len     lane = sorted record: its bytes (block_size + 4); the workgroup's exclusive scan and sum (64 bit)
//   k_bs_gather  wave = record: the record's bytes to their place in the sorted array.  The destination is brought to a dword boundary with single bytes,
//                then every lane stores one aligned dword per trip, funnel-shifted from two aligned dwords of the (differently aligned) source; the last
//                0..3 bytes go singly.  One trip moves 256 bytes: a record of 2x101 reads leaves in one.
// Every record's place follows from the keys and the scanned lengths alone, so the array is the same whatever the grid, the batch split, the contexts used
// or the growth history of the store.  The key, the two walks with their checks and the segment order are host-callable (tests/native/bamsort_checks.hip).
#ifndef DG_BAMSORT_H
#define DG_BAMSORT_H
#include "dg_bamrec.h"
#include "dg_sort.h"
#include "dg_wgscan.h"
#include <algorithm>

#define BS_HD __host__ __device__ __forceinline__
// BS_THREADS (dg_bamrec.h) is also the reads per workgroup of k_bs_count / k_bs_emit
#define BS_MIN_BYTES 4096        // the smallest store (dg_bam_sort_granules [2])
#define BS_GATHER_WAVES 4        // records per workgroup of k_bs_gather
static_assert(BS_THREADS == SAM_LEN_THREADS, "k_bs_count reads k_bam_len's per-workgroup offsets");
static_assert(BS_THREADS == WG_THREADS, "k_bs_count and k_bs_len scan with d_wg_exclusive");

// bits that hold tid' (0 .. n_chr)
BS_HD int bs_chr_bits(int n_chr) { int b = 0; for (uint32_t x = (uint32_t)n_chr; x; x >>= 1) b++; return b; }
BS_HD int bs_key_bits(int n_chr) { return 33 + bs_chr_bits(n_chr); }
// the sort key of the record that starts (with its block_size) at rec.  Nothing is checked: the caller's walk has seen the fixed part inside its range
BS_HD uint64_t bs_key(const unsigned char *rec, int n_chr)
{
    const BamHead h = bam_head(rec, BAM_FIXED);
    const uint64_t tid = h.refid >= 0 && h.refid < n_chr ? (uint64_t)h.refid : (uint64_t)n_chr;
    return tid << 33 | (uint64_t)((uint32_t)h.pos + 1u) << 1 | (uint64_t)(h.flag >> 4 & 1u);
}

// ---- records from outside (dg_bam_sort_add): every field the store relies on is checked ----
enum { BS_REC_OK = 0, BS_REC_TRUNCATED, BS_REC_SIZE, BS_REC_NAME, BS_REC_REFID, BS_REC_POS };
BS_HD const char *bs_rec_why(int code)
{
    switch (code) {
    case BS_REC_TRUNCATED: return "the record ends behind the input";
    case BS_REC_SIZE: return "block_size is smaller than the record's fields need";
    case BS_REC_NAME: return "l_read_name is 0";
    case BS_REC_REFID: return "refID is not below the number of chromosomes";
    case BS_REC_POS: return "pos is below -1";
    default: return "ok";
    }
}
// the record at p with `left` bytes behind p: BS_REC_OK and *size = its bytes with the block_size field, or the first rule it breaks
BS_HD int bs_record_check(const unsigned char *p, size_t left, int n_chr, size_t *size)
{
    if (left < 4) return BS_REC_TRUNCATED;
    const uint64_t bs = bs_le32(p);
    if (bs < 32) return BS_REC_SIZE;
    if (bs > left - 4) return BS_REC_TRUNCATED;
    const BamHead h = bam_head(p, left);                      // (bs >= 32 lies inside left: the fixed part does)
    if (h.block < h.aux_at) return BS_REC_SIZE;
    if (h.l_name == 0) return BS_REC_NAME;
    if (h.refid >= n_chr) return BS_REC_REFID;
    if (h.pos < -1) return BS_REC_POS;
    *size = (size_t)bs + 4;
    return BS_REC_OK;
}
// whole records in n bytes: f(index, offset) for each; returns their number, or sets *why (and *bad = the first bad record's index) and stops
template <class F>
inline size_t bs_walk_checked(const unsigned char *p, size_t n, int n_chr, size_t *bad, int *why, F f)
{
    size_t at = 0, k = 0;
    *why = BS_REC_OK;
    while (at < n) {
        size_t sz = 0;
        const int rc = bs_record_check(p + at, n - at, n_chr, &sz);
        if (rc) { *why = rc; *bad = k; return k; }
        f(k, at);
        at += sz; k++;
    }
    return k;
}

// ---- a read's records inside the batch's array: [beg, end) holds whole records the library wrote itself; the walk still never leaves the range ----
template <class F>
BS_HD uint32_t bs_range_walk(const unsigned char *rec, uint64_t beg, uint64_t end, F f)
{
    uint32_t k = 0;
    uint64_t at = beg;
    while (at + BAM_FIXED <= end) {
        const uint64_t nxt = at + 4 + (uint64_t)bs_le32(rec + at);
        if (nxt > end || nxt < at + BAM_FIXED) break;
        f(k, at);
        at = nxt; k++;
    }
    return k;
}
struct BsNoop { BS_HD void operator()(uint32_t, uint64_t) const {} };
struct BsEmit {
    const unsigned char *rec; uint64_t *keys; int64_t *offs; uint64_t first, limit, store_base; int n_chr;
    BS_HD void operator()(uint32_t k, uint64_t at) const
    {
        const uint64_t i = first + k;
        if (i < limit) { keys[i] = bs_key(rec + at, n_chr); offs[i] = (int64_t)(store_base + at); }
    }
};
// where read k's records begin in the batch's array (k_bam_len's offsets); k == n_reads: the array's end
BS_HD uint64_t bs_read_begin(const uint64_t *read_off, const uint64_t *tile_base, int k, int n_reads, uint64_t total)
{
    return k < n_reads ? tile_base[k / BS_THREADS] + read_off[k] : total;
}

// ---- the segments of a store: one per accumulate / add call, in call order; the sort takes them in ascending ordinal, equal ordinals in list order ----
struct BsSeg { uint32_t ordinal; uint64_t start, count; };
inline void bs_order_segments(const BsSeg *segs, size_t n, uint32_t *order)
{
    for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    std::stable_sort(order, order + n, [segs](uint32_t a, uint32_t b) { return segs[a].ordinal < segs[b].ordinal; });
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BS_THREADS)
k_bs_count(const unsigned char *__restrict__ rec, const uint64_t *__restrict__ read_off, const uint64_t *__restrict__ tile_base, int n_reads, unsigned long long total,
           uint32_t *__restrict__ cnt_off, uint32_t *__restrict__ tile_cnt)
{
    __shared__ uint32_t s_wave[BS_THREADS / 64];
    const int k = (int)(blockIdx.x * BS_THREADS + threadIdx.x);
    uint32_t mine = 0;
    if (k < n_reads) mine = bs_range_walk(rec, bs_read_begin(read_off, tile_base, k, n_reads, total), bs_read_begin(read_off, tile_base, k + 1, n_reads, total), BsNoop());
    uint32_t all;
    const uint32_t ex = d_wg_exclusive(mine, all, s_wave);
    if (k < n_reads) cnt_off[k] = ex;
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = all;
}

// rec_first: the store's record count before this batch; limit = rec_first + the records the formatter counted (nothing is written behind it)
__global__ void __launch_bounds__(BS_THREADS)
k_bs_emit(const unsigned char *__restrict__ rec, const uint64_t *__restrict__ read_off, const uint64_t *__restrict__ tile_base, int n_reads, unsigned long long total,
          const uint32_t *__restrict__ cnt_off, const uint32_t *__restrict__ tile_cnt_base, int n_chr, unsigned long long rec_first, unsigned long long limit,
          unsigned long long store_base, uint64_t *__restrict__ keys, int64_t *__restrict__ offs)
{
    const int k = (int)(blockIdx.x * BS_THREADS + threadIdx.x);
    if (k >= n_reads) return;
    const BsEmit e{rec, keys, offs, rec_first + tile_cnt_base[blockIdx.x] + cnt_off[k], limit, store_base, n_chr};
    (void)bs_range_walk(rec, bs_read_begin(read_off, tile_base, k, n_reads, total), bs_read_begin(read_off, tile_base, k + 1, n_reads, total), e);
}

__global__ void __launch_bounds__(256)
k_bs_shift(const int64_t *__restrict__ src, int64_t *__restrict__ dst, unsigned long long n, long long delta)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i < n) dst[i] = src[i] + delta;
}

__global__ void __launch_bounds__(BS_THREADS)
k_bs_len(const unsigned char *__restrict__ store, const int64_t *__restrict__ offs, uint32_t n, uint64_t *__restrict__ dst_off, uint64_t *__restrict__ tile_sum)
{
    __shared__ uint64_t s_wave[BS_THREADS / 64];
    const uint32_t i = blockIdx.x * BS_THREADS + threadIdx.x;
    const uint64_t mine = i < n ? 4ull + (uint64_t)bs_le32(store + offs[i]) : 0ull;
    uint64_t all;
    const uint64_t ex = d_wg_exclusive(mine, all, s_wave);
    if (i < n) dst_off[i] = ex;
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// `out` is dword aligned and holds out_bytes; the store is readable up to 3 bytes behind its last record (its allocation is padded)
__global__ void __launch_bounds__(64 * BS_GATHER_WAVES)
k_bs_gather(const unsigned char *__restrict__ store, const int64_t *__restrict__ offs, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base,
            uint32_t n, unsigned long long out_bytes, unsigned char *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * BS_GATHER_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    const unsigned char *s = store + offs[i];
    const uint64_t at = bam_rec_start(dst_off, tile_base, (uint32_t)i);
    unsigned char *d = out + at;
    const uint32_t len = 4u + bs_le32(s);
    if (at + len > out_bytes) return;                          // (the lengths add up to the store's bytes; a record that would not fit is never written)
    uint32_t head = (4u - (uint32_t)((uintptr_t)d & 3u)) & 3u;
    if (head > len) head = len;
    if (lane < head) d[lane] = s[lane];
    s += head; d += head;
    const uint32_t rem = len - head, nd = rem >> 2, tail = rem & 3u;
    const uint32_t mis = (uint32_t)((uintptr_t)s & 3u), sh = mis * 8u;
    const uint32_t *sa = (const uint32_t *)(s - mis);
    uint32_t *da = (uint32_t *)d;
    if (sh == 0) { for (uint32_t j = lane; j < nd; j += 64u) da[j] = sa[j]; }
    else { for (uint32_t j = lane; j < nd; j += 64u) da[j] = sa[j] >> sh | sa[j + 1] << (32u - sh); }
    if (lane < tail) d[4u * nd + lane] = s[4u * nd + lane];
}
#endif
#endif
