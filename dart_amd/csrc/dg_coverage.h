// dg_coverage.h -- the coverage track (bedGraph) of the coordinate-sorted BAM, built in HBM next to the sort (dg_bamsort.h): after dg_bam_sort_finish every
// record of the job lies in one array and its place is known, so the per-base depth a genome browser shows is arithmetic over the records' own bytes.  It needs
// neither the blocks' sizes nor the file.  The reference has no such output: an opt-in extension (what `bedtools genomecov -bg -split` or `samtools depth`
// would compute from the sorted file, read back and inflated, on one core).
//
// THE DEFINITION.  No bedtools or samtools exists where this project is built and tested: this definition -- modelled on `bedtools genomecov -bg -split`
// (blocks, 0-based half-open intervals, zero depth not printed) with the default filter of `samtools depth` (FLAG 0x704 skipped) -- is what the tests pin
// (tests/coverage_inputs.py is its sequential twin).
//
// Per sorted record (its fields and CIGAR as bam_head and bam_cigar_walk of dg_bamrec.h read them; no read ever passes the record's block_size or the array's end):
//   counted  all of: 0 <= refID < n_chr; pos >= 0; flag & 4 clear; n_cigar_op > 0; (flag & exclude_flags) == 0; mapq >= min_mapq; the strand selection, if
//            any, passes; and the CIGAR lies inside the record and the array: 36 + l_read_name + 4 n_cigar_op <= 4 + block_size (dg_bam_sort_add refuses a
//            record that breaks the last rule, so it is reachable only by the lane code's tests)
//   strand   s = (flag >> 4 & 1) ^ (flag >> 7 & 1): a second mate counts for the opposite strand.  DG_COV_STRAND_PLUS keeps s == 0, DG_COV_STRAND_MINUS
//            s == 1; both set, or neither: every record
//   blocks   walk with p = pos: op 0, 7, 8 (M, =, X) of length L > 0 is a block [p, p + L), then p += L; op 2, 3 (D, N) is p += L and no block; every other op
//            changes nothing.  Mates that overlap both count.
//   range    a block end above 2^32 - 1 on a counted record: DG_ERR_RANGE, the text names the record's index; no track is left behind
//   Positions are not clamped to the chromosome's length (the BAI does not clamp either; the formatter never writes such a record).
// Depth.  Every block gives two events, (refID, start, +1) and (refID, end, -1), ordered by the key refID << 32 | position.  The deltas of equal keys are
//   summed; keys whose sum is 0 are dropped (a read ending where another begins is no breakpoint); the running sum over what remains is the depth from that
//   position to the next.  Every block opens and closes on one reference, so the running sum is 0 at each reference's end: a plain scan, no segmented one.
// Entries.  dg_cov_entry { uint32_t chr, start, end, depth; }: one for every breakpoint with depth > 0, end = the next breakpoint's position; ascending
//   (chr, start); neighbours that touch always differ in depth; a chromosome without coverage has none.
// Text.  Per entry "name\tstart\tend\tdepth\n", decimal, no header line; the names are dg_set_chr_names'.
// The result is a function of the record SET: the same records give the same bytes whatever their order, the grid, the batch split, the ordinals, the
// contexts used or the store's growth history (sums of equal keys do not depend on the order inside a run of equal keys).
//
//   k_cv_count      lane = sorted record: the field reads, the filter and the CIGAR walk; the workgroup's exclusive scan of the block counts and their sum;
//                   per workgroup the counted records, the aligned bases, the smallest and largest event key and the first record out of range
//   k_cv_top        one workgroup: the scan of the workgroups' sums and their total; the workgroups' other values summed, or their maximum taken.  (Behind
//                   k_cv_count, k_cv_flag and k_cv_entries.  The first shape had every wave add to one global word per value: 31 k waves on five
//                   addresses made the counting walk thirteen times as slow as the emitting walk over the same bytes.)
//   -- the first wait: the number of events sizes the sorter's buffers; a record out of range ends the call --
//   k_cv_emit       lane = sorted record: the same walk; block b of the array leaves the pairs (start key, +1) and (end key, -1) at 2 b and 2 b + 1
//   (sort)          one stable radix sort of the events (rs_sort_passes of dg_sort.h): only the low digits in which the smallest and largest key differ
//   k_cv_depth      lane = sorted event: the workgroup's inclusive scan of the deltas and its sum (k_tiles_top of dg_wgscan.h).  32 bit: a record's blocks do not overlap,
//                   so no prefix of the sorted deltas exceeds the number of records (< 2^32), and none is negative (an end's start lies in front of it)
//   k_cv_tails      lane = event: the last event of a run of equal keys (a tail) carries the depth behind its position; per workgroup its last tail's depth
//   k_cv_tails_top  one workgroup: a last-valid scan over those, so every workgroup knows the depth of the last tail in front of it, however far back it lies
//   k_cv_flag       lane = event: the last-valid scan inside the workgroup; a tail is a breakpoint iff its depth differs from the previous tail's, an entry iff
//                   that depth is above 0; the workgroup's exclusive scan of both counts (k_cv_top over entries << 32 | breakpoints); the largest depth
//   -- the second wait: the numbers of breakpoints and entries size their arrays and bound the text --
//   k_cv_compact    lane = event: breakpoint q gets its key and depth, entry j the number of its breakpoint
//   k_cv_entries    lane = entry: the dg_cov_entry (end = the next breakpoint's position: the last breakpoint of a reference has depth 0, so an entry always
//                   has a successor on its reference), its line's length, the workgroup's scan (k_cv_top); covered bases and the sum of depth x length
//   k_cv_write      lane = entry: the line's bytes at the scanned place
// A run of equal keys may straddle workgroups and sorter tiles, and the previous tail may lie any number of workgroups back: both scans carry what they need
// across workgroups (k_tiles_top, k_cv_tails_top); no lane reads a neighbour's result, and no kernel here uses an atomic.
// Memory: 4 bytes per record; 40 bytes per event (two key and two value buffers of the sorter, the scanned delta, the marks) and the sorter's histograms; 12
// per breakpoint; 24 per entry and its line; up to 40 per workgroup.  Everything a lane computes is host-callable: tests/native/coverage_checks.hip runs the same code on the CPU.
#ifndef DG_COVERAGE_H
#define DG_COVERAGE_H
#include "dg_bamsort.h"
#include "dg_wgscan.h"

#define CV_HD __host__ __device__ __forceinline__
#define CV_THREADS 256               // records / events / entries per workgroup of every kernel here (dg_bam_coverage_granules [0])
#define CV_MAX_POS 0xFFFFFFFFull     // the largest block end an entry holds
#define CV_NONE (~0ull)              // no tail yet (the last-valid scans)
#define CV_PLANES 5                  // the most per-workgroup values a kernel leaves for k_cv_top
static_assert(CV_THREADS == BS_THREADS, "k_cv_count reads k_bs_len's per-workgroup offsets");
static_assert(CV_THREADS == WG_THREADS, "the kernels here and of dg_markdup.h scan with d_wg_exclusive");
// the call's small device state, 64-bit words.  k_cv_top's outputs lie side by side: sums first, then maxima
enum { CV_ST_BLOCKS = 0, CV_ST_COUNTED, CV_ST_ALIGNED, CV_ST_NMIN /* max of ~key = ~min */, CV_ST_MAX, CV_ST_NBAD /* max of ~index of a record out of range; 0: none */,
       CV_ST_DEPTH_END /* the scanned deltas' total: 0 */, CV_ST_MARKS /* entries << 32 | breakpoints */, CV_ST_MAX_DEPTH, CV_ST_BYTES, CV_ST_COVERED, CV_ST_AREA /* sum of depth x length */,
       CV_ST_WORDS = 16 };

struct CvFilter { uint32_t flags /* DG_COV_STRAND_* */, exclude, min_mapq; };
struct CvRec { bool counted; int32_t refid, pos; uint64_t cigar_at; uint32_t n_ops; };

static_assert(sizeof(dg_cov_entry) == 16, "an entry is 16 bytes");

CV_HD bool cv_strand_passes(uint32_t flags, uint32_t flag)
{
    const uint32_t want = flags & (DG_COV_STRAND_PLUS | DG_COV_STRAND_MINUS), s = (flag >> 4 & 1u) ^ (flag >> 7 & 1u);
    if (want == 0u || want == (DG_COV_STRAND_PLUS | DG_COV_STRAND_MINUS)) return true;
    return want == DG_COV_STRAND_PLUS ? s == 0u : s == 1u;
}
// the record with the fixed fields h: counted only when its whole CIGAR lies inside the record and the array
CV_HD CvRec cv_record(const BamHead &h, int n_chr, const CvFilter &f)
{
    CvRec r; r.refid = h.refid; r.pos = h.pos; r.cigar_at = h.cigar_at; r.n_ops = h.n_cigar;
    r.counted = h.ok && h.refid >= 0 && h.refid < n_chr && h.pos >= 0 && !(h.flag & 4u) && h.n_cigar > 0u && !(h.flag & f.exclude) && h.mapq >= f.min_mapq &&
                cv_strand_passes(f.flags, h.flag) && h.seq_at <= h.size;
    return r;
}
// the record that starts (with its block_size) at rec, `avail` bytes of the array behind rec
CV_HD CvRec cv_record(const unsigned char *rec, uint64_t avail, int n_chr, const CvFilter &f) { return cv_record(bam_head(rec, avail), n_chr, f); }
CV_HD uint64_t cv_key(int32_t refid, uint64_t position) { return (uint64_t)(uint32_t)refid << 32 | position; }
CV_HD int cv_key_bits_max(int n_chr) { return 32 + bs_chr_bits(n_chr); }
// how many low bits the smallest and the largest key differ in: every key between them shares the digits above
CV_HD int cv_key_bits(uint64_t lo, uint64_t hi) { int b = 0; for (uint64_t x = lo ^ hi; x; x >>= 1) b++; return b; }
// the blocks of a counted record: f(k, start, end) for block k; returns their number.  p stays below 2^31 + 65535 * 2^28
template <class F>
CV_HD uint32_t cv_blocks(const unsigned char *rec, const CvRec &r, F &f)
{
    uint32_t k = 0;
    bam_cigar_walk(rec, r.cigar_at, r.n_ops, (uint64_t)r.pos, [&](uint32_t op, uint32_t len, uint64_t p, uint64_t) { if (bam_op_aligned(op) && len) { f(k, p, p + len); k++; } });
    return k;
}
struct CvTally {                    // k_cv_count's walk
    uint64_t aligned, lo, hi; bool bad;
    CV_HD void operator()(uint32_t, uint64_t s, uint64_t e) { aligned += e - s; if (s < lo) lo = s; if (e > hi) hi = e; if (e > CV_MAX_POS) bad = true; }
};
struct CvEmit {                     // k_cv_emit's: block `first + k` of the array, nothing written at or behind block `limit`
    uint64_t *keys; int64_t *vals; uint64_t first, limit; int32_t refid;
    CV_HD void operator()(uint32_t k, uint64_t s, uint64_t e)
    {
        const uint64_t b = first + k;
        if (b < limit && e <= CV_MAX_POS) { keys[2 * b] = cv_key(refid, s); vals[2 * b] = 1; keys[2 * b + 1] = cv_key(refid, e); vals[2 * b + 1] = -1; }
    }
};
// the last-valid scans: a tail keeps its own depth, every other event takes what lies to its left
CV_HD uint64_t cv_fill(uint64_t left, uint64_t own) { return own != CV_NONE ? own : left; }
CV_HD bool cv_is_tail(uint64_t key, uint64_t key_behind, bool last) { return last || key != key_behind; }
CV_HD bool cv_is_breakpoint(bool tail, uint32_t depth, uint32_t depth_of_previous_tail) { return tail && depth != depth_of_previous_tail; }
// an event's mark: the breakpoints and entries in front of it in its workgroup (at most 255 each), and what it is itself
CV_HD uint32_t cv_mark(uint32_t counts_before, bool bp, bool ent) { return counts_before | (bp ? 1u << 30 : 0u) | (ent ? 1u << 31 : 0u); }
CV_HD uint32_t cv_mark_bps(uint32_t m) { return m & 0x1ffu; }
CV_HD uint32_t cv_mark_ents(uint32_t m) { return m >> 16 & 0x1ffu; }
CV_HD dg_cov_entry cv_entry(uint64_t key, uint64_t key_next, uint32_t depth)
{
    dg_cov_entry e; e.chr = (uint32_t)(key >> 32); e.start = (uint32_t)key; e.end = (uint32_t)key_next; e.depth = depth;
    return e;
}
// "%s\t%u\t%u\t%u\n"
CV_HD void cv_line_numbers(SamSink &o, const dg_cov_entry &e)
{
    o.ch('\t'); sam_put_num(o, (long long)e.start);
    o.ch('\t'); sam_put_num(o, (long long)e.end);
    o.ch('\t'); sam_put_num(o, (long long)e.depth);
    o.ch('\n');
}
CV_HD uint32_t cv_line_len(const uint32_t *name_off, const dg_cov_entry &e)
{
    SamSink o{nullptr, 0, 0};
    cv_line_numbers(o, e);
    return o.n + (name_off[e.chr + 1] - name_off[e.chr]);
}
CV_HD uint32_t cv_line_write(char *out, const uint32_t *name_off, const char *names, const dg_cov_entry &e)
{
    SamSink o{out, 0, 0xFFFFFFFFu};
    for (uint32_t i = name_off[e.chr]; i < name_off[e.chr + 1]; i++) o.ch(names[i]);
    cv_line_numbers(o, e);
    return o.n;
}
// the most bytes a line takes: a name, three numbers of at most 10 digits, three tabs and the line end
CV_HD uint64_t cv_line_bound(uint32_t name_max) { return (uint64_t)name_max + 3 * 10 + 4; }

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
// the workgroup's values -- v[p] summed for p < n_sum, else the maximum -- into plane p of `part` (planes x workgroups): every wave leaves its own in LDS, the first N
// threads combine the four.  s_part holds 4 N words.
template <int N>
__device__ __forceinline__ void cv_block_partials(const unsigned long long (&v)[N], int n_sum, unsigned long long *s_part, uint64_t *__restrict__ part)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < N; p++) {
        const unsigned long long w = p < n_sum ? d_wave_sum(v[p]) : d_wave_max(v[p]);
        if (lane == 0u) s_part[p * (CV_THREADS / 64) + wv] = w;
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)N) {
        const int p = (int)threadIdx.x;
        unsigned long long a = s_part[p * (CV_THREADS / 64)];
        for (uint32_t k = 1; k < CV_THREADS / 64; k++) { const unsigned long long b = s_part[p * (CV_THREADS / 64) + k]; a = p < n_sum ? a + b : (b > a ? b : a); }
        part[(size_t)p * gridDim.x + blockIdx.x] = a;
    }
}

// one workgroup: tile_sum scanned in place (exclusive), *total = its sum; out[p] = plane p of `part` (n_planes x n_tiles) summed for p < n_sum, else its maximum
__global__ void __launch_bounds__(CV_THREADS)
k_cv_top(uint64_t *__restrict__ tile_sum, uint32_t n_tiles, unsigned long long *__restrict__ total, const uint64_t *__restrict__ part, int n_planes, int n_sum, unsigned long long *__restrict__ out)
{
    __shared__ uint64_t s_wave[CV_THREADS / 64];
    __shared__ unsigned long long s_part[CV_PLANES * (CV_THREADS / 64)];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t all = d_tiles_exclusive<uint64_t>(tile_sum, n_tiles, 1, s_wave);
    if (threadIdx.x == 0) *total = all;
    unsigned long long acc[CV_PLANES];
#pragma unroll
    for (int p = 0; p < CV_PLANES; p++) acc[p] = 0ull;
    for (uint32_t t = threadIdx.x; t < n_tiles; t += CV_THREADS) {
#pragma unroll
        for (int p = 0; p < CV_PLANES; p++)
            if (p < n_planes) { const unsigned long long v = part[(size_t)p * n_tiles + t]; acc[p] = p < n_sum ? acc[p] + v : (v > acc[p] ? v : acc[p]); }
    }
#pragma unroll
    for (int p = 0; p < CV_PLANES; p++) {
        const unsigned long long w = p < n_sum ? d_wave_sum(acc[p]) : d_wave_max(acc[p]);
        if (lane == 0u) s_part[p * (CV_THREADS / 64) + wv] = w;
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)n_planes && threadIdx.x < CV_PLANES) {
        const int p = (int)threadIdx.x;
        unsigned long long a = s_part[p * (CV_THREADS / 64)];
        for (uint32_t k = 1; k < CV_THREADS / 64; k++) { const unsigned long long b = s_part[p * (CV_THREADS / 64) + k]; a = p < n_sum ? a + b : (b > a ? b : a); }
        out[p] = a;
    }
}

__global__ void __launch_bounds__(CV_THREADS)
k_cv_count(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, int n_chr,
           const CvFilter f, uint32_t *__restrict__ blk_off, uint64_t *__restrict__ tile_sum, uint64_t *__restrict__ part /* 5 planes: counted, aligned | ~min key, max key, ~bad */)
{
    __shared__ uint64_t s_wave[CV_THREADS / 64];
    __shared__ unsigned long long s_part[5 * (CV_THREADS / 64)];
    const uint32_t i = blockIdx.x * CV_THREADS + threadIdx.x;
    uint64_t mine = 0, counted = 0, nmin = 0, kmax = 0, nbad = 0;
    CvTally t; t.aligned = 0; t.lo = CV_NONE; t.hi = 0; t.bad = false;
    if (i < n) {
        const uint64_t at = bam_rec_start(dst_off, tile_base, i);
        if (at < n_raw) {
            const CvRec r = cv_record(sorted + at, n_raw - at, n_chr, f);
            if (r.counted) {
                counted = 1;
                mine = cv_blocks(sorted + at, r, t);
                if (t.bad) nbad = ~(uint64_t)i;
                else if (mine) { nmin = ~cv_key(r.refid, t.lo); kmax = cv_key(r.refid, t.hi); }
            }
        }
    }
    uint64_t all;
    const uint64_t ex = d_wg_exclusive(mine, all, s_wave);
    if (i < n) blk_off[i] = (uint32_t)ex;                      // (at most 255 records of at most 65535 blocks in front)
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
    const unsigned long long v[5] = {counted, t.bad ? 0ull : t.aligned, nmin, kmax, nbad};
    cv_block_partials(v, 2, s_part, part);
}

// blk_base: k_cv_count's sums, scanned; n_blocks: their total as the host read it
__global__ void __launch_bounds__(CV_THREADS)
k_cv_emit(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, int n_chr,
          const CvFilter f, const uint32_t *__restrict__ blk_off, const uint64_t *__restrict__ blk_base, unsigned long long n_blocks, uint64_t *__restrict__ keys, int64_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * CV_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t at = bam_rec_start(dst_off, tile_base, i);
    if (at >= n_raw) return;
    const CvRec r = cv_record(sorted + at, n_raw - at, n_chr, f);
    if (!r.counted) return;
    CvEmit e{keys, vals, blk_base[blockIdx.x] + blk_off[i], n_blocks, r.refid};
    (void)cv_blocks(sorted + at, r, e);
}

__global__ void __launch_bounds__(CV_THREADS)
k_cv_depth(const int64_t *__restrict__ vals, uint32_t n_ev, uint32_t *__restrict__ incl, uint32_t *__restrict__ tile_sum)
{
    __shared__ uint32_t s_wave[CV_THREADS / 64];
    const uint32_t i = blockIdx.x * CV_THREADS + threadIdx.x;
    const uint32_t mine = i < n_ev ? (uint32_t)vals[i] : 0u;
    uint32_t all;
    const uint32_t ex = d_wg_exclusive(mine, all, s_wave);
    if (i < n_ev) incl[i] = ex + mine;
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// event i's depth when it is a tail, else CV_NONE (dep_base: k_cv_depth's sums, scanned)
__device__ __forceinline__ uint64_t cv_tail_depth(const uint64_t *keys, const uint32_t *incl, const uint32_t *dep_base, uint32_t i, uint32_t n_ev)
{
    if (i >= n_ev || !cv_is_tail(keys[i], i + 1u < n_ev ? keys[i + 1u] : 0ull, i + 1u == n_ev)) return CV_NONE;
    return (uint64_t)(uint32_t)(dep_base[i / CV_THREADS] + incl[i]);
}
// inclusive last-valid scan over the wave's lanes
__device__ __forceinline__ uint64_t cv_wave_fill(uint64_t v, uint32_t lane)
{
    for (int o = 1; o < 64; o <<= 1) { const uint64_t left = __shfl_up(v, o, 64); if (lane >= (uint32_t)o) v = cv_fill(left, v); }
    return v;
}

__global__ void __launch_bounds__(CV_THREADS)
k_cv_tails(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ incl, const uint32_t *__restrict__ dep_base, uint32_t n_ev, uint64_t *__restrict__ tile_last)
{
    __shared__ uint64_t s_last[CV_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t v = cv_wave_fill(cv_tail_depth(keys, incl, dep_base, blockIdx.x * CV_THREADS + threadIdx.x, n_ev), lane);
    if (lane == 63u) s_last[wv] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t all = CV_NONE;
        for (uint32_t k = 0; k < CV_THREADS / 64; k++) all = cv_fill(all, s_last[k]);
        tile_last[blockIdx.x] = all;
    }
}

// tile_prev[t] = the depth of the last tail in front of workgroup t (0 in front of the first tail); n_tiles + 1 values
__global__ void __launch_bounds__(CV_THREADS)
k_cv_tails_top(const uint64_t *__restrict__ tile_last, uint32_t n_tiles, uint32_t *__restrict__ tile_prev)
{
    __shared__ uint64_t s_last[CV_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint64_t carry = 0;
    if (threadIdx.x == 0) tile_prev[0] = 0u;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += CV_THREADS) {
        const uint32_t t = t0 + threadIdx.x;
        uint64_t v = cv_wave_fill(t < n_tiles ? tile_last[t] : CV_NONE, lane);
        if (lane == 63u) s_last[wv] = v;
        __syncthreads();
        uint64_t before = carry, all = carry;
        for (uint32_t k = 0; k < CV_THREADS / 64; k++) { all = cv_fill(all, s_last[k]); if (k < wv) before = all; }
        v = cv_fill(before, v);
        if (t < n_tiles) tile_prev[t + 1u] = (uint32_t)v;
        carry = all;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(CV_THREADS)
k_cv_flag(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ incl, const uint32_t *__restrict__ dep_base, const uint32_t *__restrict__ tile_prev, uint32_t n_ev,
          uint32_t *__restrict__ mark, uint64_t *__restrict__ tile_cnt, uint64_t *__restrict__ part /* 1 plane: the largest depth */)
{
    __shared__ uint64_t s_last[CV_THREADS / 64];
    __shared__ uint32_t s_wave[CV_THREADS / 64];
    __shared__ unsigned long long s_part[CV_THREADS / 64];
    const uint32_t i = blockIdx.x * CV_THREADS + threadIdx.x, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t own = cv_tail_depth(keys, incl, dep_base, i, n_ev);
    const uint64_t w = cv_wave_fill(own, lane);
    uint64_t left = __shfl_up(w, 1, 64);
    if (lane == 0u) left = CV_NONE;
    if (lane == 63u) s_last[wv] = w;
    __syncthreads();
    uint64_t before = (uint64_t)tile_prev[blockIdx.x];
    for (uint32_t k = 0; k < wv; k++) before = cv_fill(before, s_last[k]);
    const uint32_t prev = (uint32_t)cv_fill(before, left);
    const bool tail = own != CV_NONE, bp = cv_is_breakpoint(tail, (uint32_t)own, prev), ent = bp && (uint32_t)own > 0u;
    uint32_t all;
    const uint32_t ex = d_wg_exclusive((bp ? 1u : 0u) | (ent ? 1u << 16 : 0u), all, s_wave);
    if (i < n_ev) mark[i] = cv_mark(ex, bp, ent);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (uint64_t)(all >> 16) << 32 | (uint64_t)(all & 0xffffu);
    const unsigned long long v[1] = {tail ? (unsigned long long)(uint32_t)own : 0ull};
    cv_block_partials(v, 0, s_part, part);
}

// cnt_base: k_cv_flag's counts, scanned (entries << 32 | breakpoints)
__global__ void __launch_bounds__(CV_THREADS)
k_cv_compact(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ incl, const uint32_t *__restrict__ dep_base, const uint32_t *__restrict__ mark, const uint64_t *__restrict__ cnt_base,
             uint32_t n_ev, uint32_t n_bp, uint32_t n_ent, uint64_t *__restrict__ bp_key, uint32_t *__restrict__ bp_depth, uint32_t *__restrict__ ent_bp)
{
    const uint32_t i = blockIdx.x * CV_THREADS + threadIdx.x;
    if (i >= n_ev) return;
    const uint32_t m = mark[i];
    if (!(m >> 30 & 1u)) return;
    const uint64_t base = cnt_base[blockIdx.x];
    const uint32_t q = (uint32_t)base + cv_mark_bps(m), j = (uint32_t)(base >> 32) + cv_mark_ents(m);
    if (q >= n_bp) return;
    bp_key[q] = keys[i]; bp_depth[q] = dep_base[blockIdx.x] + incl[i];
    if ((m >> 31) && j < n_ent) ent_bp[j] = q;
}

// name_off == nullptr: entries only
__global__ void __launch_bounds__(CV_THREADS)
k_cv_entries(const uint64_t *__restrict__ bp_key, const uint32_t *__restrict__ bp_depth, const uint32_t *__restrict__ ent_bp, uint32_t n_bp, uint32_t n_ent, int n_chr,
             const uint32_t *__restrict__ name_off, dg_cov_entry *__restrict__ entries, uint32_t *__restrict__ line_off, uint64_t *__restrict__ tile_sum,
             uint64_t *__restrict__ part /* 2 planes: covered bases, depth x length */)
{
    __shared__ uint64_t s_wave[CV_THREADS / 64];
    __shared__ unsigned long long s_part[2 * (CV_THREADS / 64)];
    const uint32_t j = blockIdx.x * CV_THREADS + threadIdx.x;
    uint64_t mine = 0, covered = 0, area = 0;
    if (j < n_ent) {
        const uint32_t q = ent_bp[j];
        dg_cov_entry e; e.chr = 0; e.start = 0; e.end = 0; e.depth = 0;
        if (q < n_bp - 1u) e = cv_entry(bp_key[q], bp_key[q + 1u], bp_depth[q]);
        entries[j] = e;
        covered = (uint64_t)e.end - e.start; area = covered * e.depth;
        if (name_off && e.chr < (uint32_t)n_chr) mine = cv_line_len(name_off, e);
    }
    uint64_t all;
    const uint64_t ex = d_wg_exclusive(mine, all, s_wave);
    if (j < n_ent) line_off[j] = (uint32_t)ex;
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
    const unsigned long long v[2] = {covered, area};
    cv_block_partials(v, 2, s_part, part);
}

__global__ void __launch_bounds__(CV_THREADS)
k_cv_write(const dg_cov_entry *__restrict__ entries, uint32_t n_ent, int n_chr, const uint32_t *__restrict__ name_off, const char *__restrict__ names, const uint32_t *__restrict__ line_off,
           const uint64_t *__restrict__ line_base, const unsigned long long *__restrict__ stat, unsigned long long cap, char *__restrict__ out)
{
    const uint32_t j = blockIdx.x * CV_THREADS + threadIdx.x;
    if (j >= n_ent || stat[CV_ST_BYTES] > cap) return;
    const dg_cov_entry e = entries[j];
    if (e.chr >= (uint32_t)n_chr) return;
    cv_line_write(out + line_base[blockIdx.x] + line_off[j], name_off, names, e);
}
#endif
#endif
