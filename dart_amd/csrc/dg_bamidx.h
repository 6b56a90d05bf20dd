// dg_bamidx.h -- the BAM index (.bai) of the coordinate-sorted BAM, built in HBM next to the sort (dg_bamsort.h): after dg_bam_sort_finish the records lie in
// coordinate order in one array, every record's place in it is known (k_bs_len's scanned offsets and the per-tile bases), and after dg_bam_sort_compress so is
// every BGZF block's compressed size.  A record's virtual file offset follows by arithmetic, because the array is cut into blocks of exactly 0xff00 input
// bytes: the host never looks at a record.  The reference has no such output: an opt-in extension (what `samtools index` would write behind `samtools sort`).
//
// THE DEFINITION.  The index is the BAI of SAM specification 5.2, built the way htslib's hts_idx_push / hts_idx_finish build it for a BAM read record by
// record, with two deliberate differences (named below).  No samtools or htslib binary exists where this project is built and tested: this definition -- not
// a run of samtools -- is what the tests pin (tests/bamidx_inputs.py is its sequential twin).
//
// Per sorted record (its fields and CIGAR as bam_head and bam_cigar_walk of dg_bamrec.h read them):
//   placed   0 <= refID < n_chr.  All other records come last in the sorted array; they are only counted, in n_no_coor
//   mapped   flag & 4 is clear
//   rlen     the sum of len over ops 0, 2, 3, 7, 8 (M, D, N, =, X) when the record is mapped and n_cigar_op > 0, else 0
//   end_raw  pos + (rlen ? rlen : 1);  beg = max(pos, 0), end = max(end_raw, beg + 1)
//            (the clamp applies to every placed record; htslib clamps only mapped ones.  The formatter never writes a placed record with pos = -1, so the
//             difference is reachable only through dg_bam_sort_add)
//   bin      bam_reg2bin(beg, end) of dg_bamfmt.h: recomputed, not read from the record's bin field -- exactly as htslib does
//   end > 2^29 on a placed record: DG_ERR_RANGE, the text names the record's index and says that such a reference needs a CSI index; no index is left
//   behind, the sorted array and the store stay as they were
// Virtual offsets.  B = 0xff00; coff[k] = first_block_offset + the compressed sizes of blocks 0 .. k-1, coff[n_blocks] = the file offset behind the last data
//   block.  For a position r of the sorted array: voff(r) = coff[r / B] << 16 | r % B for r < n_raw, voff(n_raw) = coff[n_blocks] << 16: what bgzf_tell
//   returns after reading up to r (a position at a block's end reads as the start of the next block).  Every coff must stay below 2^48, else DG_ERR_RANGE.
// Chunks, as hts_idx_push makes them.  Walk the placed records in file order: a chunk is a maximal run of consecutive records with the same (refID, bin); its
//   begin is voff of its first record's start, its end voff of the start of the record behind the run (for the last placed record: the first unplaced
//   record's start, or voff(n_raw)).  Per reference the bins are written in ASCENDING BIN NUMBER (difference 1: htslib writes them in hash-table order; the
//   specification allows any).  Inside a bin the chunks lie in file order; neighbours are merged when prev.end >> 16 >= next.beg >> 16, the merged chunk
//   keeping the earlier begin and the later end (compress_binning's last loop; a bin's chunks are disjoint and ascending, so the test is local).  htslib's
//   other compression step -- moving a bin that spans less than 64 KiB of file to its parent -- is NOT done (difference 2: larger, equally valid).
// The pseudo-bin 37450, only for a reference that has records, last (the largest bin number): two chunks, (voff of the reference's first record's start, voff
//   of its last record's end) and (n_mapped, n_unmapped).  A reference without records has n_bin = 0 and n_intv = 0.
// The linear index.  n_intv = max over the reference's mapped records of ((end - 1) >> 14) + 1; window w holds the smallest voff(start) over the mapped records
//   with beg >> 14 <= w <= (end - 1) >> 14 (= the first such record in file order).  Placed unmapped records are binned and counted but do not touch it.  Empty
//   windows are filled as update_loff fills them: leading ones get the reference's first record's start (the pseudo-bin's first value), a later one its
//   predecessor's value.
// The bytes, all little endian: "BAI\1", int32 n_ref = n_chr; per reference int32 n_bin (counting the pseudo-bin), per bin {u32 bin, int32 n_chunk, n_chunk x
//   {u64 beg, u64 end}}, int32 n_intv, n_intv x u64; finally u64 n_no_coor.  An empty store gives 8 + 8 * n_chr + 8 bytes.
// The same records and the same block sizes give the same bytes, whatever the grid, the batch split, the contexts used, the store's growth history or the piece
// size of dg_bam_sort_compress.
//
//   k_bi_coff        one workgroup: coff[] = first_block_offset + the exclusive scan of the block sizes (64 bit)
//   k_bi_rec         lane = sorted record: the field reads and the CIGAR walk (never past the record's block_size); leaves the key refID << 16 | bin (all ones
//                    for an unplaced record), voff of the record's start, its window span and mapped bit; per reference (wave reduction, then one global
//                    atomic per wave): the number of windows, the mapped and unmapped counts, the first and last record; the first record that is out of range
//   k_bi_heads       lane = record: head flag where (refID, bin) differs from the previous placed record; the workgroup's count        (k_tiles_top)
//   -- the one mid-way wait: the per-reference values, the chunk count and the error word go to the host, which sizes the linear index and the output --
//   k_bi_lin         lane = record: 64-bit atomicMin of voff(start) into its windows (an array of all ones; the minimum makes the order of the atomics irrelevant),
//                    but not into a window the mapped record in front covers too: that one, or one further in front, holds the smaller offset
//   k_bi_chunks      lane = record: the heads compacted, in file order: (key, chunk number) pairs and each chunk's first record
//   (sort)           one stable radix sort of the chunks by refID << 16 | bin (rs_sort_passes of dg_sort.h; 16 + bs_chr_bits(n_chr) key bits)
//   k_bi_merge_scan  lane = sorted chunk: the neighbour merge test and the bin head test; workgroup scan of both counts in one 64-bit word    (k_tiles_top)
//   k_bi_merge_emit  lane = sorted chunk: merged chunk q -> its first sorted chunk and its bin; bin b -> its first merged chunk; reference t -> its first bin and chunk
//   k_bi_refs        one workgroup: every reference's bytes, their scan = its byte offset; magic, n_ref, n_no_coor, the total
//   k_bi_write_chunks lane = merged chunk: its 16 bytes; a bin's first chunk writes the bin's 8 bytes too
//   k_bi_write_refs  workgroup = reference: n_bin, the pseudo-bin, n_intv and the linear index, filled by a segmented last-valid scan
// Every field of the file is dword aligned (a reference's bytes are a multiple of 8), so a u64 goes out as two dword stores.  Everything a lane computes is
// host-callable: tests/native/bamidx_checks.hip runs the same code on the CPU.
#ifndef DG_BAMIDX_H
#define DG_BAMIDX_H
#include "dg_bamsort.h"
#include "dg_wgscan.h"

#define BI_HD __host__ __device__ __forceinline__
#define BI_THREADS 256               // records per workgroup of k_bi_rec (dg_bam_index_granules [0])
static_assert(BI_THREADS == WG_THREADS, "the kernels here scan with d_wg_exclusive");
#define BI_BLOCK 0xff00ull           // input bytes per BGZF block (dg_bgzf.h: BGZF_BLOCK)
#define BI_MAX_END (1ll << 29)       // the largest end a BAI holds
#define BI_PSEUDO_BIN 37450u
#define BI_NONE (~0ull)              // the key of an unplaced record; an empty linear window
#define BI_REF_PLANES 5              // per reference: [0] windows, [1] mapped, [2] unmapped, [3] first record, [4] last record
enum { BI_ST_BAD = 0, BI_ST_CHUNKS, BI_ST_COFF_END, BI_ST_MERGED, BI_ST_BYTES, BI_ST_WORDS = 8 };     // BI_ST_MERGED: bins << 32 | merged chunks

struct BiRec { int32_t refid, pos; long long beg, end, rlen; uint32_t bin; bool placed, mapped; };

// the record that starts (with its block_size) at rec, `avail` bytes of the array behind rec: the walk never leaves the record nor the array
BI_HD BiRec bi_record(const unsigned char *rec, uint64_t avail, int n_chr)
{
    BiRec r; r.refid = -1; r.pos = -1; r.beg = 0; r.end = 1; r.rlen = 0; r.bin = 4680u; r.placed = false; r.mapped = false;
    const BamHead h = bam_head(rec, avail);
    if (!h.ok) return r;
    r.refid = h.refid; r.pos = h.pos;
    r.placed = r.refid >= 0 && r.refid < n_chr;
    r.mapped = !(h.flag & 4u);
    if (r.mapped && h.n_cigar) {                               // the ops are cut to what fits in the record and the array; nothing is refused
        uint64_t n_ops = h.cigar_at <= h.size ? (h.size - h.cigar_at) / 4 : 0;
        if (n_ops > h.n_cigar) n_ops = h.n_cigar;
        r.rlen = (long long)bam_cigar_walk(rec, h.cigar_at, n_ops, 0, BamNoOp()).p;
    }
    const long long end_raw = (long long)r.pos + (r.rlen ? r.rlen : 1);
    r.beg = r.pos > 0 ? (long long)r.pos : 0;
    r.end = end_raw > r.beg + 1 ? end_raw : r.beg + 1;
    r.bin = bam_reg2bin(r.beg, r.end);
    return r;
}
BI_HD uint64_t bi_key(const BiRec &r) { return r.placed ? (uint64_t)(uint32_t)r.refid << 16 | (uint64_t)r.bin : BI_NONE; }
BI_HD int bi_key_bits(int n_chr) { return 16 + bs_chr_bits(n_chr); }
// window span and bits of a record: first window | last window << 15 | mapped << 30 | placed << 31 (end <= 2^29: a window number has 15 bits)
BI_HD uint32_t bi_span(const BiRec &r)
{
    if (!r.placed || r.end > BI_MAX_END) return 0u;
    return (uint32_t)(r.beg >> 14) | (uint32_t)((r.end - 1) >> 14) << 15 | (r.mapped ? 1u << 30 : 0u) | 1u << 31;
}
BI_HD uint32_t bi_span_first(uint32_t s) { return s & 0x7fffu; }
BI_HD uint32_t bi_span_last(uint32_t s) { return s >> 15 & 0x7fffu; }
BI_HD bool bi_span_mapped(uint32_t s) { return (s >> 30 & 3u) == 3u; }
// the virtual file offset of position r of the sorted array; coff holds n_blocks + 1 values
BI_HD uint64_t bi_voff(uint64_t r, uint64_t n_raw, const uint64_t *coff, uint64_t n_blocks)
{
    if (r >= n_raw) return coff[n_blocks] << 16;
    return coff[r / BI_BLOCK] << 16 | r % BI_BLOCK;
}
// a chunk begins at record i: the first record, or another (refID, bin) than the record before; unplaced records begin none
BI_HD bool bi_is_head(uint64_t key_before, uint64_t key, bool first) { return key != BI_NONE && (first || key != key_before); }
// two neighbouring chunks of one bin become one
BI_HD bool bi_merges(uint64_t prev_end, uint64_t next_beg) { return prev_end >> 16 >= next_beg >> 16; }
// the linear index's fill: a window keeps its own value, an empty one takes what lies to its left
BI_HD uint64_t bi_fill(uint64_t left, uint64_t own) { return own != BI_NONE ? own : left; }
// window w lies in the span [first, last] of the mapped record in front (first > last: there is none): that record's start is the smaller offset
BI_HD bool bi_lin_covered(uint32_t w, uint32_t first, uint32_t last) { return w >= first && w <= last; }
// ---- where things lie in the file.  A reference with n_bins bins (without the pseudo-bin) and n_chunks merged chunks: ----
BI_HD uint64_t bi_ref_bytes(uint64_t n_bins, uint64_t n_chunks, bool has_records, uint64_t n_intv) { return 4 + 8 * n_bins + 16 * n_chunks + (has_records ? 40u : 0u) + 4 + 8 * n_intv; }
// bin number `bin_in_ref` of the reference, `chunks_before` merged chunks of the reference in front of its first
BI_HD uint64_t bi_bin_at(uint64_t ref_at, uint64_t bin_in_ref, uint64_t chunks_before) { return ref_at + 4 + 8 * bin_in_ref + 16 * chunks_before; }
// merged chunk number `chunk_in_ref` of the reference, in its bin number `bin_in_ref`
BI_HD uint64_t bi_chunk_at(uint64_t ref_at, uint64_t bin_in_ref, uint64_t chunk_in_ref) { return ref_at + 4 + 8 * (bin_in_ref + 1) + 16 * chunk_in_ref; }
BI_HD uint64_t bi_pseudo_at(uint64_t ref_at, uint64_t n_bins, uint64_t n_chunks) { return ref_at + 4 + 8 * n_bins + 16 * n_chunks; }
BI_HD uint64_t bi_intv_at(uint64_t ref_at, uint64_t n_bins, uint64_t n_chunks, bool has_records) { return bi_pseudo_at(ref_at, n_bins, n_chunks) + (has_records ? 40u : 0u); }
// dword stores into the dword-aligned output of `cap` bytes: nothing is ever written behind it
BI_HD void bi_put32(unsigned char *out, uint64_t cap, uint64_t at, uint32_t v) { if (at + 4 <= cap) *(uint32_t *)(out + at) = v; }
BI_HD void bi_put64(unsigned char *out, uint64_t cap, uint64_t at, uint64_t v) { bi_put32(out, cap, at, (uint32_t)v); bi_put32(out, cap, at + 4, (uint32_t)(v >> 32)); }
// a reference's fixed parts: n_bin, the pseudo-bin, n_intv (its bins and chunks, and the windows, go out elsewhere); ref = the reference's BI_REF_PLANES values
BI_HD void bi_put_ref(unsigned char *out, uint64_t cap, uint64_t ref_at, uint64_t n_bins, uint64_t n_chunks, const uint64_t ref[BI_REF_PLANES], uint64_t voff_first, uint64_t voff_last_end)
{
    const bool has = ref[1] + ref[2] > 0;
    bi_put32(out, cap, ref_at, (uint32_t)(n_bins + (has ? 1u : 0u)));
    if (has) {
        const uint64_t p = bi_pseudo_at(ref_at, n_bins, n_chunks);
        bi_put32(out, cap, p, BI_PSEUDO_BIN); bi_put32(out, cap, p + 4, 2u);
        bi_put64(out, cap, p + 8, voff_first); bi_put64(out, cap, p + 16, voff_last_end);
        bi_put64(out, cap, p + 24, ref[1]); bi_put64(out, cap, p + 32, ref[2]);
    }
    bi_put32(out, cap, bi_intv_at(ref_at, n_bins, n_chunks, has), (uint32_t)ref[0]);
}
BI_HD void bi_put_head(unsigned char *out, uint64_t cap, int n_chr, uint64_t total, uint64_t n_no_coor)
{
    bi_put32(out, cap, 0, 0x01494142u);                        // "BAI\1"
    bi_put32(out, cap, 4, (uint32_t)n_chr);
    bi_put64(out, cap, total - 8, n_no_coor);
}
// the most bytes an index of n_chunks chunks (before the merge) and n_intv windows in all takes
BI_HD uint64_t bi_bytes_bound(uint64_t n_chr, uint64_t n_chunks, uint64_t n_intv) { return 16 + 48 * n_chr + 24 * n_chunks + 8 * n_intv; }

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BI_THREADS)
k_bi_coff(const uint32_t *__restrict__ sizes, uint32_t n_blocks, unsigned long long first, uint64_t *__restrict__ coff, unsigned long long *__restrict__ stat)
{
    __shared__ uint64_t s_wave[BI_THREADS / 64];
    uint64_t carry = first;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += BI_THREADS) {
        const uint32_t k = b0 + threadIdx.x;
        const uint64_t mine = k < n_blocks ? (uint64_t)sizes[k] : 0ull;
        uint64_t all;
        const uint64_t ex = d_wg_exclusive(mine, all, s_wave);
        if (k < n_blocks) coff[k] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0) { coff[n_blocks] = carry; stat[BI_ST_COFF_END] = carry; }
}

__global__ void __launch_bounds__(BI_THREADS)
k_bi_rec(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw,
         const uint64_t *__restrict__ coff, uint32_t n_blocks, int n_chr, uint64_t *__restrict__ key, uint64_t *__restrict__ voff, uint32_t *__restrict__ span,
         unsigned long long *__restrict__ ref /* BI_REF_PLANES x n_chr */, unsigned long long *__restrict__ stat)
{
    const uint32_t i = blockIdx.x * BI_THREADS + threadIdx.x, lane = threadIdx.x & 63u;
    bool placed = false, bad = false;
    int32_t refid = -1;
    unsigned long long windows = 0, mapped = 0, unmapped = 0, lo = BI_NONE, hi = 0;
    if (i < n) {
        const uint64_t at = bam_rec_start(dst_off, tile_base, i);
        BiRec r; r.placed = false;
        if (at < n_raw) r = bi_record(sorted + at, n_raw - at, n_chr);
        key[i] = r.placed ? bi_key(r) : BI_NONE;
        voff[i] = bi_voff(at, n_raw, coff, n_blocks);
        span[i] = r.placed ? bi_span(r) : 0u;
        if (r.placed) {
            placed = true; refid = r.refid; bad = r.end > BI_MAX_END;
            if (r.mapped) { mapped = 1; if (!bad) windows = (unsigned long long)((r.end - 1) >> 14) + 1ull; } else unmapped = 1;
            lo = hi = i;
        }
    }
    if (i == n - 1u) voff[n] = bi_voff(n_raw, n_raw, coff, n_blocks);
    if (bad) atomicMin(stat + BI_ST_BAD, (unsigned long long)i);
    // the array is sorted by reference: nearly every wave holds one reference, and then one lane speaks for all
    const unsigned long long m = __ballot(placed);
    if (!m) return;
    const int leader = __ffsll((long long)m) - 1;
    const int32_t lref = __shfl(refid, leader, 64);
    if (__all(!placed || refid == lref)) {
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long w2 = __shfl_xor(windows, o, 64), l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
            windows = w2 > windows ? w2 : windows; lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
            mapped += __shfl_xor(mapped, o, 64); unmapped += __shfl_xor(unmapped, o, 64);
        }
        placed = (int)lane == leader;
    }
    if (placed) {
        unsigned long long *p = ref + refid;
        if (windows) atomicMax(p, windows);
        if (mapped) atomicAdd(p + n_chr, mapped);
        if (unmapped) atomicAdd(p + 2 * (size_t)n_chr, unmapped);
        atomicMin(p + 3 * (size_t)n_chr, lo); atomicMax(p + 4 * (size_t)n_chr, hi);
    }
}

__device__ __forceinline__ uint32_t bi_head_flag(const uint64_t *key, uint32_t i, uint32_t n)
{
    return i < n && bi_is_head(i ? key[i - 1] : BI_NONE, key[i], i == 0) ? 1u : 0u;
}
__global__ void __launch_bounds__(BI_THREADS)
k_bi_heads(const uint64_t *__restrict__ key, uint32_t n, uint32_t *__restrict__ tile_cnt)
{
    __shared__ uint32_t s_wave[BI_THREADS / 64];
    uint32_t all;
    (void)d_wg_exclusive(bi_head_flag(key, blockIdx.x * BI_THREADS + threadIdx.x, n), all, s_wave);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = all;
}

// lin_at[t]: where reference t's windows begin in lin
__global__ void __launch_bounds__(BI_THREADS)
k_bi_lin(const uint64_t *__restrict__ key, const uint32_t *__restrict__ span, const uint64_t *__restrict__ voff, uint32_t n, int n_chr, const uint64_t *__restrict__ lin_at,
         unsigned long long *__restrict__ lin)
{
    const uint32_t i = blockIdx.x * BI_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = span[i];
    if (!bi_span_mapped(s)) return;
    const uint64_t t = key[i] >> 16;
    if (t >= (uint64_t)n_chr) return;
    const uint64_t base = lin_at[t], limit = lin_at[t + 1], v = voff[i];
    // a window the mapped record in front covers too (same reference) is not this record's: that record's offset is smaller, and it, or one further in
    // front, stores it.  Under deep coverage this leaves about one atomic per window instead of one per record and window.
    uint32_t skip_first = 1u, skip_last = 0u;
    if (i) { const uint32_t p = span[i - 1]; if (bi_span_mapped(p) && key[i - 1] >> 16 == t) { skip_first = bi_span_first(p); skip_last = bi_span_last(p); } }
    for (uint32_t w = bi_span_first(s); w <= bi_span_last(s); w++)
        if (!bi_lin_covered(w, skip_first, skip_last) && base + w < limit) atomicMin(lin + base + w, (unsigned long long)v);
}

// The head flags and their workgroup scan are computed a second time here rather than kept from k_bi_heads: the chunk count has to reach the host between
// the two kernels (it sizes the chunk arrays), and recomputing reads the 8-byte keys the flags come from once more, where keeping the per-lane places would
// write and read 4 more bytes per record and hold them in HBM across the wait.
// tile_base: k_bi_heads' counts, scanned; chunk c (file order) gets the pair (key, c) and its first record; chead[n_chunks] = n_placed closes the last chunk
__global__ void __launch_bounds__(BI_THREADS)
k_bi_chunks(const uint64_t *__restrict__ key, uint32_t n, const uint32_t *__restrict__ tile_base, uint32_t n_chunks, uint32_t n_placed,
            uint64_t *__restrict__ ckey, int64_t *__restrict__ cval, uint32_t *__restrict__ chead)
{
    __shared__ uint32_t s_wave[BI_THREADS / 64];
    const uint32_t i = blockIdx.x * BI_THREADS + threadIdx.x, h = bi_head_flag(key, i, n);
    uint32_t all;
    const uint32_t c = tile_base[blockIdx.x] + d_wg_exclusive(h, all, s_wave);
    if (h && c < n_chunks) { ckey[c] = key[i]; cval[c] = (int64_t)c; chead[c] = i; }
    if (i == 0) chead[n_chunks] = n_placed;
}

// sorted chunk j is chunk c = sval[j] of the file: from voff of its first record to voff of the next chunk's first record
__device__ __forceinline__ uint64_t bi_chunk_beg(const uint64_t *voff, const uint32_t *chead, const int64_t *sval, uint32_t j) { return voff[chead[sval[j]]]; }
__device__ __forceinline__ uint64_t bi_chunk_end(const uint64_t *voff, const uint32_t *chead, const int64_t *sval, uint32_t j) { return voff[chead[sval[j] + 1]]; }

// flag bit 0: sorted chunk j begins a merged chunk; bit 1: it begins a bin.  The two counts are scanned in one word: bins << 32 | merged chunks
__global__ void __launch_bounds__(BI_THREADS)
k_bi_merge_scan(const uint64_t *__restrict__ skey, const int64_t *__restrict__ sval, const uint32_t *__restrict__ chead, const uint64_t *__restrict__ voff, uint32_t n_chunks,
                unsigned char *__restrict__ flag, uint64_t *__restrict__ excl, uint64_t *__restrict__ tile_sum)
{
    __shared__ uint64_t s_wave[BI_THREADS / 64];
    const uint32_t j = blockIdx.x * BI_THREADS + threadIdx.x;
    uint32_t f = 0;
    if (j < n_chunks) {
        const bool bin_head = j == 0 || skey[j] != skey[j - 1];
        const bool merged = !bin_head && bi_merges(bi_chunk_end(voff, chead, sval, j - 1), bi_chunk_beg(voff, chead, sval, j));
        f = (merged ? 0u : 1u) | (bin_head ? 2u : 0u);
    }
    uint64_t all;
    const uint64_t ex = d_wg_exclusive((uint64_t)(f & 1u) | (uint64_t)(f >> 1) << 32, all, s_wave);
    if (j < n_chunks) { flag[j] = (unsigned char)f; excl[j] = ex; }
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// ref_q[t] / ref_b[t]: the merged chunks / bins of all references before t (n_chr + 1 values each)
__global__ void __launch_bounds__(BI_THREADS)
k_bi_merge_emit(const uint64_t *__restrict__ skey, const unsigned char *__restrict__ flag, const uint64_t *__restrict__ excl, const uint64_t *__restrict__ tile_base, uint32_t n_chunks,
                int n_chr, const unsigned long long *__restrict__ stat, uint32_t *__restrict__ mhead, uint32_t *__restrict__ mbin, uint32_t *__restrict__ binq,
                uint32_t *__restrict__ ref_q, uint32_t *__restrict__ ref_b)
{
    const uint32_t j = blockIdx.x * BI_THREADS + threadIdx.x;
    if (j >= n_chunks) return;
    const uint64_t at = tile_base[blockIdx.x] + excl[j];
    const uint32_t f = flag[j], q = (uint32_t)at, b = (uint32_t)(at >> 32);       // the merged chunks and the bins in front of j
    if ((f & 1u) && q < n_chunks) { mhead[q] = j; mbin[q] = b + (f >> 1) - 1u; }
    if ((f & 2u) && b < n_chunks) binq[b] = q;
    const int64_t t = (int64_t)(skey[j] >> 16), before = j ? (int64_t)(skey[j - 1] >> 16) : -1;
    for (int64_t x = before + 1; x <= t && x <= (int64_t)n_chr; x++) { ref_q[x] = q; ref_b[x] = b; }
    if (j == n_chunks - 1u) {
        const uint32_t all_q = (uint32_t)stat[BI_ST_MERGED], all_b = (uint32_t)(stat[BI_ST_MERGED] >> 32);
        for (int64_t x = t + 1; x <= (int64_t)n_chr; x++) { ref_q[x] = all_q; ref_b[x] = all_b; }
        if (all_b < n_chunks + 1u) binq[all_b] = all_q;
        if (all_q < n_chunks + 1u) mhead[all_q] = n_chunks;
    }
}

__global__ void __launch_bounds__(BI_THREADS)
k_bi_refs(int n_chr, const unsigned long long *__restrict__ ref, const uint32_t *__restrict__ ref_q, const uint32_t *__restrict__ ref_b, unsigned long long n_no_coor,
          uint64_t *__restrict__ ref_at, unsigned char *__restrict__ out, unsigned long long cap, unsigned long long *__restrict__ stat)
{
    __shared__ uint64_t s_wave[BI_THREADS / 64];
    uint64_t carry = 8;
    for (int t0 = 0; t0 < n_chr; t0 += BI_THREADS) {
        const int t = t0 + (int)threadIdx.x;
        uint64_t mine = 0;
        if (t < n_chr) mine = bi_ref_bytes(ref_b[t + 1] - ref_b[t], ref_q[t + 1] - ref_q[t], ref[n_chr + t] + ref[2 * (size_t)n_chr + t] > 0, ref[t]);
        uint64_t all;
        const uint64_t ex = d_wg_exclusive(mine, all, s_wave);
        if (t < n_chr) ref_at[t] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0) {
        ref_at[n_chr] = carry;
        stat[BI_ST_BYTES] = carry + 8;
        bi_put_head(out, cap, n_chr, carry + 8, n_no_coor);
    }
}

__global__ void __launch_bounds__(BI_THREADS)
k_bi_write_chunks(const uint64_t *__restrict__ skey, const int64_t *__restrict__ sval, const uint32_t *__restrict__ chead, const uint64_t *__restrict__ voff, uint32_t n_chunks,
                  const unsigned long long *__restrict__ stat, const uint32_t *__restrict__ mhead, const uint32_t *__restrict__ mbin, const uint32_t *__restrict__ binq,
                  const uint32_t *__restrict__ ref_q, const uint32_t *__restrict__ ref_b, const uint64_t *__restrict__ ref_at, int n_chr, unsigned char *__restrict__ out, unsigned long long cap)
{
    const uint32_t q = blockIdx.x * BI_THREADS + threadIdx.x, all_q = (uint32_t)stat[BI_ST_MERGED];
    if (q >= all_q || q >= n_chunks) return;
    const uint32_t j = mhead[q], j_next = mhead[q + 1], b = mbin[q];
    if (j >= n_chunks || j_next > n_chunks || j_next <= j || b >= n_chunks) return;
    const uint64_t t = skey[j] >> 16;
    if (t >= (uint64_t)n_chr) return;
    const uint64_t at = ref_at[t], bin_in_ref = b - ref_b[t], chunk_in_ref = q - ref_q[t];
    const uint64_t c = bi_chunk_at(at, bin_in_ref, chunk_in_ref);
    bi_put64(out, cap, c, bi_chunk_beg(voff, chead, sval, j));
    bi_put64(out, cap, c + 8, bi_chunk_end(voff, chead, sval, j_next - 1u));
    if (binq[b] == q) {
        const uint64_t h = bi_bin_at(at, bin_in_ref, chunk_in_ref);
        bi_put32(out, cap, h, (uint32_t)(skey[j] & 0xffffu));
        bi_put32(out, cap, h + 4, binq[b + 1] - q);
    }
}

// the fill is a last-valid scan over the reference's windows, a workgroup's 256 at a time; what is carried in front of window 0 is the reference's first record's start
__global__ void __launch_bounds__(BI_THREADS)
k_bi_write_refs(int n_chr, const unsigned long long *__restrict__ ref, const uint32_t *__restrict__ ref_q, const uint32_t *__restrict__ ref_b, const uint64_t *__restrict__ ref_at,
                const uint64_t *__restrict__ voff, uint32_t n, const uint64_t *__restrict__ lin_at, const unsigned long long *__restrict__ lin, unsigned char *__restrict__ out, unsigned long long cap)
{
    __shared__ uint64_t s_last[BI_THREADS / 64];
    const int t = (int)blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint64_t r[BI_REF_PLANES];
    for (int p = 0; p < BI_REF_PLANES; p++) r[p] = ref[(size_t)p * n_chr + t];
    const bool has = r[1] + r[2] > 0;
    const uint64_t n_bins = ref_b[t + 1] - ref_b[t], n_chunks = ref_q[t + 1] - ref_q[t], at = ref_at[t];
    uint64_t first = 0, last_end = 0;
    if (has && r[3] < n && r[4] < n) { first = voff[r[3]]; last_end = voff[r[4] + 1]; }
    if (threadIdx.x == 0) bi_put_ref(out, cap, at, n_bins, n_chunks, r, first, last_end);
    const uint64_t base = lin_at[t], n_intv = lin_at[t + 1] - base, dst = bi_intv_at(at, n_bins, n_chunks, has) + 4;
    uint64_t carry = first;
    for (uint64_t w0 = 0; w0 < n_intv; w0 += BI_THREADS) {
        const uint64_t w = w0 + threadIdx.x;
        uint64_t v = w < n_intv ? (uint64_t)lin[base + w] : BI_NONE;
        for (int o = 1; o < 64; o <<= 1) { const uint64_t left = __shfl_up(v, o, 64); if (lane >= (uint32_t)o) v = bi_fill(left, v); }
        if (lane == 63u) s_last[wv] = v;
        __syncthreads();
        uint64_t before = carry, all = carry;
        for (uint32_t k = 0; k < BI_THREADS / 64; k++) { all = bi_fill(all, s_last[k]); if (k < wv) before = all; }
        v = bi_fill(before, v);
        if (w < n_intv) bi_put64(out, cap, dst + 8 * w, v);
        carry = all;
        __syncthreads();
    }
}
#endif
#endif
