// dg_fastq.h -- FASTQ text on the device: the bytes of one or two read files -> the batch the mapping kernels and the SAM formatter read (ASCII bases at
// seq_off[], rlen[], names at hdr_off[], stored qualities at qual_off[]).  This is GetNextEntry / GetNextChunk (GetData.cpp:77-179) for a range of whole
// records: a record is four lines, whatever they hold.  The rules are stated once, in __host__ __device__ functions that the kernels below and the CPU
// suite (tests/native/fastq_checks.hip) share:
//   k_fq_count   a thread takes 16 bytes at a time: newlines per tile of FQ_TILE bytes
//   k_fq_top     one workgroup: exclusive scan of the tile counts, the lines and records of each text, the number of reads
//   k_fq_lines   the same tiling: every newline writes the start of the line behind it to line_start[line number]
//   k_fq_len     lane = read: name length, read length, quality length; the first read without bases / longer than DG_MAX_RLEN; every workgroup leaves the
//                exclusive scans of its 256 x 3 lengths and their sums
//   k_fq_top3    one workgroup: exclusive scans of the workgroup sums (64 bit), the totals, the status
//   k_fq_write   wave = read: bases (reverse-complemented for a stored mate 2), name and quality (reversed for a stored mate 2) lane beside lane
// A text that is a piece of a file (dg_batch_upload_fastq_bgzf without `last`: the blocks of a compressed file do not end where records end) is taken in
// whole records -- four lines, each ended by its newline; two texts give the same number of records, the smaller of the two counts -- by k_fq_top's `whole`
// mode; what lies behind the last record taken is the text's tail:
//   k_fq_tail    where each text's tail begins, and its bytes into a buffer of their own (the next call's head)
//   k_fq_unlike  wave = read: counts the records the reference's gz reader (gzgets into 1024 bytes) and its plain reader would read differently
// Plain scans in launches (no look-back: an upload never runs twice).  Every byte's place follows from the scanned lengths alone, so the batch is the
// same whatever the grid.
#ifndef DG_FASTQ_H
#define DG_FASTQ_H
#include "../../include/dartgpu.h"
#include "dg_wgscan.h"

#define FQ_HD __host__ __device__ __forceinline__

#define FQ_THREADS 256
static_assert(FQ_THREADS == WG_THREADS, "the kernels here scan with d_wg_exclusive");
#define FQ_ROUNDS 4
#define FQ_TILE DG_FASTQ_TILE                 // bytes of text per workgroup of k_fq_count / k_fq_lines: FQ_ROUNDS rounds of 256 threads x 16 bytes
static_assert(FQ_TILE == FQ_THREADS * 16 * FQ_ROUNDS, "a tile is FQ_ROUNDS rounds of 16 bytes per thread");

// ------------------------------------------------------------------------------------------
// the record rules
// ------------------------------------------------------------------------------------------
// 16 bytes of text (as four little-endian words) -> bit i set when byte i is '\n'; only the first `valid` bytes count
FQ_HD uint32_t fq_nl_nibble(uint32_t w)
{
    const uint32_t x = w ^ 0x0A0A0A0Au;                                              // a newline is now a zero byte
    const uint32_t m = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);       // 0x80 exactly where a byte is zero (no borrow between bytes)
    return (((m >> 7) * 0x00204081u) >> 21) & 15u;                                   // bits 0, 8, 16, 24 -> bits 0..3
}
FQ_HD uint32_t fq_nl_mask16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint64_t valid)
{
    const uint32_t m = fq_nl_nibble(w0) | (fq_nl_nibble(w1) << 4) | (fq_nl_nibble(w2) << 8) | (fq_nl_nibble(w3) << 12);
    return valid >= 16 ? m : m & ((1u << (uint32_t)valid) - 1u);
}
// IdentifyHeaderBegPos / IdentifyHeaderEndPos (GetData.cpp:55-75) over line 0 of `len` bytes (its newline included)
FQ_HD int64_t fq_hdr_beg(const char *s, int64_t len) { for (int64_t i = 1; i < len; i++) if (s[i] != '>' && s[i] != '@') return i; return len - 1; }
FQ_HD int64_t fq_hdr_end(const char *s, int64_t len) { for (int64_t i = 1; i < len; i++) if (s[i] == ' ' || s[i] == '/' || s[i] == '\t') return i; return len - 1; }
// comp_base (tools.cpp:3-17)
FQ_HD char fq_comp_base(char c)
{
    switch (c) {
    case 'A': case 'a': return 'T';
    case 'C': case 'c': return 'G';
    case 'G': case 'g': return 'C';
    case 'T': case 't': return 'A';
    default: return 'N';
    }
}
// One record from the lengths of its four lines (a line = its bytes up to and including '\n', or up to the end of the text; 0 = it does not exist) and the
// offset of line 0 in the text.  rlen <= 0: a record without bases (GetData.cpp:95-103: the line's length minus one).
struct FqRecord { uint32_t name_at, hl, seq_at, qual_at, ql; int64_t rlen; };
FQ_HD FqRecord fq_record(const char *text, uint64_t off, uint32_t l0, uint32_t l1, uint32_t l2, uint32_t l3)
{
    FqRecord r;
    const int64_t p1 = fq_hdr_beg(text + off, (int64_t)l0), p2 = fq_hdr_end(text + off, (int64_t)l0);
    r.name_at = (uint32_t)(off + (uint64_t)(p1 > 0 ? p1 : 0)); r.hl = p2 > p1 ? (uint32_t)(p2 - p1) : 0u;
    r.rlen = (int64_t)l1 - 1;
    r.seq_at = (uint32_t)(off + l0); r.qual_at = (uint32_t)(off + l0 + l1 + l2);
    r.ql = r.rlen > 0 ? (uint32_t)(r.rlen < (int64_t)l3 ? r.rlen : (int64_t)l3) : 0u;      // the quality is cut to the read's length (GetData.cpp:100-101)
    return r;
}
// read k of the batch = record `rec` of text `file`: with two texts the reads alternate (GetNextChunk, GetData.cpp:141,152)
FQ_HD void fq_read_place(uint32_t k, bool two, int &file, uint32_t &rec) { file = two ? (int)(k & 1u) : 0; rec = two ? k >> 1 : k; }
// reads of a batch from the records of its texts: -1 when the counts do not fit (two texts: equal, or text 1 holds one more -- the stream's last read)
FQ_HD int64_t fq_read_count(bool two, uint64_t rec1, uint64_t rec2)
{
    if (!two) return (int64_t)rec1;
    if (rec1 == rec2) return (int64_t)(2 * rec1);
    if (rec1 == rec2 + 1) return (int64_t)(2 * rec2 + 1);
    return -1;
}
// whole records only: a text with `nl` newlines holds nl / 4 of them; two texts give the smaller count each
FQ_HD uint64_t fq_whole_records(bool two, uint64_t nl1, uint64_t nl2) { const uint64_t a = nl1 / 4, b = nl2 / 4; return !two ? a : a < b ? a : b; }
// Would the reference's gz reader (gzGetNextEntry, GetData.cpp:181-210: gzgets into 1024 bytes, strlen) read this record as its plain reader does?  The rules
// of the host program's gz_reader_sees_the_same on the four line lengths (newlines included, 0 = the line does not exist); a NUL in the record is the caller's.
FQ_HD bool fq_gz_reader_same(const char *text, uint64_t off, uint32_t l0, uint32_t l1, uint32_t l2, uint32_t l3)
{
    if (!(l0 >= 2u && l1 >= 2u && l2 >= 1u && l3 >= 1u && l0 < 1024u && l1 < 1024u && l2 < 1024u && l3 < 1024u && text[off] == '@')) return false;
    return fq_hdr_end(text + off, (int64_t)l0) - fq_hdr_beg(text + off, (int64_t)l0) > 0;       // the name must not be empty (GetData.cpp:194)
}
FQ_HD bool fq_stored_rc(uint32_t k, int rc_odd_reads) { return rc_odd_reads && (k & 1u); }
// byte i of the stored read / the stored quality (GetData.cpp:157-166: an odd read of a pair is kept reverse-complemented, its quality reversed)
FQ_HD char fq_stored_base(const char *line1, uint32_t rlen, uint32_t i, bool rc) { return rc ? fq_comp_base(line1[rlen - 1u - i]) : line1[i]; }
FQ_HD char fq_stored_qual(const char *line3, uint32_t ql, uint32_t i, bool rc) { return rc ? line3[ql - 1u - i] : line3[i]; }

// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
enum { FQ_OK = 0, FQ_E_COUNT = 1, FQ_E_CAPACITY = 2, FQ_E_EMPTY = 3, FQ_E_LONG = 4, FQ_E_OFFSETS = 5 };
// the sizes block the host waits for
struct FqInfo {
    unsigned long long total[3];           // bases, name bytes, quality bytes
    uint32_t n_nl[2], n_lines[2];          // per text: newlines; lines (a last line without '\n' counts)
    uint32_t n_reads, max_rlen, status, bad_read, bad_long, pad;
    uint32_t tail_at[2], n_unlike, pad2;   // whole-record mode: where each text's tail begins; records the reference's gz reader would read differently
};
struct FqText {
    const unsigned char *t[2]; uint32_t n[2];      // the texts in HBM (16-byte aligned, readable up to the next multiple of 16) and their lengths
    uint32_t *line_start[2]; uint32_t line_cap[2]; // line_start[i] = offset of line i; entries [0, line_cap)
    int two;
};

__device__ __forceinline__ uint32_t fq_load_mask(const unsigned char *t, uint64_t pos, uint64_t n)
{
    if (pos >= n) return 0u;
    const uint4 v = *reinterpret_cast<const uint4 *>(t + pos);
    return fq_nl_mask16(v.x, v.y, v.z, v.w, n - pos);
}

__global__ void __launch_bounds__(FQ_THREADS)
k_fq_count(const FqText x, uint32_t *__restrict__ tile_cnt, uint32_t tile_stride)
{
    __shared__ uint32_t s_w[FQ_THREADS / 64];
    const int f = (int)blockIdx.y;
    const uint64_t n = x.n[f], base = (uint64_t)blockIdx.x * FQ_TILE;
    if (base >= n) return;
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < FQ_ROUNDS; j++) cnt += (uint32_t)__popc(fq_load_mask(x.t[f], base + ((uint64_t)j * FQ_THREADS + threadIdx.x) * 16u, n));
    uint32_t total;
    (void)d_wg_exclusive<uint32_t>(cnt, total, s_w);
    if (threadIdx.x == 0) tile_cnt[(size_t)f * tile_stride + blockIdx.x] = total;
}

// tile_cnt becomes its exclusive scan; info: lines per text, the number of reads, FQ_E_COUNT / FQ_E_CAPACITY
// whole: the texts are pieces of files: whole records only, the same number from each text; n_lines becomes the lines of the records taken
__global__ void __launch_bounds__(FQ_THREADS)
k_fq_top(const FqText x, uint32_t *__restrict__ tile_cnt, uint32_t tile_stride, uint32_t max_reads, FqInfo *__restrict__ info, int whole)
{
    __shared__ uint32_t s_w[FQ_THREADS / 64];
    __shared__ uint32_t s_lines[2];
    for (int f = 0; f < (x.two ? 2 : 1); f++) {
        const uint32_t n_tiles = (uint32_t)(((uint64_t)x.n[f] + FQ_TILE - 1) / FQ_TILE);
        const uint32_t carry = d_tiles_exclusive<uint32_t>(tile_cnt + (size_t)f * tile_stride, n_tiles, 1, s_w);
        if (threadIdx.x == 0) {
            const uint32_t lines = carry + ((x.n[f] && x.t[f][x.n[f] - 1] != '\n') ? 1u : 0u);
            info->n_nl[f] = carry; info->n_lines[f] = lines; s_lines[f] = lines;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (!x.two) { info->n_nl[1] = 0; info->n_lines[1] = 0; s_lines[1] = 0; }
        uint64_t rec1 = ((uint64_t)s_lines[0] + 3) / 4, rec2 = ((uint64_t)s_lines[1] + 3) / 4;
        if (whole) {
            rec1 = fq_whole_records(x.two != 0, info->n_nl[0], info->n_nl[1]); rec2 = x.two ? rec1 : 0;
            info->n_lines[0] = (uint32_t)(4 * rec1); info->n_lines[1] = (uint32_t)(4 * rec2);
        }
        const int64_t n = fq_read_count(x.two != 0, rec1, rec2);
        uint32_t status = FQ_OK;
        if (n < 0) status = FQ_E_COUNT;
        else if ((uint64_t)n > max_reads) status = FQ_E_CAPACITY;
        info->n_reads = n < 0 ? 0u : (uint32_t)(n > 0xFFFFFFFFll ? 0xFFFFFFFFll : n);
        info->status = status; info->max_rlen = 0; info->bad_read = 0xFFFFFFFFu; info->bad_long = 0xFFFFFFFFu; info->pad = 0;
        info->total[0] = info->total[1] = info->total[2] = 0;
        info->tail_at[0] = x.n[0]; info->tail_at[1] = x.two ? x.n[1] : 0u; info->n_unlike = 0; info->pad2 = 0;
    }
}

__global__ void __launch_bounds__(FQ_THREADS)
k_fq_lines(const FqText x, const uint32_t *__restrict__ tile_off, uint32_t tile_stride, const FqInfo *__restrict__ info)
{
    __shared__ uint32_t s_w[FQ_THREADS / 64];
    if (info->status != FQ_OK) return;
    const int f = (int)blockIdx.y;
    const uint64_t n = x.n[f], base = (uint64_t)blockIdx.x * FQ_TILE;
    if (base >= n) return;
    uint32_t *ls = x.line_start[f];
    const uint32_t cap = x.line_cap[f];
    if (blockIdx.x == 0 && threadIdx.x == 0 && cap) ls[0] = 0;
    uint32_t line = tile_off[(size_t)f * tile_stride + blockIdx.x] + 1u;       // the line behind the tile's first newline
#pragma unroll 1
    for (int j = 0; j < FQ_ROUNDS; j++) {
        const uint64_t pos = base + ((uint64_t)j * FQ_THREADS + threadIdx.x) * 16u;
        uint32_t m = fq_load_mask(x.t[f], pos, n);
        uint32_t total;
        uint32_t at = line + d_wg_exclusive<uint32_t>((uint32_t)__popc(m), total, s_w);
        while (m) {
            const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
            m &= m - 1u;
            if (at < cap) ls[at] = (uint32_t)(pos + b + 1u);
            at++;
        }
        line += total;
    }
}

// the lengths of line i of text f, and where it starts (0 / 0 when it does not exist)
__device__ __forceinline__ uint32_t fq_dev_line(const FqText &x, const FqInfo *info, int f, uint64_t i, uint32_t &start)
{
    if (i >= info->n_lines[f]) { start = 0; return 0u; }
    start = x.line_start[f][i];
    const uint32_t end = i < info->n_nl[f] ? x.line_start[f][i + 1] : x.n[f];
    return end - start;
}

// whole-record mode, behind k_fq_lines: text f's tail begins behind the last line taken; its bytes go to tail (text 2's at tail_off2)
__global__ void __launch_bounds__(FQ_THREADS)
k_fq_tail(const FqText x, FqInfo *info, unsigned char *__restrict__ tail, uint32_t tail_off2)
{
    if (info->status != FQ_OK) return;
    const int f = (int)blockIdx.y;
    if (f && !x.two) return;
    const uint32_t taken = info->n_lines[f];
    const uint32_t at = taken ? x.line_start[f][taken] : 0u;          // (taken <= the text's newlines: the entry exists, and taken < line_cap)
    if (blockIdx.x == 0 && threadIdx.x == 0) info->tail_at[f] = at;
    unsigned char *dst = tail + (f ? tail_off2 : 0u);
    for (uint64_t i = (uint64_t)at + blockIdx.x * FQ_THREADS + threadIdx.x; i < x.n[f]; i += (uint64_t)gridDim.x * FQ_THREADS) dst[i - at] = x.t[f][i];
}

// One wave per read, behind k_fq_lines: the record's four lines against fq_gz_reader_same, its bytes against NUL
__global__ void __launch_bounds__(64)
k_fq_unlike(const FqText x, FqInfo *info)
{
    if (info->status != FQ_OK) return;
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (k >= info->n_reads) return;
    int f; uint32_t rec;
    fq_read_place(k, x.two != 0, f, rec);
    uint32_t s0, s1, s2, s3;
    const uint32_t l0 = fq_dev_line(x, info, f, 4ull * rec, s0), l1 = fq_dev_line(x, info, f, 4ull * rec + 1, s1);
    const uint32_t l2 = fq_dev_line(x, info, f, 4ull * rec + 2, s2), l3 = fq_dev_line(x, info, f, 4ull * rec + 3, s3);
    const char *t = (const char *)x.t[f];
    bool nul = false;
    for (uint32_t i = lane; i < l0 + l1 + l2 + l3; i += 64) nul |= t[s0 + i] == 0;      // (the lines of a record lie one behind the other)
    const bool bad = __any(nul) || !fq_gz_reader_same(t, s0, l0, l1, l2, l3);
    if (lane == 0 && bad) atomicAdd(&info->n_unlike, 1u);
}

// loc / tile_sum hold three rows (bases, name bytes, quality bytes) of `stride` / n_tiles entries
__global__ void __launch_bounds__(FQ_THREADS)
k_fq_len(const FqText x, FqInfo *info, uint16_t *__restrict__ rlen_out, uint32_t *__restrict__ name_at, uint32_t *__restrict__ name_len,
         uint32_t *__restrict__ loc, uint32_t stride, unsigned long long *__restrict__ tile_sum, uint32_t n_tiles)
{
    __shared__ uint32_t s_w[FQ_THREADS / 64];
    if (info->status != FQ_OK) return;
    const uint32_t n_reads = info->n_reads;
    const uint32_t k = blockIdx.x * FQ_THREADS + threadIdx.x;
    if (blockIdx.x * FQ_THREADS >= n_reads) { if (threadIdx.x < 3) tile_sum[(size_t)threadIdx.x * n_tiles + blockIdx.x] = 0ull; return; }
    uint32_t len[3] = {0u, 0u, 0u};
    if (k < n_reads) {
        int f; uint32_t rec;
        fq_read_place(k, x.two != 0, f, rec);
        uint32_t s0, s1, s2, s3;
        const uint32_t l0 = fq_dev_line(x, info, f, 4ull * rec, s0), l1 = fq_dev_line(x, info, f, 4ull * rec + 1, s1);
        const uint32_t l2 = fq_dev_line(x, info, f, 4ull * rec + 2, s2), l3 = fq_dev_line(x, info, f, 4ull * rec + 3, s3);
        const FqRecord r = fq_record((const char *)x.t[f], s0, l0, l1, l2, l3);
        bool good = true;
        if (r.rlen <= 0) { atomicMin(&info->bad_read, k); good = false; }
        else if (r.rlen > DG_MAX_RLEN) { atomicMin(&info->bad_long, k); good = false; }
        if (good) { len[0] = (uint32_t)r.rlen; len[1] = r.hl; len[2] = r.ql; }
        rlen_out[k] = (uint16_t)len[0];
        name_at[k] = r.name_at; name_len[k] = len[1];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        uint32_t total;
        const uint32_t ex = d_wg_exclusive<uint32_t>(len[i], total, s_w);
        if (k < n_reads) loc[(size_t)i * stride + k] = ex;
        if (threadIdx.x == 0) tile_sum[(size_t)i * n_tiles + blockIdx.x] = total;
    }
    const uint32_t mx = d_wave_max(len[0]);
    if ((threadIdx.x & 63u) == 0 && mx) atomicMax(&info->max_rlen, mx);
}

__global__ void __launch_bounds__(FQ_THREADS)
k_fq_top3(unsigned long long *__restrict__ tile_sum, uint32_t n_tiles, FqInfo *__restrict__ info)
{
    __shared__ unsigned long long s_w[FQ_THREADS / 64];
    if (info->status != FQ_OK) return;
    const uint32_t used = (info->n_reads + FQ_THREADS - 1) / FQ_THREADS;
    const uint32_t nt = used < n_tiles ? used : n_tiles;
    for (int r = 0; r < 3; r++) {
        const unsigned long long total = d_tiles_exclusive<unsigned long long>(tile_sum + (size_t)r * n_tiles, nt, 1, s_w);
        if (threadIdx.x == 0) info->total[r] = total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t be = info->bad_read, bl = info->bad_long;
        if (be != 0xFFFFFFFFu && be < bl) info->status = FQ_E_EMPTY;
        else if (bl != 0xFFFFFFFFu) { info->status = FQ_E_LONG; info->bad_read = bl; }
        else if (info->total[0] > 0xFFFFFF00ull || info->total[1] > 0xFFFFFF00ull || info->total[2] > 0xFFFFFF00ull) info->status = FQ_E_OFFSETS;
    }
}

// One wave per workgroup, one workgroup per read.  Nothing is written when the status is raised.
__global__ void __launch_bounds__(64)
k_fq_write(const FqText x, const FqInfo *__restrict__ info, int rc_odd_reads, const uint16_t *__restrict__ rlen, const uint32_t *__restrict__ name_at,
           const uint32_t *__restrict__ name_len, const uint32_t *__restrict__ loc, uint32_t stride, const unsigned long long *__restrict__ tile_base, uint32_t n_tiles,
           uint32_t *__restrict__ seq_off, unsigned char *__restrict__ seq, uint32_t *__restrict__ hdr_off, char *__restrict__ hdr,
           uint32_t *__restrict__ qual_off, char *__restrict__ qual)
{
    if (info->status != FQ_OK) return;
    const uint32_t n_reads = info->n_reads, k = blockIdx.x, lane = threadIdx.x;
    if (k >= n_reads) return;
    const uint32_t tile = k / FQ_THREADS;
    const uint32_t so = (uint32_t)tile_base[tile] + loc[k], ho = (uint32_t)tile_base[(size_t)n_tiles + tile] + loc[(size_t)stride + k];
    const uint32_t qo = (uint32_t)tile_base[2 * (size_t)n_tiles + tile] + loc[2 * (size_t)stride + k];
    int f; uint32_t rec;
    fq_read_place(k, x.two != 0, f, rec);
    uint32_t s1, s3;
    (void)fq_dev_line(x, info, f, 4ull * rec + 1, s1);
    const uint32_t l3 = fq_dev_line(x, info, f, 4ull * rec + 3, s3);
    const uint32_t rl = rlen[k], hl = name_len[k], ql = rl < l3 ? rl : l3;
    const bool rc = fq_stored_rc(k, rc_odd_reads);
    const char *t = (const char *)x.t[f];
    const char *line1 = t + s1, *line3 = t + s3, *name = t + name_at[k];
    for (uint32_t i = lane; i < rl; i += 64) seq[so + i] = (unsigned char)fq_stored_base(line1, rl, i, rc);
    for (uint32_t i = lane; i < hl; i += 64) hdr[ho + i] = name[i];
    for (uint32_t i = lane; i < ql; i += 64) qual[qo + i] = fq_stored_qual(line3, ql, i, rc);
    if (lane == 0) { seq_off[k] = so; hdr_off[k] = ho; qual_off[k] = qo; }
    if (k == 0 && lane == 1) { seq_off[n_reads] = (uint32_t)info->total[0]; hdr_off[n_reads] = (uint32_t)info->total[1]; qual_off[n_reads] = (uint32_t)info->total[2]; }
}
#endif
