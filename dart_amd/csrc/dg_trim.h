// dg_trim.h -- adapters, poly tails and low-quality ends cut on the device, between "the lines are known" (k_fq_lines) and "the lengths are scanned": a window
// [a, b) per read, a keep flag per read, one more scanned row.  The definition is the comment on dg_set_trim in include/dartgpu.h; the rules are stated once,
// in __host__ __device__ functions that the kernels below and the CPU suite (tests/native/trim_checks.hip) share:
//   k_trim_cut    wave = read: the read's two lines straight from the text; the lanes pack the read into 2-bit codes and a not-ACGT mask in LDS (a ballot per
//                 bit plane, spread to the even bits); quality and poly walks are prefix sums across the wave with a carry between rounds of 64, their early
//                 stop a ballot; adapter: lane = start position p, the 64-base window is two unaligned 64-bit extracts of codes and two of the mask, the
//                 mismatches one xor, a fold and a popcount under the overlap mask, the first matching p a ballot.  Leaves one TrimRead per read.
//   k_trim_len    k_fq_len with the windows: the mate's verdict, a fourth scanned row (the keep flags), the sums of the statistics
//   k_trim_top3   k_fq_top3 with four rows; the kept count
//   k_trim_write  k_fq_write with the window and the compacted index; it also writes rlen[] (k_fq_len writes it at the input index)
// dg_set_umi puts one more cut in front: k_trim_cut starts u bases in, k_trim_len gives the pairwise verdict, the longer name and two sums, and k_trim_umi_name, a
// launch of its own behind k_trim_write when the rule is set, writes the suffix (inside k_trim_write it cost that kernel 14 spilled SGPRs and a wave of occupancy).
// The statistics are integer sums, so they -- like the batch -- are the same whatever the grid.
#ifndef DG_TRIM_H
#define DG_TRIM_H
#include "dg_fastq.h"

#define TR_WORDS 36                    // 64-bit words of a packed plane in LDS: 32 hold DG_MAX_RLEN bases at 2 bits, an extract at the last base reads two more
static_assert(DG_MAX_RLEN <= 1024 && (DG_MAX_RLEN * 2 + 64) / 64 + 2 <= TR_WORDS, "an unaligned extract behind the last base stays inside the plane");
#define TR_EVEN 0x5555555555555555ull
#define TR_QUAL_MAX 255u               // qual3, qual5, qual_base: sums of a walk stay far inside 32 bits

// the switches as the kernels take them: the adapters as 2-bit words (base j of adapter i at bits 2j, 2j + 1 of word j / 32)
struct TrimPar {
    uint32_t flags, qual3, qual5, qual_base, min_overlap, max_err_permille, poly_mask, poly_min, min_len, alen[2];
    uint64_t acode[2][2];
    uint32_t umi_on, umi_flags, umi_len[2], umi_skip[2], umi_sep;      // dg_set_umi: the inline UMI cut in front of the four steps
};
// what of them k_trim_write needs: the name's suffix
struct TrimUmi { uint32_t on, flags, len[2], sep; };
// what k_trim_cut leaves per read
enum { TR_F_ADAPTER = 1, TR_F_ADAPTER1 = 2, TR_F_POLY = 4, TR_F_QSKIP = 8, TR_F_KEEP = 16 };
struct TrimRead { uint16_t a, b, cut5, cut3, ad_cut, poly_cut, flags, umi_fail /* the read is too short for its UMI and linker (k_trim_len never writes it: the partner's lane reads it) */; };
static_assert(sizeof(TrimRead) == 16, "one 16-byte store per read");
struct TrimInfo { unsigned long long stats[16]; uint32_t n_kept, pad[3]; };

// ------------------------------------------------------------------------------------------
// the rules
// ------------------------------------------------------------------------------------------
// a base by its upper case: 0..3 = ACGT, 4 = anything else (equals nothing)
FQ_HD uint32_t trim_code(char ch)
{
    switch ((unsigned char)ch) {
    case 'A': case 'a': return 0u;
    case 'C': case 'c': return 1u;
    case 'G': case 'g': return 2u;
    case 'T': case 't': return 3u;
    default: return 4u;
    }
}
// bit i of x -> bit 2i
FQ_HD uint64_t trim_spread32(uint32_t x)
{
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull; v = (v | (v << 8)) & 0x00FF00FF00FF00FFull; v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull; v = (v | (v << 1)) & TR_EVEN;
    return v;
}
// 64 bases as three bit planes (bit i = base i: low code bit, high code bit, not ACGT) -> two words of codes and two of the mask (bit 2i of the mask = base i)
FQ_HD void trim_pack64(uint64_t lo, uint64_t hi, uint64_t bad, uint64_t code[2], uint64_t mask[2])
{
    code[0] = trim_spread32((uint32_t)lo) | (trim_spread32((uint32_t)hi) << 1); code[1] = trim_spread32((uint32_t)(lo >> 32)) | (trim_spread32((uint32_t)(hi >> 32)) << 1);
    mask[0] = trim_spread32((uint32_t)bad); mask[1] = trim_spread32((uint32_t)(bad >> 32));
}
// 64 bits of a plane from bit `at` on (w[at / 64 + 1] is read when at is not a multiple of 64: the plane is TR_WORDS long)
FQ_HD uint64_t trim_extract64(const uint64_t *w, uint32_t at)
{
    const uint32_t k = at >> 6, s = at & 63u;
    return s ? (w[k] >> s) | (w[k + 1] << (64u - s)) : w[k];
}
// the even bits of the first n bases of a 64-base window, words 0 and 1
FQ_HD uint64_t trim_overlap_mask(uint32_t n, int word)
{
    const uint32_t m = word ? (n > 32u ? n - 32u : 0u) : (n < 32u ? n : 32u);
    return m >= 32u ? TR_EVEN : ((1ull << (2u * m)) - 1ull) & TR_EVEN;
}
// rule 2's m: positions i < n with s[p + i] != A[i]
FQ_HD uint32_t trim_mismatches(const uint64_t *code, const uint64_t *mask, uint32_t p, uint64_t a0, uint64_t a1, uint32_t n)
{
    const uint64_t x0 = trim_extract64(code, 2u * p) ^ a0, f0 = (x0 | (x0 >> 1) | trim_extract64(mask, 2u * p)) & trim_overlap_mask(n, 0);
    uint32_t m = (uint32_t)__builtin_popcountll(f0);
    if (n > 32u) {
        const uint64_t x1 = trim_extract64(code, 2u * p + 64u) ^ a1, f1 = (x1 | (x1 >> 1) | trim_extract64(mask, 2u * p + 64u)) & trim_overlap_mask(n, 1);
        m += (uint32_t)__builtin_popcountll(f1);
    }
    return m;
}
FQ_HD bool trim_adapter_ok(uint32_t m, uint32_t n, uint32_t max_err_permille) { return m * 1000u <= n * max_err_permille; }
// which adapter a read takes: text 2's reads, and the odd reads of one text that holds pairs, take adapter 1
FQ_HD int trim_adapter_of(uint32_t k, bool two, int file, uint32_t flags) { return two ? file : ((flags & DG_TRIM_PAIRS) ? (int)(k & 1u) : 0); }
// rule 1's term at quality byte q; rule 3's at base ch for the poly base of code c
FQ_HD int trim_qual_term(uint32_t cutoff, char q, uint32_t qual_base) { return (int)cutoff - ((int)(unsigned char)q - (int)qual_base); }
FQ_HD int trim_poly_term(char ch, uint32_t c) { return trim_code(ch) == c ? 1 : -2; }
// a round of 64 steps of a walk: the lanes that count (in front of the first negative sum); the first / the last of a set of lanes
FQ_HD uint64_t trim_live_lanes(uint64_t valid, uint64_t neg) { return neg ? valid & ((1ull << __builtin_ctzll(neg)) - 1ull) : valid; }
FQ_HD uint32_t trim_first_lane(uint64_t m) { return (uint32_t)__builtin_ctzll(m); }
FQ_HD uint32_t trim_last_lane(uint64_t m) { return 63u - (uint32_t)__builtin_clzll(m); }
// rule 3: no later suffix can reach `best` any more (a step adds at most 1; an equal sum further in would still win, so strictly less)
FQ_HD bool trim_poly_hopeless(int carry, uint32_t steps_left, int best) { return (long long)carry + (long long)steps_left < (long long)best; }
// rule 1's end: walk results (-1: the sum never rose above 0) -> the window; an empty one is [0, 0), its bases charged to the 5' rule first
FQ_HD void trim_qual_window(uint32_t L, int t3, int t5, uint32_t &a, uint32_t &b, uint32_t &cut5, uint32_t &cut3)
{
    b = t3 < 0 ? L : L - 1u - (uint32_t)t3; a = t5 < 0 ? 0u : (uint32_t)t5 + 1u;
    if (a >= b) { cut5 = a; cut3 = L - a; a = b = 0u; } else { cut5 = a; cut3 = L - b; }
}
// rule 4 on a read's own window
FQ_HD bool trim_long_enough(uint32_t a, uint32_t b, uint32_t min_len) { return b - a >= min_len; }
// the stored quality's length: q[a .. min(b, ql))
FQ_HD uint32_t trim_stored_ql(uint32_t a, uint32_t b, uint32_t ql) { const uint32_t e = b < ql ? b : ql; return e > a ? e - a : 0u; }

// ---- the inline UMI (dg_set_umi): cut in front of the four steps, which then work on s[u .. L) ----
// the slot of a read (as trim_adapter_of picks the adapter); whether reads 2k and 2k + 1 are partners; the bases cut in front; the rule; a stored letter; what a name gains
FQ_HD int trim_umi_slot(uint32_t k, bool two, int file, uint32_t umi_flags) { return two ? file : ((umi_flags & DG_UMI_PAIRS) ? (int)(k & 1u) : 0); }
FQ_HD bool trim_umi_partnered(uint32_t k, bool two, uint32_t umi_flags, uint32_t n_reads) { return (two || (umi_flags & DG_UMI_PAIRS)) && (k ^ 1u) < n_reads; }
FQ_HD uint32_t trim_umi_cut(const TrimPar &p, int slot) { return p.umi_on ? p.umi_len[slot] + p.umi_skip[slot] : 0u; }
FQ_HD bool trim_umi_ok(uint32_t L, uint32_t u) { return L >= u + 1u; }
FQ_HD char trim_umi_letter(char ch) { const uint32_t c = trim_code(ch); return c == 0u ? 'A' : c == 1u ? 'C' : c == 2u ? 'G' : c == 3u ? 'T' : 'N'; }
FQ_HD uint32_t trim_umi_suffix(const TrimPar &p, int slot, bool partnered) { return p.umi_on ? 1u + (partnered ? p.umi_len[0] + p.umi_len[1] : p.umi_len[slot]) : 0u; }

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int trim_wave_incl(int v, uint32_t lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(v, o, 64); if (lane >= (uint32_t)o) v += up; }
    return v;
}
#define TR_NONE (-0x40000000)

// rule 1, one end: steps t = 0 .. L - 1 over q[from_end ? L - 1 - t : t]; the t at which the sum first reached its strict maximum > 0, or -1
__device__ __forceinline__ int trim_dev_qual_walk(const char *q, uint32_t L, bool from_end, uint32_t cutoff, uint32_t qual_base, uint32_t lane)
{
    int best = 0, best_t = -1, carry = 0;
    for (uint32_t t0 = 0; t0 < L; t0 += 64) {
        const uint32_t t = t0 + lane;
        const bool valid = t < L;
        const int incl = carry + trim_wave_incl(valid ? trim_qual_term(cutoff, q[from_end ? L - 1u - t : t], qual_base) : 0, lane);
        const uint64_t neg = __ballot(valid && incl < 0), live = trim_live_lanes(__ballot(valid), neg);
        const bool mine = (live >> lane) & 1ull;
        const int mx = d_wave_max<int>(mine ? incl : TR_NONE);
        if (mx > best) { best = mx; best_t = (int)(t0 + trim_first_lane(__ballot(mine && incl == mx))); }
        if (neg) break;
        carry = __shfl(incl, 63, 64);
    }
    return best_t;
}

// rule 3, one base: steps t = 0 .. b - a - 1 over s[b - 1 - t]; the largest t with the maximal sum, and that sum
__device__ __forceinline__ void trim_dev_poly_walk(const char *s, uint32_t a, uint32_t b, uint32_t c, uint32_t lane, int &best, int &best_t)
{
    const uint32_t n = b - a;
    int carry = 0;
    best = TR_NONE; best_t = -1;
    for (uint32_t t0 = 0; t0 < n; t0 += 64) {
        const uint32_t t = t0 + lane;
        const bool valid = t < n;
        const int incl = carry + trim_wave_incl(valid ? trim_poly_term(s[b - 1u - t], c) : 0, lane);
        const int mx = d_wave_max<int>(valid ? incl : TR_NONE);
        if (mx >= best) { best = mx; best_t = (int)(t0 + trim_last_lane(__ballot(valid && incl == mx))); }
        carry = __shfl(incl, 63, 64);
        if (t0 + 64 < n && trim_poly_hopeless(carry, n - (t0 + 64), best)) break;
    }
}

// One wave per workgroup, one workgroup per read, behind k_fq_lines.  A record the length kernel will refuse gets the empty window.
__global__ void __launch_bounds__(64)
k_trim_cut(const FqText x, const FqInfo *__restrict__ info, const TrimPar par, TrimRead *__restrict__ out)
{
    __shared__ uint64_t s_code[TR_WORDS], s_mask[TR_WORDS];
    if (info->status != FQ_OK) return;
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (k >= info->n_reads) return;
    int f; uint32_t rec;
    fq_read_place(k, x.two != 0, f, rec);
    uint32_t s1, s3;
    const uint32_t l1 = fq_dev_line(x, info, f, 4ull * rec + 1, s1), l3 = fq_dev_line(x, info, f, 4ull * rec + 3, s3);
    TrimRead r = {0, 0, 0, 0, 0, 0, 0, 0};
    if (l1 < 2u || l1 - 1u > (uint32_t)DG_MAX_RLEN) { if (lane == 0) out[k] = r; return; }
    // the UMI and its linker leave first: everything below sees s[u .. L) and q[u .. ql); step 1's condition is that of the untouched lengths
    const uint32_t L0 = l1 - 1u, ql0 = L0 < l3 ? L0 : l3, u = trim_umi_cut(par, trim_umi_slot(k, x.two != 0, f, par.umi_flags));
    if (!trim_umi_ok(L0, u)) { r.umi_fail = 1; if (lane == 0) out[k] = r; return; }
    const uint32_t L = L0 - u, ql = ql0 == L0 ? L : (ql0 > u ? ql0 - u : 0u);
    const char *line1 = (const char *)x.t[f] + s1 + u, *line3 = (const char *)x.t[f] + s3 + u;
    // the read as 2-bit codes and the not-ACGT mask
    for (uint32_t i0 = 0; i0 < L; i0 += 64) {
        const uint32_t c = i0 + lane < L ? trim_code(line1[i0 + lane]) : 4u;
        const uint64_t lo = __ballot(c & 1u), hi = __ballot(c & 2u), bad = __ballot(c & 4u);
        if (lane == 0) trim_pack64(lo, hi, bad, s_code + (i0 >> 5), s_mask + (i0 >> 5));
    }
    __syncthreads();
    // 1. quality ends
    uint32_t a = 0, b = L, cut5 = 0, cut3 = 0, flags = 0;
    if (par.qual3 | par.qual5) {
        if (ql == L) {
            const int t3 = par.qual3 ? trim_dev_qual_walk(line3, L, true, par.qual3, par.qual_base, lane) : -1;
            const int t5 = par.qual5 ? trim_dev_qual_walk(line3, L, false, par.qual5, par.qual_base, lane) : -1;
            trim_qual_window(L, t3, t5, a, b, cut5, cut3);
        } else flags |= TR_F_QSKIP;
    }
    // 2. the adapter: lane = start position
    uint32_t ad_cut = 0;
    const int ad = trim_adapter_of(k, x.two != 0, f, par.flags);
    const uint32_t alen = par.alen[ad];
    if (alen && b - a >= par.min_overlap) {
        const uint64_t a0 = par.acode[ad][0], a1 = par.acode[ad][1];
        const uint32_t last = b - par.min_overlap;
        for (uint32_t p0 = a; p0 <= last; p0 += 64) {
            const uint32_t p = p0 + lane;
            bool hit = false;
            if (p <= last) { const uint32_t n = b - p < alen ? b - p : alen; hit = trim_adapter_ok(trim_mismatches(s_code, s_mask, p, a0, a1, n), n, par.max_err_permille); }
            const uint64_t hits = __ballot(hit);
            if (hits) { const uint32_t p_hit = p0 + trim_first_lane(hits); ad_cut = b - p_hit; b = p_hit; flags |= TR_F_ADAPTER | (ad ? TR_F_ADAPTER1 : 0); break; }
        }
    }
    // 3. poly tails: the smallest counting i* over the enabled bases
    uint32_t poly_cut = 0;
    if (par.poly_mask && b > a) {
        uint32_t nb = b;
        for (uint32_t c = 0; c < 4; c++) {
            if (!((par.poly_mask >> c) & 1u)) continue;
            int best, best_t;
            trim_dev_poly_walk(line1, a, b, c, lane, best, best_t);
            if (best > 0 && (uint32_t)best_t + 1u >= par.poly_min) { const uint32_t at = b - 1u - (uint32_t)best_t; nb = at < nb ? at : nb; }
        }
        if (nb < b) { poly_cut = b - nb; b = nb; flags |= TR_F_POLY; }
    }
    if (lane == 0) {
        r.a = (uint16_t)(a + u); r.b = (uint16_t)(b + u); r.cut5 = (uint16_t)cut5; r.cut3 = (uint16_t)cut3; r.ad_cut = (uint16_t)ad_cut; r.poly_cut = (uint16_t)poly_cut; r.flags = (uint16_t)flags;
        out[k] = r;
    }
}

// loc / tile_sum hold four rows (bases, name bytes, quality bytes, kept reads) of `stride` / n_tiles entries
__global__ void __launch_bounds__(FQ_THREADS)
k_trim_len(const FqText x, FqInfo *info, const TrimPar par, TrimRead *__restrict__ win, TrimInfo *__restrict__ ti, uint32_t *__restrict__ name_at, uint32_t *__restrict__ name_len,
           uint32_t *__restrict__ loc, uint32_t stride, unsigned long long *__restrict__ tile_sum, uint32_t n_tiles)
{
    __shared__ uint32_t s_w[FQ_THREADS / 64];
    if (info->status != FQ_OK) return;
    const uint32_t n_reads = info->n_reads;
    const uint32_t k = blockIdx.x * FQ_THREADS + threadIdx.x;
    if (blockIdx.x * FQ_THREADS >= n_reads) { if (threadIdx.x < 4) tile_sum[(size_t)threadIdx.x * n_tiles + blockIdx.x] = 0ull; return; }
    uint32_t len[4] = {0u, 0u, 0u, 0u};
    unsigned long long st[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
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
        name_at[k] = r.name_at; name_len[k] = r.hl;
        if (good) {
            const TrimRead w = win[k];
            const int slot = trim_umi_slot(k, x.two != 0, f, par.umi_flags);
            const bool partnered = par.umi_on && trim_umi_partnered(k, x.two != 0, par.umi_flags, n_reads);
            const bool umi_fail = w.umi_fail != 0, umi_drop = umi_fail || (partnered && win[k ^ 1u].umi_fail != 0);      // the UMI rule is pairwise whatever DG_TRIM_PAIRS says
            const bool own = trim_long_enough(w.a, w.b, par.min_len) && !umi_fail;
            bool mate = true;
            if ((par.flags & DG_TRIM_PAIRS) && (k ^ 1u) < n_reads) { const TrimRead m = win[k ^ 1u]; mate = trim_long_enough(m.a, m.b, par.min_len); }
            const bool keep = own && mate && !umi_drop;
            if (keep) { len[0] = (uint32_t)w.b - w.a; len[1] = r.hl + trim_umi_suffix(par, slot, partnered); len[2] = trim_stored_ql(w.a, w.b, r.ql); len[3] = 1u; }
            st[0] = 1; st[1] = keep; st[2] = (unsigned long long)r.rlen; st[3] = len[0]; st[4] = w.cut5; st[5] = w.cut3;
            st[6] = (w.flags & TR_F_ADAPTER) && !(w.flags & TR_F_ADAPTER1); st[7] = (w.flags & TR_F_ADAPTER) && (w.flags & TR_F_ADAPTER1); st[8] = w.ad_cut;
            st[9] = (w.flags & TR_F_POLY) != 0; st[10] = w.poly_cut; st[11] = !umi_drop && !own; st[12] = !umi_drop && own && !mate; st[13] = (w.flags & TR_F_QSKIP) != 0;
            st[14] = par.umi_on && !umi_fail ? trim_umi_cut(par, slot) : 0u; st[15] = umi_drop;
            if (keep) win[k].flags = (uint16_t)(w.flags | TR_F_KEEP);          // (the mate's lane reads a, b alone)
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t total;
        const uint32_t ex = d_wg_exclusive<uint32_t>(len[i], total, s_w);
        if (k < n_reads) loc[(size_t)i * stride + k] = ex;
        if (threadIdx.x == 0) tile_sum[(size_t)i * n_tiles + blockIdx.x] = total;
    }
    const uint32_t mx = d_wave_max(len[0]);
    if ((threadIdx.x & 63u) == 0 && mx) atomicMax(&info->max_rlen, mx);
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const unsigned long long v = d_wave_sum<unsigned long long>(st[i]);
        if ((threadIdx.x & 63u) == 0 && v) atomicAdd(&ti->stats[i], v);
    }
}

__global__ void __launch_bounds__(FQ_THREADS)
k_trim_top3(unsigned long long *__restrict__ tile_sum, uint32_t n_tiles, FqInfo *__restrict__ info, TrimInfo *__restrict__ ti)
{
    __shared__ unsigned long long s_w[FQ_THREADS / 64];
    if (info->status != FQ_OK) return;
    const uint32_t used = (info->n_reads + FQ_THREADS - 1) / FQ_THREADS;
    const uint32_t nt = used < n_tiles ? used : n_tiles;
    for (int r = 0; r < 4; r++) {
        const unsigned long long total = d_tiles_exclusive<unsigned long long>(tile_sum + (size_t)r * n_tiles, nt, 1, s_w);
        if (threadIdx.x == 0) { if (r < 3) info->total[r] = total; else ti->n_kept = (uint32_t)total; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t be = info->bad_read, bl = info->bad_long;
        if (be != 0xFFFFFFFFu && be < bl) info->status = FQ_E_EMPTY;
        else if (bl != 0xFFFFFFFFu) { info->status = FQ_E_LONG; info->bad_read = bl; }
        else if (info->total[0] > 0xFFFFFF00ull || info->total[1] > 0xFFFFFF00ull || info->total[2] > 0xFFFFFF00ull) info->status = FQ_E_OFFSETS;
    }
}

// One wave per workgroup, one workgroup per read of the input; a kept read goes to its place among the kept.  Nothing is written when the status is raised.
__global__ void __launch_bounds__(64)
k_trim_write(const FqText x, const FqInfo *__restrict__ info, const TrimInfo *__restrict__ ti, int rc_odd_reads, const TrimRead *__restrict__ win, const uint32_t *__restrict__ name_at,
             const uint32_t *__restrict__ name_len, const uint32_t *__restrict__ loc, uint32_t stride, const unsigned long long *__restrict__ tile_base, uint32_t n_tiles,
             uint16_t *__restrict__ rlen, uint32_t *__restrict__ seq_off, unsigned char *__restrict__ seq, uint32_t *__restrict__ hdr_off, char *__restrict__ hdr,
             uint32_t *__restrict__ qual_off, char *__restrict__ qual)
{
    if (info->status != FQ_OK) return;
    const uint32_t n_reads = info->n_reads, k = blockIdx.x, lane = threadIdx.x;
    if (k == 0 && lane == 1) { const uint32_t n = ti->n_kept; seq_off[n] = (uint32_t)info->total[0]; hdr_off[n] = (uint32_t)info->total[1]; qual_off[n] = (uint32_t)info->total[2]; }
    if (k >= n_reads) return;
    const TrimRead w = win[k];
    if (!(w.flags & TR_F_KEEP)) return;
    const uint32_t tile = k / FQ_THREADS;
    const uint32_t so = (uint32_t)tile_base[tile] + loc[k], ho = (uint32_t)tile_base[(size_t)n_tiles + tile] + loc[(size_t)stride + k];
    const uint32_t qo = (uint32_t)tile_base[2 * (size_t)n_tiles + tile] + loc[2 * (size_t)stride + k];
    const uint32_t at = (uint32_t)tile_base[3 * (size_t)n_tiles + tile] + loc[3 * (size_t)stride + k];
    int f; uint32_t rec;
    fq_read_place(k, x.two != 0, f, rec);
    uint32_t s1, s3;
    const uint32_t l1 = fq_dev_line(x, info, f, 4ull * rec + 1, s1), l3 = fq_dev_line(x, info, f, 4ull * rec + 3, s3);
    const uint32_t L = l1 - 1u, rl = (uint32_t)w.b - w.a, hl = name_len[k], ql = trim_stored_ql(w.a, w.b, L < l3 ? L : l3);
    const bool rc = fq_stored_rc(k, rc_odd_reads);
    const char *t = (const char *)x.t[f];
    const char *line1 = t + s1 + w.a, *line3 = t + s3 + w.a, *name = t + name_at[k];
    for (uint32_t i = lane; i < rl; i += 64) seq[so + i] = (unsigned char)fq_stored_base(line1, rl, i, rc);
    for (uint32_t i = lane; i < hl; i += 64) hdr[ho + i] = name[i];
    for (uint32_t i = lane; i < ql; i += 64) qual[qo + i] = fq_stored_qual(line3, ql, i, rc);
    if (lane == 0) { seq_off[at] = so; hdr_off[at] = ho; qual_off[at] = qo; rlen[at] = (uint16_t)rl; }
}
// dg_set_umi only, behind k_trim_write (whose registers stay what they were): one wave per read of the input; a kept read's name gains sep, then the letters of
// read 2k and of read 2k + 1, or the read's own when it stands alone.  The partner's line 1 is found through fq_read_place(k ^ 1).
__global__ void __launch_bounds__(64)
k_trim_umi_name(const FqText x, const FqInfo *__restrict__ info, const TrimUmi um, const TrimRead *__restrict__ win, const uint32_t *__restrict__ name_len, const uint32_t *__restrict__ loc,
                uint32_t stride, const unsigned long long *__restrict__ tile_base, uint32_t n_tiles, char *__restrict__ hdr)
{
    if (info->status != FQ_OK) return;
    const uint32_t n_reads = info->n_reads, k = blockIdx.x, lane = threadIdx.x;
    if (k >= n_reads || !(win[k].flags & TR_F_KEEP)) return;
    const uint32_t ho = (uint32_t)tile_base[(size_t)n_tiles + k / FQ_THREADS] + loc[(size_t)stride + k], hl = name_len[k];
    if (um.on) {                                                    // the name's suffix: sep, then the letters of read 2k and of read 2k + 1, or the read's own when it stands alone
        const bool two = x.two != 0, partnered = trim_umi_partnered(k, two, um.flags, n_reads);
        if (lane == 0) hdr[ho + hl] = (char)um.sep;
        uint32_t o = ho + hl + 1u;
#pragma unroll 1
        for (uint32_t j = 0; j < (partnered ? 2u : 1u); j++) {
            const uint32_t kk = partnered ? (k & ~1u) + j : k;
            int ff; uint32_t rr, ss;
            fq_read_place(kk, two, ff, rr);
            const uint32_t ll = fq_dev_line(x, info, ff, 4ull * rr + 1, ss), n = um.len[trim_umi_slot(kk, two, ff, um.flags)];
            const char *from = (const char *)x.t[ff] + ss;
            for (uint32_t i = lane; i < n && i < ll; i += 64) hdr[o + i] = trim_umi_letter(from[i]);      // (a kept read's partner passed the rule: its line holds them)
            o += n;
        }
    }
}
#endif
#endif
