// dg_umidup.h -- UMI-aware duplicate marking of the coordinate-sorted BAM (dg_bam_markdup_umi_finish): dg_markdup.h's marking with the unique molecular
// identifier at the end of a record's name as one more part of a duplicate's signature, and, with max_edit 1, with UMIs one letter apart taken for copies of
// one molecule with a sequencing error.  Position alone flags the independent fragments of a highly expressed transcript as copies: this is why RNA-seq
// libraries carry UMIs.  The definition stands in include/dartgpu.h (tests/umidup_inputs.py is its sequential twin); in short:
//   U        of a record: the bytes behind the last `sep` of its name, 1..21 of A C G T N + - as codes 1..7, first letter most significant (3 bits each); else 0
//   group    the pairs with equal (lo, hi, U) inside the family of equal (lo, hi); the ends (two per pair, one per fragment) with equal (E, U) inside the
//            family of equal E.  count: its pairs / ends
//   cluster  max_edit 1, families of 2..UD_FAMILY groups: in the order (count descending, U ascending) a group joins the first earlier group that is still
//            its own root, has a UMI of the same length at most one letter away (neither U is 0) and count_root >= 2 count - 1.  One hop only.
//   verdict  the best pair of a cluster survives; a fragment is a duplicate when its cluster holds a pair end or a better fragment
// Everything else -- the filter, the end key, the score, the hash, the runs, pairs and fragments -- is dg_markdup.h's code, called from here.
//
//   k_ud_rec          lane = sorted record: md_record_fields and ONE pass over the name for both the hash and U (ud_name); the candidates' scan; per workgroup the
//                     examined records, those with a UMI, the first record out of range, the largest U
//   -- the first wait: the candidates, and the largest U: the UMI sorts take only the bits in use, 4 per pass --
//   k_md_compact, sort, k_md_mate, k_md_count -- the second wait -- k_md_emit: dg_markdup.h's, unchanged
//   (pair sorts)      by inverted score, k_ud_rekey_u to U, sort, k_md_rekey to hi, sort, to lo, sort: (lo, hi, U, score descending, rep)
//   (end sorts)       by (paired first, inverted score), to U, sort, to E, sort: (E, U, paired first, score descending, index)
//                     The head of a group is then its best pair; for ends a pair end if the group has one, else its best fragment.
//   for the pairs, then for the ends (the same five kernels, the same arrays):
//   k_ud_heads        lane = sorted item: is it the first of its family / of its group; the workgroup's scan of families << 32 | groups
//   k_ud_groups       lane = item: its group's number; a group head leaves its place (the next head's place minus its own is the group's count), a family head
//                     its first group's number; every group starts as its own winner
//   k_ud_fams         lane = family: its number of groups; 2..UD_FAMILY with max_edit 1: work, scanned; families of more than one group and crowded ones counted
//   k_ud_worklist     lane = family: the work list, compacted
//   k_ud_cluster      wave = family of the work list, lane = group: the rank by (count descending, U ascending) counted across the wave; the walk over the
//                     ranks with the current group's (U, count, still a root) broadcast, all lanes testing at once (xor, or-fold of the 3-bit fields, popcount);
//                     per root the lane that holds the best head of the cluster: that group wins, every other loses.  No LDS: 64 groups live in registers and
//                     talk through cross-lane reads
//   k_ud_flag         lane = item: a duplicate unless it is the head of its group and its group wins.  Byte 19 of both records of a pair, of a fragment's record;
//                     pair ends write nothing.  One writer per examined record, plain byte stores
//   -- the third wait: the counts --
// No kernel of this file uses an atomic (k_cv_top sums what the workgroups leave).  The array is sorted once per list: the clustering needs group heads only.
// Memory beside dg_markdup.h's buffers (which this call uses as its own: the two never run at once on a context): 8 bytes per record (U); per end 13 bytes
// (mark, group number, place, first group, winner) and 8 per family of the work list.
// Measured (profiles/umidup/umidup_rate.json; one MI355X, markdup_rate.py's 2.2 M records with an 8-letter UMI in every name, 495 MB): 8.12 ms of kernels with
// max_edit 0 and 8.27 ms with 1, beside 7.37 ms of dg_bam_markdup_finish over the same array: 12 more sorter passes (63), 0.20 ms for heads, groups and
// families, 0.11 ms for the clustering (a grid sized for the worst case; 51 families had two groups), flag writes as before.  The record pass dominates here too.
#ifndef DG_UMIDUP_H
#define DG_UMIDUP_H
#include "dg_markdup.h"

#define UD_FAMILY 64                 // the most groups a family may hold and still be clustered: one wave, lane = group (dg_bam_markdup_umi_granules [3])
#define UD_MAX_LEN 21                // letters of a UMI: 63 bits
#define UD_FIELD_LSB 0x1249249249249249ull      // bit 0 of each of the 21 3-bit fields
static_assert(UD_FAMILY == 64, "k_ud_cluster keeps a family in one wave");
enum { UD_ST_CAND = 0, UD_ST_EXAMINED, UD_ST_WITH_UMI, UD_ST_NBAD, UD_ST_UMAX, UD_ST_COUNTS, UD_ST_CROWDED, UD_ST_JUNK, UD_ST_PAIRS = 8, UD_ST_ENDS = 16, UD_ST_WORDS = 24 };
// the words of one list (at UD_ST_PAIRS / UD_ST_ENDS): k_cv_top's outputs lie side by side
enum { UD_L_HEADS = 0 /* families << 32 | groups */, UD_L_WORK, UD_L_MULTI, UD_L_CROWDED, UD_L_ABSORBED, UD_L_CLUSTER_MAX, UD_L_DUP, UD_L_GROUP_MAX };

MD_HD uint32_t ud_code(unsigned char b)
{
    return b == 'A' ? 1u : b == 'C' ? 2u : b == 'G' ? 3u : b == 'T' ? 4u : b == 'N' ? 5u : b == '+' ? 6u : b == '-' ? 7u : 0u;
}
// one pass over a name: its hash as md_hash gives it, and its UMI
struct UdName { uint64_t h, U; };
MD_HD UdName ud_name(const unsigned char *name, uint32_t len, int hash_bits, unsigned char sep)
{
    uint64_t h = 0xcbf29ce484222325ull, U = 0;
    uint32_t ulen = 0;
    bool ok = false;                                             // a sep was seen, and every byte behind the last one is a letter, at most UD_MAX_LEN of them
    for (uint32_t k = 0; k < len; k++) {
        const unsigned char b = name[k];
        h ^= (uint64_t)b; h *= 0x100000001b3ull;
        if (b == sep) { ok = true; U = 0; ulen = 0; continue; }
        const uint32_t code = ud_code(b);
        if (!code || ulen >= UD_MAX_LEN) ok = false;
        else { U = U << 3 | code; ulen++; }
    }
    h ^= h >> 48;
    UdName r; r.h = hash_bits >= 64 ? h : h & ((1ull << hash_bits) - 1ull); r.U = ok && ulen ? U : 0ull;
    return r;
}
struct UdRec { MdRec r; uint64_t U; };
MD_HD UdRec ud_record(const unsigned char *rec, uint64_t avail, int n_chr, int hash_bits, unsigned char sep)
{
    BamHead h;
    UdRec u; u.r = md_record_fields(rec, avail, n_chr, h); u.U = 0;
    if (!u.r.examined || u.r.bad) return u;
    const UdName nm = ud_name(rec + BAM_FIXED, md_name_len(h), hash_bits, sep);
    u.U = nm.U;
    if (u.r.candidate) u.r.h = nm.h;
    return u;
}
// the bits of the largest U, as the sorter takes them
MD_HD int ud_umi_bits(uint64_t u_max) { int b = 0; while (b < 64 && (u_max >> b) != 0) b++; return b; }
MD_HD uint32_t ud_popcount(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
MD_HD uint32_t ud_fields(uint64_t x) { return ud_popcount((x | x >> 1 | x >> 2) & UD_FIELD_LSB); }     // the 3-bit fields of x that are not 0: of a U its letters, of an xor the mismatches
// group (U_r, count_r), a root walked earlier, takes in group (U_g, count_g)
MD_HD bool ud_joins(uint64_t Ur, uint64_t count_r, uint64_t Ug, uint64_t count_g)
{
    return Ur != 0ull && Ug != 0ull && ud_fields(Ur) == ud_fields(Ug) && ud_fields(Ur ^ Ug) <= 1u && count_r >= 2ull * count_g - 1ull;
}
// a is walked before b
MD_HD bool ud_before(uint64_t count_a, uint64_t Ua, uint64_t count_b, uint64_t Ub) { return count_a > count_b || (count_a == count_b && Ua < Ub); }
// what a group's head brings to its cluster: the smallest wins.  A pair: (inverted score, rep); an end: (paired first, inverted score, index)
MD_HD uint64_t ud_pair_rank(uint32_t rep, const uint32_t *score, const uint32_t *mate) { return md_pair_score_key(score[rep], score[mate[rep]]) << 32 | (uint64_t)rep; }
MD_HD uint64_t ud_end_rank(int64_t v, const uint32_t *score) { return v < 0 ? (uint64_t)(uint32_t)~v : md_end_score_key(false, score[(uint32_t)v]) << 32 | (uint64_t)(uint32_t)v; }
// sorted item q (keys = lo of a pair / E of an end): the first of its family, of its group
MD_HD bool ud_family_head(const uint64_t *keys, const int64_t *vals, uint32_t q, int ends, const uint64_t *E, const uint32_t *mate)
{
    if (ends) return q == 0u || keys[q] != keys[q - 1u];
    return md_pair_is_head(keys, vals, q, E, mate);
}
MD_HD bool ud_group_head(const uint64_t *keys, const int64_t *vals, uint32_t q, int ends, const uint64_t *E, const uint32_t *mate, const uint64_t *U)
{
    return ud_family_head(keys, vals, q, ends, E, mate) || U[md_end_record(vals[q])] != U[md_end_record(vals[q - 1u])];
}
// an item's mark: the groups and families in front of it in its workgroup (at most 255 each), and what it is itself
MD_HD uint32_t ud_mark(uint64_t before, bool fh, bool gh) { return ((uint32_t)before & 0x1ffu) | ((uint32_t)(before >> 32) & 0x1ffu) << 9 | (gh ? 1u << 30 : 0u) | (fh ? 1u << 31 : 0u); }
MD_HD uint32_t ud_mark_groups(uint32_t m) { return m & 0x1ffu; }
MD_HD uint32_t ud_mark_fams(uint32_t m) { return m >> 9 & 0x1ffu; }
MD_HD bool ud_family_is_work(uint32_t n_groups, uint32_t max_edit) { return max_edit != 0u && n_groups >= 2u && n_groups <= UD_FAMILY; }
// an item's verdict
MD_HD bool ud_is_dup(bool head_of_group, bool group_wins) { return !(head_of_group && group_wins); }

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MD_THREADS)
k_ud_rec(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, int n_chr, int hash_bits,
         unsigned char sep, uint64_t *__restrict__ E, uint64_t *__restrict__ h, uint64_t *__restrict__ U, uint32_t *__restrict__ score, uint32_t *__restrict__ mate,
         uint32_t *__restrict__ cand_off, uint64_t *__restrict__ tile_sum, uint64_t *__restrict__ part /* 4 planes: examined, with a UMI | ~bad, the largest U */)
{
    __shared__ uint64_t s_wave[MD_THREADS / 64];
    __shared__ unsigned long long s_part[4 * (MD_THREADS / 64)];
    const uint32_t i = blockIdx.x * MD_THREADS + threadIdx.x;
    uint64_t mine = 0, examined = 0, nbad = 0, umi = 0;
    if (i < n) {
        UdRec u; u.r.examined = false; u.r.candidate = false; u.r.bad = false; u.r.E = 0; u.r.h = 0; u.r.score = 0; u.U = 0;
        const uint64_t at = bam_rec_start(dst_off, tile_base, i);
        if (at < n_raw) u = ud_record(sorted + at, n_raw - at, n_chr, hash_bits, sep);
        if (u.r.bad) nbad = ~(uint64_t)i;
        examined = u.r.examined ? 1 : 0; mine = u.r.candidate ? 1 : 0; umi = u.U;
        E[i] = u.r.E; h[i] = u.r.h; U[i] = u.U; score[i] = u.r.score; mate[i] = u.r.examined ? MD_FRAGMENT : MD_NOT_EXAMINED;
    }
    uint64_t all;
    const uint64_t ex = d_wg_exclusive(mine, all, s_wave);
    if (i < n) cand_off[i] = (uint32_t)ex | (mine ? 1u << 31 : 0u);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
    const unsigned long long v[4] = {examined, umi ? 1ull : 0ull, nbad, umi};
    cv_block_partials(v, 2, s_part, part);
}

// the next key of the sorted items: their U
__global__ void __launch_bounds__(MD_THREADS)
k_ud_rekey_u(uint64_t *__restrict__ keys, const int64_t *__restrict__ vals, uint32_t n_items, const uint64_t *__restrict__ U, uint32_t n)
{
    const uint32_t q = blockIdx.x * MD_THREADS + threadIdx.x;
    if (q >= n_items) return;
    const uint32_t i = md_end_record(vals[q]);
    if (i < n) keys[q] = U[i];
}

__global__ void __launch_bounds__(MD_THREADS)
k_ud_heads(const uint64_t *__restrict__ keys, const int64_t *__restrict__ vals, uint32_t n_items, int ends, const uint64_t *__restrict__ E, const uint32_t *__restrict__ mate,
           const uint64_t *__restrict__ U, uint32_t *__restrict__ mark, uint64_t *__restrict__ tile_sum)
{
    __shared__ uint64_t s_wave[MD_THREADS / 64];
    const uint32_t q = blockIdx.x * MD_THREADS + threadIdx.x;
    bool fh = false, gh = false;
    if (q < n_items) { fh = ud_family_head(keys, vals, q, ends, E, mate); gh = fh || ud_group_head(keys, vals, q, ends, E, mate, U); }
    uint64_t all;
    const uint64_t ex = d_wg_exclusive<uint64_t>((uint64_t)((fh ? 1ull << 32 : 0ull) | (gh ? 1ull : 0ull)), all, s_wave);
    if (q < n_items) mark[q] = ud_mark(ex, fh, gh);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// head_base: k_ud_heads' sums, scanned.  grp_of: n_items; gpos, ffirst: n_items + 1 (the last item closes both lists); win: n_items
__global__ void __launch_bounds__(MD_THREADS)
k_ud_groups(const uint32_t *__restrict__ mark, const uint64_t *__restrict__ head_base, uint32_t n_items, uint32_t *__restrict__ grp_of, uint32_t *__restrict__ gpos,
            uint32_t *__restrict__ ffirst, unsigned char *__restrict__ win)
{
    const uint32_t q = blockIdx.x * MD_THREADS + threadIdx.x;
    if (q >= n_items) return;
    const uint32_t m = mark[q];
    const uint64_t base = head_base[blockIdx.x];
    const uint32_t gh = m >> 30 & 1u, fh = m >> 31;
    const uint32_t g_incl = (uint32_t)base + ud_mark_groups(m) + gh, f_incl = (uint32_t)(base >> 32) + ud_mark_fams(m) + fh;
    if (g_incl == 0u || f_incl == 0u || g_incl > q + 1u || f_incl > g_incl) return;      // (item 0 is a head of both: never taken on a sorted list)
    const uint32_t g = g_incl - 1u;
    grp_of[q] = g;
    if (gh) { gpos[g] = q; win[g] = 1; }
    if (fh) ffirst[f_incl - 1u] = g;
    if (q + 1u == n_items) { gpos[g_incl] = n_items; ffirst[f_incl] = g_incl; }
}

// heads: the total of k_ud_heads' scan.  The grid covers n_items families: a bound
__global__ void __launch_bounds__(MD_THREADS)
k_ud_fams(const uint32_t *__restrict__ ffirst, const unsigned long long *__restrict__ heads, uint32_t n_items, uint32_t max_edit, uint32_t *__restrict__ woff, uint64_t *__restrict__ tile_sum,
          uint64_t *__restrict__ part /* 2 planes: families of more than one group, crowded families */)
{
    __shared__ uint64_t s_wave[MD_THREADS / 64];
    __shared__ unsigned long long s_part[2 * (MD_THREADS / 64)];
    const uint32_t f = blockIdx.x * MD_THREADS + threadIdx.x;
    const unsigned long long hd = *heads;
    const uint32_t n_fam = (uint32_t)(hd >> 32), n_grp = (uint32_t)hd;
    uint32_t ng = 0;
    if (f < n_fam && f < n_items) { const uint32_t a = ffirst[f], b = ffirst[f + 1u]; if (a < b && b <= n_grp) ng = b - a; }
    const bool work = ud_family_is_work(ng, max_edit);
    uint64_t all;
    const uint64_t ex = d_wg_exclusive<uint64_t>((uint64_t)(work ? 1 : 0), all, s_wave);
    if (f < n_items) woff[f] = (uint32_t)ex | (work ? 1u << 31 : 0u);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
    const unsigned long long v[2] = {ng > 1u ? 1ull : 0ull, ng > UD_FAMILY ? 1ull : 0ull};
    cv_block_partials(v, 2, s_part, part);
}

// work_base: k_ud_fams' sums, scanned; wl holds n_items / 2 + 1 families at the most (a family of the list has two groups or more)
__global__ void __launch_bounds__(MD_THREADS)
k_ud_worklist(const uint32_t *__restrict__ woff, const uint64_t *__restrict__ work_base, uint32_t n_items, uint32_t *__restrict__ wl)
{
    const uint32_t f = blockIdx.x * MD_THREADS + threadIdx.x;
    if (f >= n_items) return;
    const uint32_t o = woff[f];
    if (!(o >> 31)) return;
    const uint64_t w = work_base[blockIdx.x] + (o & 0x7FFFFFFFu);
    if (w <= n_items / 2u) wl[w] = f;
}

// n_work: the total of k_ud_fams' scan.  Any grid: a wave takes every (waves of the grid)-th family of the list; one without a family only takes part in the sums
__global__ void __launch_bounds__(MD_THREADS)
k_ud_cluster(const uint32_t *__restrict__ wl, const unsigned long long *__restrict__ n_work, const uint32_t *__restrict__ ffirst, const uint32_t *__restrict__ gpos,
             const int64_t *__restrict__ vals, uint32_t n_items, int ends, const uint64_t *__restrict__ U, const uint32_t *__restrict__ score, const uint32_t *__restrict__ mate, uint32_t n,
             unsigned char *__restrict__ win, uint64_t *__restrict__ part /* 2 planes: absorbed groups | the largest cluster */)
{
    __shared__ unsigned long long s_part[2 * (MD_THREADS / 64)];
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long todo = *n_work;
    unsigned long long absorbed = 0, cluster = 0;
    for (uint32_t w = blockIdx.x * (MD_THREADS / 64) + (threadIdx.x >> 6); (unsigned long long)w < todo && w <= n_items / 2u; w += gridDim.x * (MD_THREADS / 64)) {
        const uint32_t f = wl[w];
        uint32_t g0 = 0, ng = 0;
        if (f < n_items) { g0 = ffirst[f]; const uint32_t g1 = ffirst[f + 1u]; if (g0 < g1 && g1 <= n_items && g1 - g0 <= UD_FAMILY) ng = g1 - g0; }
        const bool live = lane < ng;
        uint64_t Ug = 0, cnt = 0, rank_key = ~0ull;
        if (live) {
            const uint32_t q = gpos[g0 + lane], q1 = gpos[g0 + lane + 1u];
            if (q < q1 && q1 <= n_items) {
                cnt = q1 - q;
                const int64_t v = vals[q];
                const uint32_t i = md_end_record(v);
                if (i < n) { Ug = U[i]; rank_key = ends ? ud_end_rank(v, score) : (mate[i] < n ? ud_pair_rank(i, score, mate) : ~0ull); }
            }
        }
        // the lane's place in the walk
        uint32_t place = 0;
        for (uint32_t m = 0; m < ng; m++) {
            const uint64_t cm = __shfl(cnt, (int)m, 64), Um = __shfl(Ug, (int)m, 64);
            if (m != lane && (ud_before(cm, Um, cnt, Ug) || (cm == cnt && Um == Ug && m < lane))) place++;
        }
        // the walk: every lane behind the current group tests it at once
        uint32_t root = lane;
        for (uint32_t r = 0; r + 1u < ng; r++) {
            const unsigned long long at = __ballot(live && place == r);
            if (!at) continue;
            const int src = __ffsll((long long)at) - 1;
            const uint64_t Ur = __shfl(Ug, src, 64), cr = __shfl(cnt, src, 64);
            const uint32_t root_r = __shfl(root, src, 64);
            if (root_r == (uint32_t)src && live && root == lane && place > r && ud_joins(Ur, cr, Ug, cnt)) root = (uint32_t)src;
        }
        // per root: the lane of the best head, and the cluster's pairs / ends
        uint64_t best = rank_key; uint32_t best_lane = lane; unsigned long long sum = 0;
        for (uint32_t m = 0; m < ng; m++) {
            const uint64_t km = __shfl(rank_key, (int)m, 64), cm = __shfl(cnt, (int)m, 64);
            const uint32_t rm = __shfl(root, (int)m, 64);
            if (rm != root) continue;
            sum += cm;
            if (km < best || (km == best && m < best_lane)) { best = km; best_lane = m; }
        }
        if (live) { win[g0 + lane] = best_lane == lane ? 1 : 0; absorbed += root != lane ? 1ull : 0ull; if (sum > cluster) cluster = sum; }
    }
    const unsigned long long v[2] = {absorbed, cluster};
    cv_block_partials(v, 1, s_part, part);
}

__global__ void __launch_bounds__(MD_THREADS)
k_ud_flag(const int64_t *__restrict__ vals, uint32_t n_items, int ends, const uint32_t *__restrict__ grp_of, const uint32_t *__restrict__ gpos, const unsigned char *__restrict__ win,
          const uint32_t *__restrict__ mate, unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw,
          int write, uint64_t *__restrict__ part /* 2 planes: duplicate pairs / fragments | the largest group */)
{
    __shared__ unsigned long long s_part[2 * (MD_THREADS / 64)];
    const uint32_t q = blockIdx.x * MD_THREADS + threadIdx.x;
    unsigned long long dups = 0, size = 0;
    if (q < n_items) {
        const uint32_t g = grp_of[q];
        if (g < n_items) {
            const uint32_t first = gpos[g];
            const bool dup = ud_is_dup(first == q, win[g] != 0);
            const int64_t v = vals[q];
            if (first <= q) size = (unsigned long long)(q - first) + 1ull;
            if (!ends) {
                const uint32_t i = (uint32_t)v;
                dups = dup ? 1 : 0;
                if (write) { md_write(sorted, dst_off, tile_base, i, n, n_raw, dup); if (i < n) md_write(sorted, dst_off, tile_base, mate[i], n, n_raw, dup); }
            } else if (v >= 0) {
                dups = dup ? 1 : 0;
                if (write) md_write(sorted, dst_off, tile_base, (uint32_t)v, n, n_raw, dup);
            }
        }
    }
    const unsigned long long v2[2] = {dups, size};
    cv_block_partials(v2, 1, s_part, part);
}
#endif
#endif
