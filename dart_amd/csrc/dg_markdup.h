// dg_markdup.h -- duplicate marking of the coordinate-sorted BAM, in HBM between the sort (dg_bamsort.h) and everything that reads the sorted array: after
// dg_bam_sort_finish every record of the job lies in one array with its place known, and the verdict is one bit (0x400) in byte 19 of a record.  Written
// before dg_bam_sort_compress, the file, the .bai and the coverage track (whose default filter 0x704 skips duplicates) all see it.  The reference has no such
// output: an opt-in extension (what `samtools markdup` or Picard MarkDuplicates would compute from the sorted file, read back, inflated and deflated again).
//
// THE DEFINITION.  No samtools or Picard exists where this project is built and tested: this definition -- modelled on Picard's rules (unclipped 5' ends, sum
// of base qualities, a fragment loses to any pair that shares its end) -- is what the tests pin (tests/markdup_inputs.py is its sequential twin).
//
// Per sorted record (its fields, CIGAR and the places of its parts as bam_head and bam_cigar_walk of dg_bamrec.h give them):
//   examined  all of: 0 <= refID < n_chr; pos >= 0; flag & 4 clear; flag & 0x900 clear; n_cigar_op > 0; and name, CIGAR, bases and qualities lie inside the
//             record and the array: 36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq <= 4 + block_size, and <= the bytes the array holds from the
//             record's start.  Every other record plays no part and leaves with its bytes unchanged.
//   0x400     the input's bit plays no part.  An examined record leaves with the verdict, set or cleared: the call is idempotent.
//   end key   s = flag >> 4 & 1; rlen = the sum of the lengths of M, D, N, =, X (ops 0, 2, 3, 7, 8); lead / trail = the sum of the S and H ops (4, 5) in front
//             of the first / behind the last op that is neither (a CIGAR of clips alone: lead = their sum, trail = 0);
//             u5 = s ? pos + rlen - 1 + trail : pos - lead, in 64-bit arithmetic: the unclipped 5' end.  u5 + 2^31 must lie in [0, 2^33): otherwise the call
//             fails with DG_ERR_RANGE, the text names the first such record's index in the sorted array, and nothing is written.
//             E = refID << 34 | (u5 + 2^31) << 1 | s
//   score     the sum of the quality bytes q with 15 <= q <= 93, saturated at 2^20 - 1 (0xff, the quality of FASTA input, counts as 0 like every q > 93)
//   paired candidate   an examined record with flag & 1 set, flag & 8 clear, and exactly one of 0x40 and 0x80 set
//   name      the l_read_name - 1 bytes at byte 36 (without the NUL; none when l_read_name is 0).  The reference cuts names at '/', so mates carry the same
//   hash      h = FNV-1a 64 over the name (basis 0xcbf29ce484222325, prime 0x100000001b3), folded as (h ^ h >> 48) and masked to hash_bits bits.  hash_bits
//             is 48; DG_MARKDUP_HASH_BITS = 1..48 in the environment of dg_init overrides it (a test hook: it makes collisions and crowds reachable).
// Runs.  The candidates, ordered stably by h, fall into runs of equal h.  A run of more than 64 candidates is CROWDED: all its members are fragments.  Else the
//   candidates of a run with the same name bytes form a group; a group of exactly two, one with 0x40 and one with 0x80, is a PAIR; members of any other
//   group are fragments.  A FRAGMENT is an examined record that is in no pair.
// Pairs.  lo = min(Ea, Eb), hi = max(Ea, Eb); score = the sum of both members'; rep = the smaller of the members' indices in the sorted array.  Among pairs
//   with equal (lo, hi) the one with the largest score survives, on equal scores the one with the smallest rep; both records of every other pair get 0x400.
// Fragments.  A fragment with end key E is a duplicate when any pair has lo == E or hi == E, or when another fragment with the same E has a larger score, or
//   an equal score and a smaller index.
// Optical duplicates and the propagation to secondary or supplementary records are not done; UMIs are dg_umidup.h's (dg_bam_markdup_umi_finish), which reuses
// every function below.
// The verdict is a function of the sorted array alone, and that array is a function of the record set and the ordinals (dg_bamsort.h).
//
//   k_md_rec         lane = sorted record: the filter, the CIGAR walk, the quality sum, the name's hash: E, score, h, the class (in `mate`: not examined /
//                    fragment); the workgroup's exclusive scan of the candidates; per workgroup the examined records and the first record out of range
//   k_cv_top         (dg_coverage.h) one workgroup: the scan of the workgroups' sums, their other values summed or their maximum taken.  Behind every
//                    counting kernel here: no kernel of this file uses an atomic
//   -- the first wait: the number of candidates sizes the sorter's buffers; a record out of range ends the call --
//   k_md_compact     lane = record: candidate c gets the pair (h, index)
//   (sort)           stable radix sort by h (rs_sort_passes of dg_sort.h), hash_bits bits: inside a run the indices ascend
//   k_md_mate        lane = candidate: walks its run at most 64 steps to either side (longer: crowded), compares name bytes, and leaves its partner's index in
//                    mate[own index] (every record has one writer); per workgroup the candidates in crowded runs
//   k_md_count       lane = record: a pair's smaller index (rep) counts one pair and two ends, a fragment one end; the workgroup's scan of pairs << 32 | ends
//   -- the second wait: the numbers of pairs and ends --
//   k_md_emit        lane = record: pair p = (inverted score, rep); ends = (0, ~member) twice for a pair, (2^20 | inverted score, index) for a fragment.  Both
//                    lists are in index order: what the stable sorts keep is the order of rep and of index
//   (pair sorts)     by inverted score (21 bits), k_md_rekey to hi, sort (34 + chromosome bits), k_md_rekey to lo, sort: ascending (lo, hi), then descending
//                    score, then ascending rep.  A pair whose (lo, hi) equals its predecessor's is a duplicate: a purely local test
//   k_md_heads       lane = sorted pair: the head of a family (first of its (lo, hi)) carries its own position; per workgroup the last head (last-valid
//   k_cv_tails_top   scan of dg_coverage.h across workgroups), so that
//   k_md_flag_pairs  lane = sorted pair: knows its family's head however far back it lies (the largest family), and writes byte 19 of both records
//   (end sorts)      by (paired first, inverted score: 21 bits), k_md_rekey to E, sort.  A fragment that is not the head of its run of equal E is a duplicate
//   k_md_flag_ends   lane = sorted end: writes byte 19 of a fragment's record.  Every examined record is a fragment or a member of one pair: one writer each,
//                    plain byte stores
//   -- the third wait: the counts --
// Memory: 32 bytes per record (E, h, score, mate, the candidate's and the pair/end offsets); 32 per candidate (two key and two value buffers of the sorter,
// which the pairs -- at most half as many -- use after the mate search), 32 per end (at most one per record) and the sorter's histograms; 40 bytes per
// workgroup.  Everything a lane computes is host-callable: tests/native/markdup_checks.hip runs the same code on the CPU.
// Measured (profiles/markdup/markdup_rate.json; one MI355X, 2.2 M records of 2x101 in 476 MB, a tenth of the pairs twice): 6.82 ms of kernels beside 1.36 ms of
// dg_bam_sort_finish and 19.7 ms of BGZF kernels; record pass 3.95 ms, mate sort and search 1.11, pair sorts 0.80, end sorts 0.71, family scan and flag writes
// 0.19, counting and emitting 0.06; 51 sorter passes.  The record pass dominates: lane = record reads quality strings byte by byte with nothing coalesced
// (120 GB/s); wave = record for the quality sum, as k_bs_gather moves bytes, is the follow-up.
#ifndef DG_MARKDUP_H
#define DG_MARKDUP_H
#include "dg_coverage.h"

#define MD_HD __host__ __device__ __forceinline__
#define MD_THREADS 256               // records / candidates / pairs / ends per workgroup of every kernel here (dg_bam_markdup_granules [0])
#define MD_CROWD 64                  // the most candidates a run of equal h may hold (dg_bam_markdup_granules [2])
#define MD_HASH_BITS 48
#define MD_SCORE_MAX 0xFFFFFu        // 2^20 - 1
#define MD_SCORE_BITS 21             // a pair's score, and (paired first, score) of an end
#define MD_NOT_EXAMINED 0xFFFFFFFFu  // mate[i]: the record plays no part
#define MD_FRAGMENT 0xFFFFFFFEu      // mate[i]: examined, in no pair; every other value: the partner's index
#define MD_DUP_BYTE 0x04u            // 0x400 in byte 19
static_assert(MD_THREADS == BS_THREADS && MD_THREADS == CV_THREADS, "k_md_rec reads k_bs_len's per-workgroup offsets; k_cv_top and k_cv_tails_top serve this file");
enum { MD_ST_CAND = 0, MD_ST_EXAMINED, MD_ST_NBAD /* max of ~index of a record out of range; 0: none */, MD_ST_COUNTS /* pairs << 32 | ends */, MD_ST_CROWDED, MD_ST_DUP_PAIRS,
       MD_ST_FAMILY, MD_ST_DUP_FRAGS, MD_ST_JUNK /* the scan total of a kernel that leaves no sums */, MD_ST_WORDS = 16 };

struct MdRec { bool examined, candidate, bad; uint64_t E, h; uint32_t score; };

MD_HD uint64_t md_hash(const unsigned char *name, uint32_t len, int hash_bits)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint32_t k = 0; k < len; k++) { h ^= (uint64_t)name[k]; h *= 0x100000001b3ull; }
    h ^= h >> 48;
    return hash_bits >= 64 ? h : h & ((1ull << hash_bits) - 1ull);
}
MD_HD uint32_t md_name_len(const BamHead &h) { return h.l_name ? h.l_name - 1u : 0u; }
MD_HD uint32_t md_name_len(const unsigned char *rec) { return md_name_len(bam_head(rec, BAM_FIXED)); }      // (of an examined record: its fixed part lies inside the array)
MD_HD int md_e_bits(int n_chr) { return 34 + bs_chr_bits(n_chr); }
// the record that starts (with its block_size) at rec, `avail` bytes of the array behind rec: everything but the name's hash (h stays 0); hd: its fixed fields
MD_HD MdRec md_record_fields(const unsigned char *rec, uint64_t avail, int n_chr, BamHead &hd)
{
    MdRec r; r.examined = false; r.candidate = false; r.bad = false; r.E = 0; r.h = 0; r.score = 0;
    hd = bam_head(rec, avail);
    const BamHead &h = hd;
    const int32_t refid = h.refid, pos = h.pos;
    const uint32_t flag = h.flag;
    // examined only when the qualities end inside the record and the array; secondary and supplementary records are left out
    r.examined = h.ok && refid >= 0 && refid < n_chr && pos >= 0 && !(flag & 4u) && !(flag & 0x900u) && h.n_cigar > 0u && h.aux_at <= h.size;
    if (!r.examined) return r;
    const uint32_t s = flag >> 4 & 1u;
    uint64_t lead = 0, trail = 0;
    bool seen = false;
    const uint64_t rlen = bam_cigar_walk(rec, h.cigar_at, h.n_cigar, 0, [&](uint32_t op, uint32_t len, uint64_t, uint64_t) {
        if (op == 4u || op == 5u) { if (seen) trail += len; else lead += len; }
        else { seen = true; trail = 0; }
    }).p;
    const int64_t u5 = s ? (int64_t)pos + (int64_t)rlen - 1 + (int64_t)trail : (int64_t)pos - (int64_t)lead;
    const int64_t biased = u5 + (1ll << 31);
    if (biased < 0 || biased >= (1ll << 33)) { r.bad = true; return r; }
    r.E = (uint64_t)(uint32_t)refid << 34 | (uint64_t)biased << 1 | (uint64_t)s;
    uint32_t score = 0;
    for (uint64_t k = 0; k < (uint64_t)h.l_seq; k++) { const uint32_t q = rec[h.qual_at + k]; if (q >= 15u && q <= 93u && score < MD_SCORE_MAX) score += q; }
    r.score = score > MD_SCORE_MAX ? MD_SCORE_MAX : score;
    r.candidate = (flag & 1u) && !(flag & 8u) && ((flag >> 6 & 1u) ^ (flag >> 7 & 1u));
    return r;
}
MD_HD MdRec md_record(const unsigned char *rec, uint64_t avail, int n_chr, int hash_bits)
{
    BamHead h;
    MdRec r = md_record_fields(rec, avail, n_chr, h);
    if (r.candidate) r.h = md_hash(rec + BAM_FIXED, md_name_len(h), hash_bits);
    return r;
}
// bam_rec_start under the name tests/native/markdup_checks.hip calls it by
MD_HD uint64_t md_rec_start(const uint64_t *dst_off, const uint64_t *tile_base, uint32_t i) { return bam_rec_start(dst_off, tile_base, i); }
MD_HD bool md_same_name(const unsigned char *a, const unsigned char *b)
{
    const uint32_t la = md_name_len(a);
    if (la != md_name_len(b)) return false;
    for (uint32_t k = 0; k < la; k++) if (a[BAM_FIXED + k] != b[BAM_FIXED + k]) return false;
    return true;
}
// candidate j of the n_cand hash-sorted candidates (keys = h, vals = the record's index): its partner's index, or MD_FRAGMENT.  *crowded: its run holds more
// than MD_CROWD.  Only examined records are candidates: their names lie inside the array
MD_HD uint32_t md_mate(const uint64_t *keys, const int64_t *vals, uint32_t n_cand, uint32_t j, const unsigned char *sorted, const uint64_t *dst_off, const uint64_t *tile_base, bool *crowded)
{
    const uint64_t k = keys[j];
    uint32_t left = 0, right = 0;
    while (left < MD_CROWD && j >= left + 1u && keys[j - left - 1u] == k) left++;
    while (right < MD_CROWD && j + right + 1u < n_cand && keys[j + right + 1u] == k) right++;
    *crowded = left + right + 1u > MD_CROWD;
    if (*crowded) return MD_FRAGMENT;
    const unsigned char *mine = sorted + bam_rec_start(dst_off, tile_base, (uint32_t)vals[j]);
    uint32_t same = 0, other = 0;
    for (uint32_t t = j - left; t <= j + right; t++) {
        if (t == j) continue;
        if (md_same_name(mine, sorted + bam_rec_start(dst_off, tile_base, (uint32_t)vals[t]))) { same++; other = (uint32_t)vals[t]; }
    }
    if (same != 1u) return MD_FRAGMENT;
    const unsigned char *theirs = sorted + bam_rec_start(dst_off, tile_base, other);
    return ((bam_head(mine, BAM_FIXED).flag ^ bam_head(theirs, BAM_FIXED).flag) & 0x40u) ? other : MD_FRAGMENT;         // (a candidate has exactly one of 0x40 and 0x80)
}
MD_HD bool md_is_rep(uint32_t i, uint32_t mate) { return mate < MD_FRAGMENT && i < mate; }
// what record i adds to the lists: pairs << 32 | ends
MD_HD uint64_t md_counts(uint32_t i, uint32_t mate) { return mate == MD_NOT_EXAMINED ? 0ull : mate == MD_FRAGMENT ? 1ull : md_is_rep(i, mate) ? (1ull << 32 | 2ull) : 0ull; }
MD_HD uint64_t md_pair_score_key(uint32_t sa, uint32_t sb) { return (uint64_t)(2u * MD_SCORE_MAX + 1u - (sa + sb)); }        // larger score first; 21 bits
MD_HD uint64_t md_end_score_key(bool paired, uint32_t score) { return paired ? 0ull : (uint64_t)(1u << 20 | (MD_SCORE_MAX - score)); }   // pairs' ends first
MD_HD uint32_t md_end_record(int64_t v) { return (uint32_t)(v < 0 ? ~v : v); }                                                 // an end's value: index, or ~member
MD_HD uint64_t md_lo(uint64_t a, uint64_t b) { return a < b ? a : b; }
MD_HD uint64_t md_hi(uint64_t a, uint64_t b) { return a < b ? b : a; }
MD_HD unsigned char md_verdict(unsigned char byte19, bool dup) { return (unsigned char)(dup ? byte19 | MD_DUP_BYTE : byte19 & ~MD_DUP_BYTE); }
// sorted pair q (keys = lo, vals = rep): the first of its (lo, hi)?
MD_HD bool md_pair_is_head(const uint64_t *keys, const int64_t *vals, uint32_t q, const uint64_t *E, const uint32_t *mate)
{
    if (q == 0u) return true;
    if (keys[q] != keys[q - 1u]) return true;
    const uint32_t a = (uint32_t)vals[q], b = (uint32_t)vals[q - 1u];
    return md_hi(E[a], E[mate[a]]) != md_hi(E[b], E[mate[b]]);
}
// sorted end q (keys = E): a fragment behind the head of its run
MD_HD bool md_end_is_dup(const uint64_t *keys, const int64_t *vals, uint32_t q) { return vals[q] >= 0 && q > 0u && keys[q] == keys[q - 1u]; }

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MD_THREADS)
k_md_rec(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, int n_chr, int hash_bits,
         uint64_t *__restrict__ E, uint64_t *__restrict__ h, uint32_t *__restrict__ score, uint32_t *__restrict__ mate, uint32_t *__restrict__ cand_off, uint64_t *__restrict__ tile_sum,
         uint64_t *__restrict__ part /* 2 planes: examined | ~bad */)
{
    __shared__ uint64_t s_wave[MD_THREADS / 64];
    __shared__ unsigned long long s_part[2 * (MD_THREADS / 64)];
    const uint32_t i = blockIdx.x * MD_THREADS + threadIdx.x;
    uint64_t mine = 0, examined = 0, nbad = 0;
    if (i < n) {
        MdRec r; r.examined = false; r.candidate = false; r.bad = false; r.E = 0; r.h = 0; r.score = 0;
        const uint64_t at = bam_rec_start(dst_off, tile_base, i);
        if (at < n_raw) r = md_record(sorted + at, n_raw - at, n_chr, hash_bits);
        if (r.bad) nbad = ~(uint64_t)i;
        examined = r.examined ? 1 : 0; mine = r.candidate ? 1 : 0;
        E[i] = r.E; h[i] = r.h; score[i] = r.score; mate[i] = r.examined ? MD_FRAGMENT : MD_NOT_EXAMINED;
    }
    uint64_t all;
    const uint64_t ex = d_wg_exclusive(mine, all, s_wave);
    if (i < n) cand_off[i] = (uint32_t)ex | (mine ? 1u << 31 : 0u);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
    const unsigned long long v[2] = {examined, nbad};
    cv_block_partials(v, 1, s_part, part);
}

// cand_base: k_md_rec's sums, scanned
__global__ void __launch_bounds__(MD_THREADS)
k_md_compact(const uint32_t *__restrict__ cand_off, const uint64_t *__restrict__ cand_base, const uint64_t *__restrict__ h, uint32_t n, uint32_t n_cand, uint64_t *__restrict__ keys, int64_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * MD_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = cand_off[i];
    if (!(o >> 31)) return;
    const uint64_t c = cand_base[blockIdx.x] + (o & 0x7FFFFFFFu);
    if (c < n_cand) { keys[c] = h[i]; vals[c] = (int64_t)i; }
}

__global__ void __launch_bounds__(MD_THREADS)
k_md_mate(const uint64_t *__restrict__ keys, const int64_t *__restrict__ vals, uint32_t n_cand, uint32_t n, const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off,
          const uint64_t *__restrict__ tile_base, uint32_t *__restrict__ mate, uint64_t *__restrict__ part /* 1 plane: candidates in crowded runs */)
{
    __shared__ unsigned long long s_part[MD_THREADS / 64];
    const uint32_t j = blockIdx.x * MD_THREADS + threadIdx.x;
    bool crowded = false;
    if (j < n_cand) {
        const uint32_t i = (uint32_t)vals[j];
        const uint32_t m = md_mate(keys, vals, n_cand, j, sorted, dst_off, tile_base, &crowded);
        if (i < n) mate[i] = m;
    }
    const unsigned long long v[1] = {crowded ? 1ull : 0ull};
    cv_block_partials(v, 1, s_part, part);
}

__global__ void __launch_bounds__(MD_THREADS)
k_md_count(const uint32_t *__restrict__ mate, uint32_t n, uint32_t *__restrict__ cnt_off, uint64_t *__restrict__ tile_sum)
{
    __shared__ uint64_t s_wave[MD_THREADS / 64];
    const uint32_t i = blockIdx.x * MD_THREADS + threadIdx.x;
    const uint64_t mine = i < n ? md_counts(i, mate[i]) : 0ull;
    uint64_t all;
    const uint64_t ex = d_wg_exclusive(mine, all, s_wave);
    if (i < n) cnt_off[i] = (uint32_t)(ex >> 32) << 16 | ((uint32_t)ex & 0xFFFFu);          // (at most 255 pairs and 510 ends in front)
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// cnt_base: k_md_count's sums, scanned; nothing is written at or behind pair n_pairs or end n_ends
__global__ void __launch_bounds__(MD_THREADS)
k_md_emit(const uint32_t *__restrict__ mate, const uint32_t *__restrict__ score, const uint32_t *__restrict__ cnt_off, const uint64_t *__restrict__ cnt_base, uint32_t n, uint32_t n_pairs,
          uint32_t n_ends, uint64_t *__restrict__ pk, int64_t *__restrict__ pv, uint64_t *__restrict__ ek, int64_t *__restrict__ ev)
{
    const uint32_t i = blockIdx.x * MD_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = mate[i];
    if (m == MD_NOT_EXAMINED) return;
    const uint64_t base = cnt_base[blockIdx.x];
    const uint32_t o = cnt_off[i], p = (uint32_t)(base >> 32) + (o >> 16), e = (uint32_t)base + (o & 0xFFFFu);
    if (m == MD_FRAGMENT) { if (e < n_ends) { ek[e] = md_end_score_key(false, score[i]); ev[e] = (int64_t)i; } return; }
    if (!md_is_rep(i, m) || m >= n) return;
    if (p < n_pairs) { pk[p] = md_pair_score_key(score[i], score[m]); pv[p] = (int64_t)i; }
    if (e + 1u < n_ends) { ek[e] = md_end_score_key(true, 0u); ev[e] = ~(int64_t)i; ek[e + 1u] = md_end_score_key(true, 0u); ev[e + 1u] = ~(int64_t)m; }
}

// the next key of the sorted items: what = 0: a pair's hi, 1: a pair's lo, 2: an end's E
__global__ void __launch_bounds__(MD_THREADS)
k_md_rekey(uint64_t *__restrict__ keys, const int64_t *__restrict__ vals, uint32_t n_items, int what, const uint64_t *__restrict__ E, const uint32_t *__restrict__ mate, uint32_t n)
{
    const uint32_t q = blockIdx.x * MD_THREADS + threadIdx.x;
    if (q >= n_items) return;
    const uint32_t i = md_end_record(vals[q]);
    if (i >= n) return;
    if (what == 2) { keys[q] = E[i]; return; }
    const uint32_t m = mate[i];
    if (m >= n) return;
    keys[q] = what == 0 ? md_hi(E[i], E[m]) : md_lo(E[i], E[m]);
}

__global__ void __launch_bounds__(MD_THREADS)
k_md_heads(const uint64_t *__restrict__ keys, const int64_t *__restrict__ vals, uint32_t n_pairs, const uint64_t *__restrict__ E, const uint32_t *__restrict__ mate, uint64_t *__restrict__ tile_last)
{
    __shared__ uint64_t s_last[MD_THREADS / 64];
    const uint32_t q = blockIdx.x * MD_THREADS + threadIdx.x, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t v = cv_wave_fill(q < n_pairs && md_pair_is_head(keys, vals, q, E, mate) ? (uint64_t)q : CV_NONE, lane);
    if (lane == 63u) s_last[wv] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t all = CV_NONE;
        for (uint32_t k = 0; k < MD_THREADS / 64; k++) all = cv_fill(all, s_last[k]);
        tile_last[blockIdx.x] = all;
    }
}

// byte 19 of sorted record i
__device__ __forceinline__ void md_write(unsigned char *sorted, const uint64_t *dst_off, const uint64_t *tile_base, uint32_t i, uint32_t n, unsigned long long n_raw, bool dup)
{
    if (i >= n) return;
    const uint64_t at = bam_rec_start(dst_off, tile_base, i) + 19ull;
    if (at < n_raw) sorted[at] = md_verdict(sorted[at], dup);
}

// tile_prev: k_cv_tails_top over k_md_heads' last heads: the last head in front of the workgroup
__global__ void __launch_bounds__(MD_THREADS)
k_md_flag_pairs(const uint64_t *__restrict__ keys, const int64_t *__restrict__ vals, uint32_t n_pairs, const uint64_t *__restrict__ E, const uint32_t *__restrict__ mate,
                const uint32_t *__restrict__ tile_prev, unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n,
                unsigned long long n_raw, int write, uint64_t *__restrict__ part /* 2 planes: duplicate pairs | the largest family */)
{
    __shared__ uint64_t s_last[MD_THREADS / 64];
    __shared__ unsigned long long s_part[2 * (MD_THREADS / 64)];
    const uint32_t q = blockIdx.x * MD_THREADS + threadIdx.x, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const bool live = q < n_pairs, head = live && md_pair_is_head(keys, vals, q, E, mate);
    const uint64_t w = cv_wave_fill(head ? (uint64_t)q : CV_NONE, lane);
    if (lane == 63u) s_last[wv] = w;
    __syncthreads();
    uint64_t before = (uint64_t)tile_prev[blockIdx.x];
    for (uint32_t k = 0; k < wv; k++) before = cv_fill(before, s_last[k]);
    const uint64_t first = cv_fill(before, w);
    if (live && write) {
        const uint32_t i = (uint32_t)vals[q];
        md_write(sorted, dst_off, tile_base, i, n, n_raw, !head);
        if (i < n) md_write(sorted, dst_off, tile_base, mate[i], n, n_raw, !head);
    }
    const unsigned long long v[2] = {live && !head ? 1ull : 0ull, live ? (unsigned long long)q - first + 1ull : 0ull};
    cv_block_partials(v, 1, s_part, part);
}

__global__ void __launch_bounds__(MD_THREADS)
k_md_flag_ends(const uint64_t *__restrict__ keys, const int64_t *__restrict__ vals, uint32_t n_ends, unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off,
               const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, int write, uint64_t *__restrict__ part /* 1 plane: duplicate fragments */)
{
    __shared__ unsigned long long s_part[MD_THREADS / 64];
    const uint32_t q = blockIdx.x * MD_THREADS + threadIdx.x;
    bool dup = false;
    if (q < n_ends && vals[q] >= 0) {
        dup = md_end_is_dup(keys, vals, q);
        if (write) md_write(sorted, dst_off, tile_base, (uint32_t)vals[q], n, n_raw, dup);
    }
    const unsigned long long v[1] = {dup ? 1ull : 0ull};
    cv_block_partials(v, 1, s_part, part);
}
#endif
#endif
