// dg_sjtab.h -- the splice-junction table on the device: the (g1, g2) tuples of every batch are counted in a hash table that stays in HBM, and at the
// end of the job the table is sorted, mapped to chromosomes and printed as the bytes of junctions.tab (UpdateLocal/GlobalSJMap, Mapping.cpp:532-577;
// OutputSpliceJunctions, Mapping.cpp:683-716).  What holds no atomics -- the key order, the hash, the chromosome look-up, a line's length and bytes -- is
// __host__ __device__ and shared with the CPU suite (tests/native/sj_checks.hip).
//
// Table: open addressing, linear probing, 24 bytes per slot: two 64-bit key words and a 32-bit count.  A key word is the coordinate with its sign bit
// flipped (so unsigned order = signed order, and 0 -- "empty" -- stands for INT64_MIN alone, the one coordinate the table refuses).
//   k_sj_insert   lane = item (a tuple of a batch, a counted entry, or a filled slot of another table).  Equal keys of a wave are combined first, so one
//                 add carries their multiplicity.  A lane claims a slot with two compare-and-swaps and waits for nobody:
//                   word 1: empty -> g1, or it already holds g1; any other value: next position
//                   word 2: empty -> g2, or it already holds g2; any other value: next position (two keys that share g1 simply collide)
//                 Both words are written once and never change, so every lane with the same key takes the same decisions along the same probe sequence:
//                 a key lives in one slot.  The lane that claims word 1 goes straight on to word 2 -- it sets it, or finds it set by a lane with the same
//                 g1 -- so a claimed slot is always filled when the kernel ends, and no lane ever polls: lanes of a wave run in lockstep, a lock held by a
//                 neighbour lane would never be released.  A lane that finds no slot within SJ_PROBES positions appends its item to the overflow list.
//                 Every access to a slot in this kernel is an agent-scope atomic (executed behind the XCDs' L2s), so no cached copy is ever read.
//   k_sj_compact  lane = slot: the filled slots' second key words and slot numbers, densely, and the smallest / largest key word of each kind (the sort
//                 then skips the digits all keys share)
//   k_sj_gather   the first key words in the order the first sort left
//   k_sj_entries  lane = sorted entry: the dg_sj_entry record with its chromosome, its line's length; the workgroup's exclusive scan (dg_scan.h)
//   k_sj_write    lane = entry: the line's bytes at the scanned place
// Sorting is two stable LSD sorts of dg_sort.h, by g2 then by g1; keys are distinct, so the order -- and with it every byte -- does not depend on where
// the slots were.
#ifndef DG_SJTAB_H
#define DG_SJTAB_H
#include "dg_samfmt.h"
#include "dg_scan.h"
#include "dg_wgscan.h"

#define SJ_HD __host__ __device__ __forceinline__
#define SJ_THREADS 256           // items per workgroup of k_sj_insert (dg_sj_granules [0])
#define SJ_MIN_SLOTS 256         // dg_sj_granules [1]
#define SJ_FIRST_SLOTS 65536     // a table nobody reserved
#define SJ_PROBES 32
#define SJ_NO_CHR 0xFFFFFFFFu
enum { SJ_SRC_TUPLES = 0, SJ_SRC_ENTRIES = 1, SJ_SRC_SLOTS = 2 };
// the table's small device state, 64-bit words
enum { SJ_ST_OVERFLOW = 0, SJ_ST_DISTINCT, SJ_ST_REFUSED, SJ_ST_ENTRIES, SJ_ST_NMIN1 /* max of ~word = ~min */, SJ_ST_MAX1, SJ_ST_NMIN2, SJ_ST_MAX2, SJ_ST_LINES, SJ_ST_BYTES, SJ_ST_WORDS = 16 };

struct SjSlot { unsigned long long k1, k2; unsigned int cnt, pad; };
static_assert(sizeof(SjSlot) == 24 && sizeof(dg_sj_entry) == 24 && sizeof(dg_sj_out) == 24, "tuples, entries and slots are 24 bytes");

SJ_HD unsigned long long sj_bias(long long g) { return (unsigned long long)g ^ 0x8000000000000000ull; }
SJ_HD long long sj_unbias(unsigned long long w) { return (long long)(w ^ 0x8000000000000000ull); }
SJ_HD bool sj_key_ok(long long g1, long long g2) { return sj_bias(g1) != 0ull && sj_bias(g2) != 0ull; }
// std::map<pair<int64, int64>> order: signed, g1 first
SJ_HD bool sj_key_less(long long a1, long long a2, long long b1, long long b2) { return a1 != b1 ? a1 < b1 : a2 < b2; }
SJ_HD unsigned long long sj_hash(unsigned long long w1, unsigned long long w2)
{
    unsigned long long h = w1 * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    h += w2 * 0xC2B2AE3D27D4EB4Full;
    h ^= h >> 32; h *= 0xD6E8FEB86659FD93ull; h ^= h >> 32;
    return h;
}
// how many low bits two sorted-by extremes differ in: every key between them shares the digits above
SJ_HD int sj_key_bits(unsigned long long lo, unsigned long long hi) { int b = 0; for (unsigned long long x = lo ^ hi; x; x >>= 1) b++; return b; }
// the chromosome of an entry: ChrLocMap.lower_bound(g1) (Mapping.cpp:683-695); past the last key: no line
SJ_HD uint32_t sj_chr_of(const LocTab &t, long long g1)
{
    const int lo = d_loc_lower_bound(t, (int64_t)g1);
    return lo >= t.n2 ? SJ_NO_CHR : (uint32_t)t.chr[lo];
}
// "%s\t%lld\t%lld\t%d\n": both positions relative to the chromosome of g1
SJ_HD void sj_line_numbers(SamSink &o, long long chr_off, long long g1, long long g2, uint32_t count)
{
    o.ch('\t'); sam_put_num(o, (long long)((unsigned long long)g1 + 1ull - (unsigned long long)chr_off));
    o.ch('\t'); sam_put_num(o, (long long)((unsigned long long)g2 + 1ull - (unsigned long long)chr_off));
    o.ch('\t'); sam_put_num(o, (long long)(int32_t)count);
    o.ch('\n');
}
SJ_HD uint32_t sj_line_len(const uint32_t *name_off, uint32_t chr, long long chr_off, long long g1, long long g2, uint32_t count)
{
    SamSink o{nullptr, 0, 0};
    sj_line_numbers(o, chr_off, g1, g2, count);
    return o.n + (name_off[chr + 1] - name_off[chr]);
}
SJ_HD uint32_t sj_line_write(char *out, const uint32_t *name_off, const char *names, uint32_t chr, long long chr_off, long long g1, long long g2, uint32_t count)
{
    SamSink o{out, 0, 0xFFFFFFFFu};
    for (uint32_t i = name_off[chr]; i < name_off[chr + 1]; i++) o.ch(names[i]);
    sj_line_numbers(o, chr_off, g1, g2, count);
    return o.n;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long sj_cas(unsigned long long *p, unsigned long long want)
{
    unsigned long long old = 0ull;      // empty -> want; returns what the word held before
    __hip_atomic_compare_exchange_strong(p, &old, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return old;
}

__global__ void __launch_bounds__(SJ_THREADS)
k_sj_insert(const unsigned char *__restrict__ src, unsigned long long n, int kind, SjSlot *tab, unsigned long long mask,
            dg_sj_entry *__restrict__ ovf, unsigned long long ovf_cap, unsigned long long *stat)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * SJ_THREADS + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    long long g1 = 0, g2 = 0; unsigned long long cnt = 0;
    if (i < n) {
        if (kind == SJ_SRC_SLOTS) {
            const SjSlot *s = (const SjSlot *)src + i;
            if (s->k1 && s->k2) { g1 = sj_unbias(s->k1); g2 = sj_unbias(s->k2); cnt = s->cnt; }
        } else {                                            // dg_sj_out and dg_sj_entry both begin with g1, g2; the word behind is the count of an entry
            const dg_sj_entry *e = (const dg_sj_entry *)src + i;
            g1 = e->g1; g2 = e->g2; cnt = kind == SJ_SRC_ENTRIES ? e->count : 1u;
        }
    }
    if (cnt && !sj_key_ok(g1, g2)) { atomicAdd(stat + SJ_ST_REFUSED, 1ull); cnt = 0; }
    if (kind != SJ_SRC_SLOTS) {
        // equal keys of the wave become one item (the loop and everything in it is wave-uniform: `todo` is a ballot)
        bool active = cnt != 0;
        unsigned long long todo = __ballot(active);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const long long l1 = __shfl(g1, leader, 64), l2 = __shfl(g2, leader, 64);
            const bool same = active && g1 == l1 && g2 == l2;
            const unsigned long long m = __ballot(same);
            if (m & (m - 1ull)) {
                unsigned long long v = same ? cnt : 0ull;
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == leader) cnt = v; else if (same) { cnt = 0; active = false; }
            }
            todo &= ~m;
        }
    }
    if (!cnt) return;
    const unsigned long long w1 = sj_bias(g1), w2 = sj_bias(g2);
    unsigned long long p = sj_hash(w1, w2) & mask;
    for (int t = 0; t < SJ_PROBES; t++, p = (p + 1ull) & mask) {
        SjSlot *s = tab + p;
        const unsigned long long o1 = sj_cas(&s->k1, w1);
        if (o1 != 0ull && o1 != w1) continue;
        const unsigned long long o2 = sj_cas(&s->k2, w2);
        if (o2 != 0ull && o2 != w2) continue;
        if (o2 == 0ull) atomicAdd(stat + SJ_ST_DISTINCT, 1ull);
        atomicAdd(&s->cnt, (unsigned int)cnt);
        return;
    }
    const unsigned long long at = atomicAdd(stat + SJ_ST_OVERFLOW, 1ull);
    if (at < ovf_cap) { dg_sj_entry e; e.g1 = g1; e.g2 = g2; e.count = (uint32_t)cnt; e.chr = 0; ovf[at] = e; }
}

__global__ void __launch_bounds__(SJ_THREADS)
k_sj_compact(const SjSlot *__restrict__ tab, unsigned long long n_slots, unsigned long long cap, uint64_t *__restrict__ keys, int64_t *__restrict__ vals, unsigned long long *stat)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * SJ_THREADS + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long k1 = 0, k2 = 0;
    if (i < n_slots) { k1 = tab[i].k1; k2 = tab[i].k2; }
    const bool filled = k1 != 0ull && k2 != 0ull;
    const unsigned long long m = __ballot(filled);
    if (!m) return;
    unsigned long long base = 0;
    const int leader = __ffsll((long long)m) - 1;
    if (lane == leader) base = atomicAdd(stat + SJ_ST_ENTRIES, (unsigned long long)__popcll(m));
    base = __shfl(base, leader, 64);
    const unsigned long long at = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
    if (filled && at < cap) { keys[at] = k2; vals[at] = (int64_t)i; }
    const unsigned long long a = d_wave_max(filled ? ~k1 : 0ull), b = d_wave_max(filled ? k1 : 0ull), c = d_wave_max(filled ? ~k2 : 0ull), d = d_wave_max(filled ? k2 : 0ull);
    if (lane == leader) { atomicMax(stat + SJ_ST_NMIN1, a); atomicMax(stat + SJ_ST_MAX1, b); atomicMax(stat + SJ_ST_NMIN2, c); atomicMax(stat + SJ_ST_MAX2, d); }
}

__global__ void __launch_bounds__(256)
k_sj_gather(const SjSlot *__restrict__ tab, const int64_t *__restrict__ vals, uint32_t n, uint64_t *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i] = tab[vals[i]].k1;
}

struct SjPrint { const int64_t *loc_key; const int32_t *loc_chr; const int64_t *chr_off; int n2; const uint32_t *name_off; const char *names; /* nullptr: entries only */ };

__global__ void __launch_bounds__(SJ_THREADS)
k_sj_entries(const SjSlot *__restrict__ tab, const int64_t *__restrict__ vals, uint32_t n, const SjPrint pr, dg_sj_entry *__restrict__ entries,
             uint64_t *__restrict__ line_off, uint64_t *__restrict__ tile_sum, unsigned long long *stat)
{
    __shared__ unsigned long long s_scan[16];
    const uint32_t i = blockIdx.x * SJ_THREADS + threadIdx.x;
    Triple mine; mine.x = 0; mine.y = 0; mine.z = 0; mine.w = 0;
    if (i < n) {
        const SjSlot s = tab[vals[i]];
        dg_sj_entry e; e.g1 = sj_unbias(s.k1); e.g2 = sj_unbias(s.k2); e.count = s.cnt;
        e.chr = sj_chr_of(LocTab{pr.loc_key, pr.loc_chr, pr.chr_off, pr.n2}, e.g1);
        entries[i] = e;
        if (e.chr != SJ_NO_CHR) {
            mine.x = 1;
            if (pr.names) mine.z = sj_line_len(pr.name_off, e.chr, pr.chr_off[e.chr], e.g1, e.g2, e.count);
        }
    }
    Triple tot;
    const Triple ex = d_block_exclusive(mine, tot, s_scan);
    if (i < n) line_off[i] = ex.z;
    if (threadIdx.x == 0) { tile_sum[blockIdx.x] = tot.z; if (tot.x) atomicAdd(stat + SJ_ST_LINES, (unsigned long long)tot.x); }
}

__global__ void __launch_bounds__(SJ_THREADS)
k_sj_write(const dg_sj_entry *__restrict__ entries, uint32_t n, const SjPrint pr, const uint64_t *__restrict__ line_off, const uint64_t *__restrict__ tile_base,
           const unsigned long long *__restrict__ stat, unsigned long long cap, char *__restrict__ out)
{
    const uint32_t i = blockIdx.x * SJ_THREADS + threadIdx.x;
    if (i >= n || stat[SJ_ST_BYTES] > cap) return;
    const dg_sj_entry e = entries[i];
    if (e.chr == SJ_NO_CHR) return;
    sj_line_write(out + tile_base[blockIdx.x] + line_off[i], pr.name_off, pr.names, e.chr, pr.chr_off[e.chr], e.g1, e.g2, e.count);
}
#endif
#endif
