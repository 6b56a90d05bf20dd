// dg_pileup.h -- allele counts of the coordinate-sorted BAM: a table of the positions at which a read shows something else than the reference, built in HBM
// next to the sort (dg_bamsort.h).  After dg_bam_sort_finish the device holds the records in coordinate order with their 4-bit bases and CIGARs, the duplicate
// flags of dg_bam_markdup_finish, and the reference itself as the index's 2-bit text: what `samtools mpileup`, `bam-readcount` or `pysamstats` compute from
// the file, read back and inflated, on one core.  The reference program has no such output: an opt-in extension.
//
// THE DEFINITION.  No pileup tool exists where this project is built and tested: this text is what the tests pin (tests/pileup_inputs.py is its sequential twin).
//
// Per sorted record (its fields, CIGAR and packed bases as bam_head and bam_cigar_walk of dg_bamrec.h give them):
//   counted  everything the coverage track asks (0 <= refID < n_chr; pos >= 0; flag & 4 clear; n_cigar_op > 0; (flag & exclude_flags) == 0; mapq >= min_mapq;
//            the CIGAR inside the record and the array), and: the packed bases inside the record and the array; l_seq > 0; the CIGAR's read length (the sum
//            of M, I, S, =, X) == l_seq; the record ends on its chromosome, pos + rlen <= chr_len[refID] (rlen: the sum of M, D, N, =, X).  A record that fails
//            only one or both of the last two is not counted and tallied in stats[8].
//   range    a block end above 2^32 - 1 on a record that passes the coverage track's conditions: DG_ERR_RANGE, the text names the record's index.  Tested
//            before the four further conditions: on a chromosome shorter than 2^32 - 1 a block that ends AT 2^32 - 1 is a stats[8] tally, one past it the error.
//   strand   s = flag >> 4 & 1: the READ's orientation, which is what strand-bias filters look at -- NOT the coverage track's transcript strand (there a
//            second mate counts for the opposite strand; here it does not).
//   walk     p = pos, q = 0.  M, =, X of length L: read base q + k is observed at reference position p + k for every k < L, then p += L, q += L; L > 0 is also a
//            block [p, p + L).  D: every position p .. p + L - 1 gets one DEL observation, p += L.  N: p += L.  I of length L > 0: one INS observation at the
//            anchor max(p, pos + 1) - 1 (the reference base in front of the insertion, or the read's first position when nothing precedes it), q += L.
//            S: q += L.  H, P: nothing.
//   alleles  codes A C G T N DEL INS = 1 .. 7 in the key, 0 .. 6 in the entry.  The reference base at (chr, p) is d_refchar(ix, chr_off[chr] + p): the base the
//            index's 2-bit text holds, so an N of the FASTA is whatever base the indexer stored there.  A read nibble 1, 2, 4, 8 is A, C, G, T; nibble 0 ('=')
//            is the reference base; every other nibble is N.  A base observation is an event only when its allele differs from the reference base; the CIGAR
//            op (M, = or X) plays no part in that.
// Events.  Key chr << 35 | position << 3 | code, a 64-bit value.  Code 0 is a depth event: every block gives (start, +(1 + (s << 32))) and (end, -(1 + (s << 32))):
//   two 32-bit counters travel in one word, sums are exact modulo 2^64 and every prefix is a true pair of non-negative counts.  Codes 1 .. 7 carry 1 + (s << 32).
//   Depth events sort in front of the allele events of their position: the running sum of the code-0 values, read at an allele event, is depth | depth_rev << 32
//   there (the starts at the position included, the ends excluded); the sum of the values of a run of equal keys is that allele's n | n_rev << 32.
// Sites.  A position with at least one allele event.  dg_site_entry { chr, pos, depth, depth_rev, ref (0..3), top, n[7], n_rev[7] }: n[0..4] the A, C, G, T, N
//   observed there, the reference allele's own count filled in as depth - (the other four), so n[0] + .. + n[4] == depth, on both strands; n[5], n[6] deleted
//   bases and insertions, outside the depth; top the non-reference allele (DEL, INS included) with the largest n, ties to the smallest code; kept when
//   n[top] >= min_alt.  Kept sites ascend in (chr, pos).
// Text.  Per kept site "name\tpos+1\tR\tdepth\tdepth_rev\tA\tC\tG\tT\tN\tDEL\tINS\tA_rev\t..\tINS_rev\n", decimal, no header line.
// The result is a function of the record SET: not of order, grid, batch split, ordinals, contexts or growth history (sums of equal keys do not depend on the
// order inside a run; no kernel here uses an atomic).
//
// The base comparison is the hot loop, sixteen bases a step (PU_STEP): sixteen read nibbles become 2-bit codes and two masks (ACGT, '='), the text's sixteen
// 2-bit symbols come from one unaligned fetch of pac at the right shift, an XOR leaves the mismatches as a bit mask.  The counting walk takes its popcount, the
// emitting walk scans its bits: ONE templated walk (pu_walk), so both give the same events by construction.
//
//   k_pu_count      lane = sorted record: filter, pre-walk of the CIGAR, the walk; the workgroup's exclusive scan of the event counts; per workgroup the
//                   counters, the key bounds and the first record out of range (k_cv_top, twice: it takes five planes a call)
//   -- the first wait: the number of events sizes the sorter's buffers; a record out of range ends the call --
//   k_pu_emit       lane = sorted record: the same walk, event k of the record at its scanned place
//   (sort)          one stable radix sort of the events over the key bits in which the bounds differ
//   k_pu_scan       lane = sorted event: two planes, the code-0 values and the allele values, each an inclusive workgroup scan (k_tiles_top carries both)
//   k_pu_tails      lane = event: the last event of a run of equal keys (a tail) carries its own index + 1; per workgroup its last tail
//   k_cv_tails_top  (dg_coverage.h) the last-valid scan over those: every workgroup knows the last tail in front of it
//   k_pu_flag       lane = event: the last-valid scan inside the workgroup; a tail with code > 0 is a distinct allele key, the first of its position a site;
//                   the workgroup's scan of both counts (k_tiles_top over sites << 32 | keys)
//   -- the second wait: the numbers of distinct allele keys and of sites --
//   k_pu_compact    lane = event: allele key j gets its key, its run's sum and the depth; site t the number of its first key
//   k_pu_sites      lane = site: looks at most 7 keys ahead, builds the entry, applies the filter, measures the line; two scans (kept sites, bytes)
//   -- the third wait: the kept sites and the text's size, both buffers exact --
//   k_pu_write      lane = site: the same entry again, stored at its scanned place with its line
// Memory: 8 bytes per record; 56 bytes per event (the sorter's pairs, two scanned planes, the previous tail, the mark) and the sorter's histograms; 24 per
// distinct allele key; 12 per site; 80 per kept site and its line.  Everything a lane computes is host-callable: tests/native/pileup_checks.hip runs it on the CPU.
#ifndef DG_PILEUP_H
#define DG_PILEUP_H
#include "dg_common.h"
#include "dg_samfmt.h"
#include "dg_coverage.h"

#define PU_HD __host__ __device__ __forceinline__
#define PU_WG CV_THREADS             // records / events / sites per workgroup (dg_bam_pileup_granules [0])
#define PU_STEP 16                   // reference bases per packed compare step (dg_bam_pileup_granules [2])
enum { PU_A = 1, PU_C, PU_G, PU_T, PU_N, PU_DEL, PU_INS };
// the call's small device state, 64-bit words.  k_cv_top's outputs lie side by side: sums first, then maxima
enum { PU_ST_EVENTS = 0, PU_ST_RECS /* counted | left out << 32 */, PU_ST_ALIGNED, PU_ST_BLK_INS /* blocks | insertions << 32 */, PU_ST_MIS_DEL /* mismatches | deleted << 32 */,
       PU_ST_NBAD /* max of ~index of a record out of range; 0: none */, PU_ST_JUNK, PU_ST_NMIN /* max of ~lower key bound */, PU_ST_MAX, PU_ST_DEPTH_END /* the code-0 plane's total: 0 */,
       PU_ST_ALLELES /* the allele plane's total */, PU_ST_MARKS /* sites << 32 | distinct allele keys */, PU_ST_KEPT, PU_ST_MAX_DEPTH, PU_ST_BYTES, PU_ST_WORDS = 16 };

struct PuFilter { uint32_t exclude, min_mapq; };
enum { PU_SKIP = 0, PU_COUNTED, PU_LEFT_OUT, PU_RANGE };
struct PuRec { int state; int32_t refid, pos; uint32_t n_ops, l_seq, s; uint64_t cigar_at, seq_at, rlen; };
struct PuTally { uint64_t events, aligned; uint32_t blocks, mism, del, ins; };

static_assert(sizeof(dg_site_entry) == 80, "an entry is 80 bytes");

PU_HD uint64_t pu_key(uint32_t chr, uint64_t position, uint32_t code) { return (uint64_t)chr << 35 | position << 3 | code; }
PU_HD int pu_key_bits_max(int n_chr) { return 35 + bs_chr_bits(n_chr); }
PU_HD int64_t pu_chr_len(const DIndex &ix, int32_t refid) { return ix.loc_key[refid] + 1 - ix.chr_off[refid]; }     // (ChrLocMap's forward keys are the chromosomes' last bases)
PU_HD uint64_t pu_value(uint32_t s) { return 1ull + ((uint64_t)s << 32); }

// the record at rec with the fixed fields h: what the coverage track counts, with the packed bases inside the record and the array and l_seq != 0; PU_RANGE comes
// before those two, PU_LEFT_OUT behind them
PU_HD PuRec pu_record(const unsigned char *rec, const BamHead &h, const DIndex &ix, const PuFilter &f)
{
    const CvFilter cf{0u, f.exclude, f.min_mapq};
    const CvRec c = cv_record(h, ix.n_chr, cf);
    PuRec r; r.state = PU_SKIP; r.refid = c.refid; r.pos = c.pos; r.n_ops = c.n_ops; r.cigar_at = c.cigar_at; r.l_seq = 0; r.s = 0; r.seq_at = 0; r.rlen = 0;
    if (!c.counted) return r;
    r.l_seq = h.l_seq; r.s = h.flag >> 4 & 1u; r.seq_at = h.seq_at;
    bool bad = false;
    const BamAt end = bam_cigar_walk(rec, c.cigar_at, c.n_ops, (uint64_t)c.pos, [&](uint32_t op, uint32_t len, uint64_t p, uint64_t) {
        if (bam_op_aligned(op) && len && p + len > CV_MAX_POS) bad = true;
    });
    r.rlen = end.p - (uint64_t)c.pos;
    if (bad) { r.state = PU_RANGE; return r; }
    if (h.qual_at > h.size || r.l_seq == 0u) return r;
    r.state = end.q == (uint64_t)r.l_seq && (int64_t)end.p <= pu_chr_len(ix, c.refid) ? PU_COUNTED : PU_LEFT_OUT;
    return r;
}
// the record that starts (with its block_size) at rec, `avail` bytes of the array behind rec
PU_HD PuRec pu_record(const unsigned char *rec, uint64_t avail, const DIndex &ix, const PuFilter &f) { return pu_record(rec, bam_head(rec, avail), ix, f); }

// sixteen symbols of the forward text from g on as 2-bit codes, the first in the top bits.  One unaligned fetch of pac at the right shift; a window that
// reaches the last bytes of the array goes base by base (on the device pac holds both strands and a pad: the forward text never gets there)
PU_HD uint32_t pu_ref16(const DIndex &ix, int64_t g)
{
    const int64_t limit = d_pac_both(ix) ? 2 * ix.l_pac : ix.l_pac;
    if (g >= 0 && g + 20 <= limit) {
        const uint8_t *b = ix.pac + (g >> 2);
        const uint64_t w = (uint64_t)__builtin_bswap32(*(const uint32_a1 *)b) << 8 | b[4];
        return (uint32_t)(w >> (8u - (((uint32_t)g & 3u) << 1)));
    }
    uint32_t out = 0;
    for (int k = 0; k < PU_STEP; k++) out |= (uint32_t)(d_nt4((unsigned char)d_refchar(ix, g + k)) & 3u) << (30 - 2 * k);
    return out;
}
// bits 0, 1 of each of sixteen nibbles, packed: nibble i from the top becomes pair i from the top
PU_HD uint32_t pu_squeeze(uint64_t x)
{
    x &= 0x3333333333333333ull;
    x = (x | x >> 2) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | x >> 4) & 0x00FF00FF00FF00FFull;
    x = (x | x >> 8) & 0x0000FFFF0000FFFFull;
    return (uint32_t)(x | x >> 16);
}
// sixteen read bases from base q on, as stored (4 bits each), the first in the top nibble; bytes behind the last base read as 0
PU_HD uint64_t pu_nibbles16(const unsigned char *seq, uint32_t l_seq, uint32_t q)
{
    const uint32_t n_bytes = (l_seq + 1u) / 2u, at = q >> 1;
    uint64_t w = 0; uint32_t next = 0;
    if (at + 9u <= n_bytes) {
        const uint2_a1 v = *(const uint2_a1 *)(seq + at);
        w = (uint64_t)__builtin_bswap32(v.x) << 32 | __builtin_bswap32(v.y); next = seq[at + 8u];
    } else {
        for (uint32_t j = 0; j < 8u; j++) w = w << 8 | (at + j < n_bytes ? (uint64_t)seq[at + j] : 0ull);
        if (at + 8u < n_bytes) next = seq[at + 8u];
    }
    return q & 1u ? w << 4 | next >> 4 : w;
}
// one step of the comparison: the mismatches among the first n (1 .. 16) of sixteen bases as a mask (base k: bit 30 - 2 k), with the read's 2-bit codes and its
// ACGT mask for the emitting walk
struct PuStep { uint32_t mis, codes, acgt; };
PU_HD PuStep pu_compare16(uint64_t nib, uint32_t ref, uint32_t n)
{
    const uint64_t one = 0x1111111111111111ull;
    const uint64_t b0 = nib & one, b1 = nib >> 1 & one, b2 = nib >> 2 & one, b3 = nib >> 3 & one;
    const uint64_t sum = b0 + b1 + b2 + b3;                                  // 0 .. 4 per nibble
    const uint64_t onehot = sum & ~(sum >> 1) & ~(sum >> 2) & one, zero = ~(b0 | b1 | b2 | b3) & one;
    PuStep s;
    s.codes = pu_squeeze((b1 | b3) | (b2 | b3) << 1);                       // 1, 2, 4, 8 -> 0, 1, 2, 3
    const uint32_t flags = pu_squeeze(onehot | zero << 1), eq = flags >> 1 & 0x55555555u;
    s.acgt = flags & 0x55555555u;
    const uint32_t x = s.codes ^ ref, differ = (x | x >> 1) & 0x55555555u;
    const uint32_t valid = n >= 16u ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> (2u * n));
    s.mis = ((differ & s.acgt) | (~s.acgt & ~eq & 0x55555555u)) & valid;    // a base that is neither ACGT nor '=' is an N: never the reference base
    return s;
}
PU_HD uint32_t pu_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }
PU_HD uint32_t pu_clz(uint32_t x) { return (uint32_t)__builtin_clz(x); }      // (x != 0)

// The walk of a counted record.  Event k of the record goes to the sink: f.depth(k, start, end) leaves two, f.bases(k, p, step) one per set bit of step.mis in
// ascending position, f.del(k, p, len) len, f.ins(k, anchor) one.  Returns what the counting pass tallies; k advances the same way whatever the sink does.
template <class F>
PU_HD PuTally pu_walk(const unsigned char *rec, const PuRec &r, const DIndex &ix, F &f)
{
    PuTally t; t.events = 0; t.aligned = 0; t.blocks = 0; t.mism = 0; t.del = 0; t.ins = 0;
    const unsigned char *seq = rec + r.seq_at;
    const int64_t g0 = ix.chr_off[r.refid];
    bam_cigar_walk(rec, r.cigar_at, r.n_ops, (uint64_t)r.pos, [&](uint32_t op, uint32_t len, uint64_t p, uint64_t q) {
        if (!len) return;
        if (bam_op_aligned(op)) {
            f.depth(t.events, p, p + len); t.events += 2; t.blocks++; t.aligned += len;
            for (uint32_t k = 0; k < len; k += PU_STEP) {
                const PuStep st = pu_compare16(pu_nibbles16(seq, r.l_seq, (uint32_t)q + k), pu_ref16(ix, g0 + (int64_t)(p + k)), len - k);
                if (st.mis) { f.bases(t.events, p + k, st); const uint32_t m = pu_popc(st.mis); t.events += m; t.mism += m; }
            }
        } else if (op == 2u) { f.del(t.events, p, len); t.events += len; t.del += len; }
        else if (op == 1u) { f.ins(t.events, (p > (uint64_t)r.pos + 1 ? p : (uint64_t)r.pos + 1) - 1); t.events++; t.ins++; }
    });
    return t;
}
struct PuNoSink {                   // k_pu_count's walk: the tally is all it wants
    PU_HD void depth(uint64_t, uint64_t, uint64_t) {}
    PU_HD void bases(uint64_t, uint64_t, const PuStep &) {}
    PU_HD void del(uint64_t, uint64_t, uint32_t) {}
    PU_HD void ins(uint64_t, uint64_t) {}
};
struct PuEmit {                     // k_pu_emit's: event `first + k` of the array, nothing written at or behind event `limit`
    uint64_t *keys; int64_t *vals; uint64_t first, limit; uint32_t chr, s;
    PU_HD void put(uint64_t k, uint64_t position, uint32_t code, bool minus)
    {
        const uint64_t e = first + k;
        if (e < limit) { keys[e] = pu_key(chr, position, code); vals[e] = minus ? -(int64_t)pu_value(s) : (int64_t)pu_value(s); }
    }
    PU_HD void depth(uint64_t k, uint64_t start, uint64_t end) { put(k, start, 0u, false); put(k + 1, end, 0u, true); }
    PU_HD void bases(uint64_t k, uint64_t p, const PuStep &st)
    {
        for (uint32_t m = st.mis; m; k++) {
            const uint32_t z = pu_clz(m), b = z >> 1;                        // base b of the step: bit 30 - 2 b
            m &= ~(0x80000000u >> z);
            put(k, p + b, (st.acgt >> (30u - 2u * b) & 1u) ? PU_A + (st.codes >> (30u - 2u * b) & 3u) : (uint32_t)PU_N, false);
        }
    }
    PU_HD void del(uint64_t k, uint64_t p, uint32_t len) { for (uint32_t i = 0; i < len; i++) put(k + i, p + i, PU_DEL, false); }
    PU_HD void ins(uint64_t k, uint64_t anchor) { put(k, anchor, PU_INS, false); }
};
// bounds of a counted record's keys: every event lies on [pos, pos + rlen]
PU_HD uint64_t pu_key_lo(const PuRec &r) { return pu_key((uint32_t)r.refid, (uint64_t)r.pos, 0u); }
PU_HD uint64_t pu_key_hi(const PuRec &r) { return pu_key((uint32_t)r.refid, (uint64_t)r.pos + r.rlen, 7u); }

// the two planes of a sorted event
PU_HD uint64_t pu_plane_depth(uint64_t key, int64_t val) { return (key & 7u) ? 0ull : (uint64_t)val; }
PU_HD uint64_t pu_plane_allele(uint64_t key, int64_t val) { return (key & 7u) ? (uint64_t)val : 0ull; }
// a tail with an allele code is a distinct allele key; it opens a site when the distinct key in front of it (key_prev, if there is one) lies elsewhere or is a depth key
PU_HD bool pu_is_allele_key(bool tail, uint64_t key) { return tail && (key & 7u) != 0u; }
PU_HD bool pu_opens_site(bool allele_key, uint64_t key, bool has_prev, uint64_t key_prev) { return allele_key && (!has_prev || (key_prev >> 3) != (key >> 3) || (key_prev & 7u) == 0u); }

// the site whose first distinct allele key is j (of n_keys): at most seven keys share its position
struct PuSite { dg_site_entry e; bool kept; };
PU_HD PuSite pu_site(const uint64_t *ak_key, const uint64_t *ak_n, const uint64_t *ak_depth, uint64_t j, uint64_t n_keys, const DIndex &ix, uint32_t min_alt)
{
    PuSite s;
    const uint64_t key = ak_key[j], at = key >> 3;
    s.e.chr = (uint32_t)(key >> 35); s.e.pos = (uint32_t)at;
    s.e.depth = (uint32_t)ak_depth[j]; s.e.depth_rev = (uint32_t)(ak_depth[j] >> 32);
    // (every array index below is a constant once the loops are unrolled: the counts stay in registers)
    uint64_t v[7] = {0, 0, 0, 0, 0, 0, 0};                                    // n | n_rev << 32 per allele
    bool live = true;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        live = live && j + (uint64_t)k < n_keys && (ak_key[j + (uint64_t)k] >> 3) == at;
        if (live) {
            const uint32_t code = (uint32_t)(ak_key[j + (uint64_t)k] & 7u);
            const uint64_t n = ak_n[j + (uint64_t)k];
#pragma unroll
            for (int a = 0; a < 7; a++) if (code == (uint32_t)a + 1u) v[a] = n;
        }
    }
    s.e.ref = s.e.chr < (uint32_t)ix.n_chr ? (uint32_t)d_nt4((unsigned char)d_refchar(ix, ix.chr_off[s.e.chr] + (int64_t)s.e.pos)) & 3u : 0u;
    uint32_t others = 0, others_rev = 0;
#pragma unroll
    for (int a = 0; a < 5; a++) if ((uint32_t)a != s.e.ref) { others += (uint32_t)v[a]; others_rev += (uint32_t)(v[a] >> 32); }
    const uint64_t own = (uint64_t)(s.e.depth - others) | (uint64_t)(s.e.depth_rev - others_rev) << 32;
    uint32_t top = 7u, top_n = 0;
#pragma unroll
    for (int a = 0; a < 7; a++) {
        if ((uint32_t)a == s.e.ref) v[a] = own;
        else if (top == 7u || (uint32_t)v[a] > top_n) { top = (uint32_t)a; top_n = (uint32_t)v[a]; }
        s.e.n[a] = (uint32_t)v[a]; s.e.n_rev[a] = (uint32_t)(v[a] >> 32);
    }
    s.e.top = top;
    s.kept = top_n >= min_alt;
    return s;
}
// "%s\t%u\t%c\t%u\t%u" and fourteen "\t%u", "\n"
PU_HD void pu_line_numbers(SamSink &o, const dg_site_entry &e)
{
    o.ch('\t'); sam_put_num(o, (long long)e.pos + 1);
    o.ch('\t'); o.ch((char)(0x54474341u >> (8u * (e.ref & 3u))));
    o.ch('\t'); sam_put_num(o, (long long)e.depth);
    o.ch('\t'); sam_put_num(o, (long long)e.depth_rev);
    for (int a = 0; a < 7; a++) { o.ch('\t'); sam_put_num(o, (long long)e.n[a]); }
    for (int a = 0; a < 7; a++) { o.ch('\t'); sam_put_num(o, (long long)e.n_rev[a]); }
    o.ch('\n');
}
PU_HD uint32_t pu_line_len(const uint32_t *name_off, const dg_site_entry &e)
{
    SamSink o{nullptr, 0, 0};
    pu_line_numbers(o, e);
    return o.n + (name_off[e.chr + 1] - name_off[e.chr]);
}
PU_HD uint32_t pu_line_write(char *out, const uint32_t *name_off, const char *names, const dg_site_entry &e)
{
    SamSink o{out, 0, 0xFFFFFFFFu};
    for (uint32_t i = name_off[e.chr]; i < name_off[e.chr + 1]; i++) o.ch(names[i]);
    pu_line_numbers(o, e);
    return o.n;
}
// an event's mark: the allele keys and sites in front of it in its workgroup (at most 255 each), and what it is itself
PU_HD uint32_t pu_mark(uint32_t counts_before, bool ak, bool site) { return cv_mark(counts_before, ak, site); }
PU_HD uint32_t pu_mark_keys(uint32_t m) { return cv_mark_bps(m); }
PU_HD uint32_t pu_mark_sites(uint32_t m) { return cv_mark_ents(m); }
// a site's mark: the kept sites in front of it in its workgroup, and whether it is kept
PU_HD uint32_t pu_site_mark(uint32_t kept_before, bool kept) { return kept_before | (kept ? 1u << 31 : 0u); }

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PU_WG)
k_pu_count(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, const DIndex ix,
           const PuFilter f, uint64_t *__restrict__ ev_off, uint64_t *__restrict__ tile_sum, uint64_t *__restrict__ part /* 5 planes: four sums | ~bad */,
           uint64_t *__restrict__ part2 /* 2 planes: ~lower key bound, upper */)
{
    __shared__ uint64_t s_wave[PU_WG / 64];
    __shared__ unsigned long long s_part[5 * (PU_WG / 64)], s_part2[2 * (PU_WG / 64)];
    const uint32_t i = blockIdx.x * PU_WG + threadIdx.x;
    uint64_t mine = 0, recs = 0, aligned = 0, blk_ins = 0, mis_del = 0, nbad = 0, nmin = 0, kmax = 0;
    if (i < n) {
        const uint64_t at = bam_rec_start(dst_off, tile_base, i);
        if (at < n_raw) {
            const PuRec r = pu_record(sorted + at, n_raw - at, ix, f);
            if (r.state == PU_RANGE) nbad = ~(uint64_t)i;
            else if (r.state == PU_LEFT_OUT) recs = 1ull << 32;
            else if (r.state == PU_COUNTED) {
                PuNoSink none;
                const PuTally t = pu_walk(sorted + at, r, ix, none);
                mine = t.events; recs = 1; aligned = t.aligned; blk_ins = (uint64_t)t.blocks | (uint64_t)t.ins << 32; mis_del = (uint64_t)t.mism | (uint64_t)t.del << 32;
                if (mine) { nmin = ~pu_key_lo(r); kmax = pu_key_hi(r); }
            }
        }
    }
    uint64_t all;
    const uint64_t ex = d_wg_exclusive(mine, all, s_wave);
    if (i < n) ev_off[i] = ex;
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
    const unsigned long long v[5] = {recs, aligned, blk_ins, mis_del, nbad};
    cv_block_partials(v, 4, s_part, part);
    const unsigned long long v2[2] = {nmin, kmax};
    cv_block_partials(v2, 0, s_part2, part2);
}

// ev_base: k_pu_count's sums, scanned; n_ev: their total as the host read it
__global__ void __launch_bounds__(PU_WG)
k_pu_emit(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, const DIndex ix,
          const PuFilter f, const uint64_t *__restrict__ ev_off, const uint64_t *__restrict__ ev_base, unsigned long long n_ev, uint64_t *__restrict__ keys, int64_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * PU_WG + threadIdx.x;
    if (i >= n) return;
    const uint64_t at = bam_rec_start(dst_off, tile_base, i);
    if (at >= n_raw) return;
    const PuRec r = pu_record(sorted + at, n_raw - at, ix, f);
    if (r.state != PU_COUNTED) return;
    PuEmit e{keys, vals, ev_base[blockIdx.x] + ev_off[i], n_ev, (uint32_t)r.refid, r.s};
    (void)pu_walk(sorted + at, r, ix, e);
}

__global__ void __launch_bounds__(PU_WG)
k_pu_scan(const uint64_t *__restrict__ keys, const int64_t *__restrict__ vals, uint32_t n_ev, uint64_t *__restrict__ incl_d, uint64_t *__restrict__ incl_a, uint64_t *__restrict__ tile_d,
          uint64_t *__restrict__ tile_a)
{
    __shared__ uint64_t s_wave[PU_WG / 64];
    const uint32_t i = blockIdx.x * PU_WG + threadIdx.x;
    uint64_t d = 0, a = 0;
    if (i < n_ev) { const uint64_t k = keys[i]; const int64_t v = vals[i]; d = pu_plane_depth(k, v); a = pu_plane_allele(k, v); }
    uint64_t all_d, all_a;
    const uint64_t ex_d = d_wg_exclusive(d, all_d, s_wave);
    const uint64_t ex_a = d_wg_exclusive(a, all_a, s_wave);
    if (i < n_ev) { incl_d[i] = ex_d + d; incl_a[i] = ex_a + a; }
    if (threadIdx.x == 0) { tile_d[blockIdx.x] = all_d; tile_a[blockIdx.x] = all_a; }
}

// event i's index + 1 when it is a tail, else CV_NONE
__device__ __forceinline__ uint64_t pu_tail_own(const uint64_t *keys, uint32_t i, uint32_t n_ev)
{
    if (i >= n_ev || !cv_is_tail(keys[i], i + 1u < n_ev ? keys[i + 1u] : 0ull, i + 1u == n_ev)) return CV_NONE;
    return (uint64_t)i + 1ull;
}

__global__ void __launch_bounds__(PU_WG)
k_pu_tails(const uint64_t *__restrict__ keys, uint32_t n_ev, uint64_t *__restrict__ tile_last)
{
    __shared__ uint64_t s_last[PU_WG / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t v = cv_wave_fill(pu_tail_own(keys, blockIdx.x * PU_WG + threadIdx.x, n_ev), lane);
    if (lane == 63u) s_last[wv] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t all = CV_NONE;
        for (uint32_t k = 0; k < PU_WG / 64; k++) all = cv_fill(all, s_last[k]);
        tile_last[blockIdx.x] = all;
    }
}

// tile_prev: k_cv_tails_top's (the last tail in front of the workgroup, index + 1; 0: none)
__global__ void __launch_bounds__(PU_WG)
k_pu_flag(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ tile_prev, uint32_t n_ev, uint32_t *__restrict__ prev_tail, uint32_t *__restrict__ mark, uint64_t *__restrict__ tile_cnt)
{
    __shared__ uint64_t s_last[PU_WG / 64];
    __shared__ uint32_t s_wave[PU_WG / 64];
    const uint32_t i = blockIdx.x * PU_WG + threadIdx.x, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t own = pu_tail_own(keys, i, n_ev);
    const uint64_t w = cv_wave_fill(own, lane);
    uint64_t left = __shfl_up(w, 1, 64);
    if (lane == 0u) left = CV_NONE;
    if (lane == 63u) s_last[wv] = w;
    __syncthreads();
    uint64_t before = (uint64_t)tile_prev[blockIdx.x];
    for (uint32_t k = 0; k < wv; k++) before = cv_fill(before, s_last[k]);
    const uint32_t prev = (uint32_t)cv_fill(before, left);                  // the tail in front of this event, index + 1
    const bool tail = own != CV_NONE;
    bool ak = false, site = false;
    if (tail) {
        const uint64_t key = keys[i];
        ak = pu_is_allele_key(true, key);
        site = pu_opens_site(ak, key, prev != 0u && prev <= n_ev, prev != 0u && prev <= n_ev ? keys[prev - 1u] : 0ull);
    }
    uint32_t all;
    const uint32_t ex = d_wg_exclusive((ak ? 1u : 0u) | (site ? 1u << 16 : 0u), all, s_wave);
    if (i < n_ev) { mark[i] = pu_mark(ex, ak, site); prev_tail[i] = prev; }
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (uint64_t)(all >> 16) << 32 | (uint64_t)(all & 0xffffu);
}

// cnt_base: k_pu_flag's counts, scanned (sites << 32 | keys); base_d, base_a: k_pu_scan's sums, scanned
__global__ void __launch_bounds__(PU_WG)
k_pu_compact(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ incl_d, const uint64_t *__restrict__ incl_a, const uint64_t *__restrict__ base_d, const uint64_t *__restrict__ base_a,
             const uint32_t *__restrict__ prev_tail, const uint32_t *__restrict__ mark, const uint64_t *__restrict__ cnt_base, uint32_t n_ev, uint32_t n_keys, uint32_t n_sites,
             uint64_t *__restrict__ ak_key, uint64_t *__restrict__ ak_n, uint64_t *__restrict__ ak_depth, uint32_t *__restrict__ site_key)
{
    const uint32_t i = blockIdx.x * PU_WG + threadIdx.x;
    if (i >= n_ev) return;
    const uint32_t m = mark[i];
    if (!(m >> 30 & 1u)) return;
    const uint64_t base = cnt_base[blockIdx.x];
    const uint32_t j = (uint32_t)base + pu_mark_keys(m), t = (uint32_t)(base >> 32) + pu_mark_sites(m);
    if (j >= n_keys) return;
    const uint32_t prev = prev_tail[i];
    const uint64_t upto = base_a[blockIdx.x] + incl_a[i], before = prev != 0u && prev <= n_ev ? base_a[(prev - 1u) / PU_WG] + incl_a[prev - 1u] : 0ull;
    ak_key[j] = keys[i]; ak_n[j] = upto - before; ak_depth[j] = base_d[blockIdx.x] + incl_d[i];
    if ((m >> 31) && t < n_sites) site_key[t] = j;
}

// name_off == nullptr: entries only
__global__ void __launch_bounds__(PU_WG)
k_pu_sites(const uint64_t *__restrict__ ak_key, const uint64_t *__restrict__ ak_n, const uint64_t *__restrict__ ak_depth, const uint32_t *__restrict__ site_key, uint32_t n_keys, uint32_t n_sites,
           const DIndex ix, uint32_t min_alt, const uint32_t *__restrict__ name_off, uint32_t *__restrict__ site_mark, uint32_t *__restrict__ line_off, uint64_t *__restrict__ kept_tile,
           uint64_t *__restrict__ line_tile, uint64_t *__restrict__ part /* 1 plane: the largest depth at a kept site */)
{
    __shared__ uint64_t s_wave[PU_WG / 64];
    __shared__ unsigned long long s_part[PU_WG / 64];
    const uint32_t t = blockIdx.x * PU_WG + threadIdx.x;
    uint64_t kept = 0, bytes = 0, deepest = 0;
    if (t < n_sites) {
        const uint32_t j = site_key[t];
        if (j < n_keys) {
            const PuSite s = pu_site(ak_key, ak_n, ak_depth, j, n_keys, ix, min_alt);
            if (s.kept && s.e.chr < (uint32_t)ix.n_chr) { kept = 1; deepest = s.e.depth; if (name_off) bytes = pu_line_len(name_off, s.e); }
        }
    }
    uint64_t all_k, all_b;
    const uint64_t ex_k = d_wg_exclusive(kept, all_k, s_wave);
    const uint64_t ex_b = d_wg_exclusive(bytes, all_b, s_wave);
    if (t < n_sites) { site_mark[t] = pu_site_mark((uint32_t)ex_k, kept != 0); line_off[t] = (uint32_t)ex_b; }
    if (threadIdx.x == 0) { kept_tile[blockIdx.x] = all_k; line_tile[blockIdx.x] = all_b; }
    const unsigned long long v[1] = {deepest};
    cv_block_partials(v, 0, s_part, part);
}

// kept_base, line_base: k_pu_sites' sums, scanned; names == nullptr: entries only
__global__ void __launch_bounds__(PU_WG)
k_pu_write(const uint64_t *__restrict__ ak_key, const uint64_t *__restrict__ ak_n, const uint64_t *__restrict__ ak_depth, const uint32_t *__restrict__ site_key, uint32_t n_keys, uint32_t n_sites,
           const DIndex ix, uint32_t min_alt, const uint32_t *__restrict__ name_off, const char *__restrict__ names, const uint32_t *__restrict__ site_mark, const uint32_t *__restrict__ line_off,
           const uint64_t *__restrict__ kept_base, const uint64_t *__restrict__ line_base, unsigned long long n_kept, unsigned long long n_bytes, dg_site_entry *__restrict__ entries,
           char *__restrict__ out)
{
    const uint32_t t = blockIdx.x * PU_WG + threadIdx.x;
    if (t >= n_sites) return;
    const uint32_t m = site_mark[t], j = site_key[t];
    if (!(m >> 31) || j >= n_keys) return;
    const uint64_t at = kept_base[blockIdx.x] + (m & 0x1ffu);
    if (at >= n_kept) return;
    const PuSite s = pu_site(ak_key, ak_n, ak_depth, j, n_keys, ix, min_alt);
    entries[at] = s.e;
    if (names && s.e.chr < (uint32_t)ix.n_chr) {
        const uint64_t b = line_base[blockIdx.x] + line_off[t];
        if (b + pu_line_len(name_off, s.e) <= n_bytes) pu_line_write(out + b, name_off, names, s.e);
    }
}
#endif
#endif
