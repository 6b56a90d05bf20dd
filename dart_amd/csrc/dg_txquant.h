// dg_txquant.h -- transcript-level expression on the device: per batch every unit's set of compatible transcripts is computed from the records in HBM (mates 2i
// and 2i + 1 are still neighbours, the position dg_batch_accumulate_genes counts at) and reduced to equivalence classes (ascending transcript list, count) in a
// class table that stays in HBM across batches; at the end of the job the tables are merged and an EM over the classes runs on the device.  No RSEM, Salmon or
// kallisto is run anywhere: the definition below is what the tests pin (tests/txquant_inputs.py is its sequential twin).
//
// Annotation.  The structs, validity rules and error texts of dg_rna_set_annotation (rm_validate, dg_rnametrics.h); cds_* and flags are validated and not used.
//   Each transcript's exons are sorted, exons that overlap or touch are merged; L_t is the sum of the merged exons.  tx_flatten (host, once) keeps per
//   transcript the merged exons with their prefix lengths, and per chromosome a segment table: ascending breakpoints, per segment the ascending ids of the
//   transcripts that have a merged exon over it (CSR), neighbouring segments with equal lists merged, the segment behind the last exon empty.  The tables are
//   kept with the index, shared by its clones, independent of the gene-count and RNA-metrics annotations, and carry a generation number.
// A read's alignment, strand s and blocks: dg_genecount.h's (gc_alignment, gc_strand, the block walk with its out-of-range behaviour).
// A read's pieces.  Blocks with L > 0 are joined into one piece across I and D ops (a D's bases belong to the piece: the piece runs from its first block's
//   start to its last block's end); an N op (op 3) of any length ends a piece, the next block begins a new one; every other op changes nothing.  A read
//   without blocks has no pieces.
// Read r is compatible with transcript t when: it has at least one piece and t is on the read's chromosome; every piece lies wholly inside one merged exon of
//   t; for consecutive pieces j, j + 1 piece j ends exactly at the end of merged exon e and piece j + 1 starts exactly at the start of merged exon e + 1;
//   strand_mode 1 (forward): t's strand == s; strand_mode 2 (reverse): t's strand != s; strand_mode 0 ignores the strand.
// A unit (units as in dg_genecount.h), decided in this order: 1. no read aligned: N_unmapped; 2. an aligned read has mapq < min_mapq: N_multimapping; 3. the
//   unit's set is the intersection of its aligned reads' compatible sets, each read under its own s; empty: N_incompatible; 4. otherwise counted: + 1 for the
//   class whose list is the set in ascending id order.
// Fragment length, for a counted unit with two aligned reads, on t0 = the set's smallest id: toff(g) = prefix length of the merged exon that holds g + g - that
//   exon's start; fl = toff(largest block end - 1) + 1 - toff(smallest block start) over both reads; FL_SUM += fl, FL_N += 1.
// Class table (CSR): uint64 off[n_classes + 1], uint32 ids[], uint64 count[], and eight words: units, unmapped, multimapping, incompatible, counted, FL_SUM,
//   FL_N, 0 (units = the sum of the next four).  As a multiset of (list, count) it is a function of the multiset of units: not of their order, the batch
//   split, the grid, the contexts or the merges.  The order of the classes is not defined.
// Effective length.  mean = floor(FL_SUM / FL_N) when FL_N > 0, else the parameter frag_mean; eff_t = L_t - mean + 1 when L_t >= mean, else L_t.
// EM (dg_tx_finish).  F = 2^20; N = the sum of the counts, N >= 2^33 is DG_ERR_RANGE; t is active when a class lists it, M = the active transcripts.  M = 0:
//   every S_t = 0, 0 rounds, converged.  Start: S_t = floor(N F / M) for active t, else 0.  One round, every floating-point operation one IEEE double
//   operation, no contraction: alpha_t = (double)S_t / F (exact); theta_t = alpha_t / (double)eff_t; per class D = the members' theta added one after the
//   other in ascending id order from 0.0; D == 0.0: the class gives nothing; else per member q = theta_t / D, x = (double)n_c q,
//   add = (uint64)floor(x 1048576.0), S'_t += add (integer).  conv_r: every t with S'_t >= F has 100 |S'_t - S_t| <= S'_t.  The EM stops after round r when
//   r == max_rounds, or when r is a multiple of 16 and conv_r holds; max_rounds 0 gives the start values.  `converged` is conv_r of the last round (1 for
//   M = 0, 0 when M > 0 and no round ran).
//   Result words: S[n_tx], then 16: units, unmapped, multimapping, incompatible, counted, classes, members, active, rounds, converged, FL_SUM, FL_N, the mean
//   used, strand_mode, 0, 0.
// Text (tx_format, host, integers only): "# name\tvalue" per summary word, "transcript_id\tlength\teff_length\test_counts\ttpm", one line per transcript:
//   est_counts = floor(S_t 1000 / F) as %llu.%03llu; rate_t = floor(S_t 1024 / eff_t), R = their sum; tpm in thousandths floor(rate_t 10^9 / R), 0 for R = 0.
//
// Everything without atomics is __host__ __device__ and shared with the CPU suite (tests/native/txquant_checks.hip).
//   k_tx_count   lane = unit: the candidates are the list of the segment under the first aligned read's first block (ascending already); each is verified
//                against every piece of the aligned reads by a binary search in its merged exons.  No per-lane set storage: the pass leaves the set's size
//                and a 64-bit hash of the list; the outcome rows and FL_SUM / FL_N go through ballots and one 8-word line per workgroup, no atomics
//   k_tx_top     one workgroup: the lines folded into the batch's eight words, the workgroups' size and item sums scanned
//   k_tx_write   lane = unit: the same walk again, the ids stored into the batch's pool; one item (offset, hash) per counted unit
//   class building (tx_build in dg_api.hip; a batch's pool, a merge and an add all fold items (list, count) into the table this way):
//   k_tx_hash    lane = item: its list's hash; rs_sort_passes sorts (hash, item)
//   k_tx_heads   lane = sorted place: the item's list against its predecessor's, in full: heads are marked; equal hash with unequal lists is reported, and
//                that build is finished exactly on the host (two lists under one hash may interleave and split a class into several runs)
//   k_tx_csr     lane = sorted place: heads write offset and ids, the counts of a run are summed per wave and added by 64-bit integer atomics
//   EM: k_tx_active (lane = member), k_tx_em_prep (one workgroup: M and N), k_tx_start / k_tx_theta (lane = transcript), k_tx_em (lane = class: D and the
//   shares, 64-bit integer atomicAdd into S'; a list above TX_LONG_LIST by the class's whole wave: loads and shares side by side, D added in the same order),
//   k_tx_conv (one workgroup: the workgroups' convergence words, every 16th round)
// No lane reads outside the arrays it was given: report and CIGAR ranges that leave them count as "not aligned" / "no blocks".
#ifndef DG_TXQUANT_H
#define DG_TXQUANT_H
#include "dg_genecount.h"
#include "dg_rnametrics.h"
#include "dg_wgscan.h"
#include <math.h>
#include <stdio.h>
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>

#define TX_HD __host__ __device__ __forceinline__
#define TX_THREADS 256           // units per workgroup of k_tx_count / k_tx_write (dg_tx_granules [0])
#define TX_WAVE 64               // (dg_tx_granules [1])
#define TX_F 1048576ull          // 2^20: the fixed point of S
#define TX_MAX_N (1ull << 33)
#define TX_CHECK_EVERY 16        // rounds between two looks at the convergence flag
#define TX_LONG_LIST 32          // k_tx_em: a class with a longer list is worked by its whole wave
enum { TX_UNMAPPED = 0, TX_MULTI, TX_INCOMPAT, TX_COUNTED };
enum { TXW_UNITS = 0, TXW_UNMAPPED, TXW_MULTI, TXW_INCOMPAT, TXW_COUNTED, TXW_FL_SUM, TXW_FL_N, TXW_WORDS = 8 };

struct TxTx { int32_t chr; uint32_t strand, n_ex, len; uint64_t first_ex; };      // 24 bytes
struct TxExon { uint32_t start, end, before; };                                   // merged, ascending; before = the transcript's bases in front of it
// segment i of chromosome c (chr_first[c] <= i < chr_first[c + 1]) begins at seg_start[i] and ends where the next begins; its transcripts are
// seg_ids[seg_off[i] .. seg_off[i + 1]), ascending
struct TxTable { const uint32_t *chr_first, *seg_start; const uint64_t *seg_off; const uint32_t *seg_ids; const TxTx *tx; const TxExon *ex; int n_chr; uint32_t n_tx; };

// ---- a read ----
struct TxRead { bool aligned, blocks; int chr, strand; unsigned long long p0; uint32_t cig_off, n_cig; };
TX_HD TxRead tx_read(const GcBatch &b, int n_chr, long long at)
{
    TxRead r{false, false, -1, 0, 0ull, 0u, 0u};
    if (at < 0) return r;
    const dg_report_out p = b.po[at];
    r.aligned = true; r.chr = p.chr; r.strand = gc_strand(p.flag);
    if (p.pos < 1 || p.chr < 0 || p.chr >= n_chr) return r;
    if ((unsigned long long)p.cigar_off + (unsigned long long)p.n_cigar > b.n_ops) return r;
    r.blocks = true; r.p0 = (unsigned long long)p.pos - 1ull; r.cig_off = p.cigar_off; r.n_cig = p.n_cigar;
    return r;
}
// the span of the read's blocks: false when it has none
TX_HD bool tx_read_span(const GcBatch &b, const TxRead &r, unsigned long long &first, unsigned long long &lo, unsigned long long &hi)
{
    if (!r.blocks) return false;
    bool any = false;
    unsigned long long q = r.p0;
    for (uint32_t k = 0; k < r.n_cig; k++) {
        const uint32_t w = b.cig[(size_t)r.cig_off + k], op = w & 15u, len = w >> 4;
        if (op == 0u || op == 7u || op == 8u) {
            if (len) { if (!any) { first = q; any = true; lo = q; hi = q + len; } if (q < lo) lo = q; if (q + len > hi) hi = q + len; }
            q += len;
        } else if (op == 2u || op == 3u) q += len;
    }
    return any;
}
// the merged exon of x that holds g
TX_HD bool tx_find_exon(const TxExon *ex, uint32_t n_ex, unsigned long long g, uint32_t &e)
{
    uint32_t l = 0, h = n_ex;                         // the first exon that begins behind g
    while (l < h) { const uint32_t m = l + (h - l) / 2; if ((unsigned long long)ex[m].start <= g) l = m + 1; else h = m; }
    if (!l) return false;
    e = l - 1;
    return g < (unsigned long long)ex[e].end;
}
// one piece [ps, pe) against the exons; prev_e / prev_pe: the piece in front of it
TX_HD bool tx_piece_ok(const TxExon *ex, uint32_t n_ex, unsigned long long ps, unsigned long long pe, bool have_prev, uint32_t &prev_e, unsigned long long prev_pe)
{
    uint32_t e;
    if (!tx_find_exon(ex, n_ex, ps, e) || pe > (unsigned long long)ex[e].end) return false;
    if (have_prev && !(prev_pe == (unsigned long long)ex[prev_e].end && e == prev_e + 1u && ps == (unsigned long long)ex[e].start)) return false;
    prev_e = e;
    return true;
}
TX_HD bool tx_compatible(const GcBatch &b, const TxTable &T, const TxRead &r, uint32_t t, uint32_t strand_mode)
{
    const TxTx x = T.tx[t];
    if (!r.blocks || x.chr != r.chr) return false;
    if (strand_mode == 1u && (int)x.strand != r.strand) return false;
    if (strand_mode == 2u && (int)x.strand == r.strand) return false;
    const TxExon *ex = T.ex + x.first_ex;
    unsigned long long q = r.p0, ps = 0, pe = 0, prev_pe = 0;
    uint32_t prev_e = 0;
    bool open = false, have_prev = false;
    for (uint32_t k = 0; k < r.n_cig; k++) {
        const uint32_t w = b.cig[(size_t)r.cig_off + k], op = w & 15u, len = w >> 4;
        if (op == 0u || op == 7u || op == 8u) {
            if (len) { if (!open) { ps = q; open = true; } pe = q + len; }
            q += len;
        } else if (op == 2u) q += len;
        else if (op == 3u) {
            q += len;
            if (open) { if (!tx_piece_ok(ex, x.n_ex, ps, pe, have_prev, prev_e, prev_pe)) return false; have_prev = true; prev_pe = pe; open = false; }
        }
    }
    if (open) { if (!tx_piece_ok(ex, x.n_ex, ps, pe, have_prev, prev_e, prev_pe)) return false; have_prev = true; }
    return have_prev;
}
TX_HD unsigned long long tx_toff(const TxTable &T, uint32_t t, unsigned long long g)
{
    const TxTx x = T.tx[t];
    const TxExon *ex = T.ex + x.first_ex;
    uint32_t e;
    if (!tx_find_exon(ex, x.n_ex, g, e)) return 0ull;
    return (unsigned long long)ex[e].before + (g - (unsigned long long)ex[e].start);
}

// ---- the hash of a list ----
TX_HD uint64_t tx_hash_step(uint64_t h, uint32_t id) { h = (h ^ (uint64_t)id) * 0x9E3779B97F4A7C15ull; return h ^ (h >> 29); }
TX_HD uint64_t tx_hash_end(uint64_t h, uint64_t n) { h ^= n; h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; return h ^ (h >> 33); }
TX_HD uint64_t tx_hash_mask(int bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1ull; }

// ---- a unit ----
struct TxUnit { uint32_t outcome, size, has_fl; uint64_t hash; unsigned long long fl; };
// out (may be null): where the set's ids go, at most cap of them
TX_HD TxUnit tx_unit(const GcBatch &b, const TxTable &T, unsigned long long u, uint32_t strand_mode, uint32_t *out, uint32_t cap)
{
    TxUnit r{TX_UNMAPPED, 0u, 0u, 0ull, 0ull};
    int n;
    const int k0 = gc_unit_first(b.n_pair_mode, u, n);
    const long long at0 = gc_alignment(b, k0), at1 = n == 2 ? gc_alignment(b, k0 + 1) : -1;
    if (at0 < 0 && at1 < 0) return r;
    if ((at0 >= 0 && (long long)b.ro[k0].mapq < (long long)b.min_mapq) || (at1 >= 0 && (long long)b.ro[k0 + 1].mapq < (long long)b.min_mapq)) { r.outcome = TX_MULTI; return r; }
    r.outcome = TX_INCOMPAT;
    const TxRead r0 = tx_read(b, T.n_chr, at0), r1 = tx_read(b, T.n_chr, at1);
    unsigned long long f0 = 0, lo0 = 0, hi0 = 0, f1 = 0, lo1 = 0, hi1 = 0;
    const bool s0 = tx_read_span(b, r0, f0, lo0, hi0), s1 = tx_read_span(b, r1, f1, lo1, hi1);
    if ((r0.aligned && !s0) || (r1.aligned && !s1)) return r;                   // an aligned read without pieces is compatible with nothing
    const int chr = r0.aligned ? r0.chr : r1.chr;
    const unsigned long long g = r0.aligned ? f0 : f1;
    const uint32_t lo = T.chr_first[chr], hi = T.chr_first[chr + 1];
    uint32_t l = lo, h = hi;                          // the first segment that begins behind g
    while (l < h) { const uint32_t m = l + (h - l) / 2; if ((unsigned long long)T.seg_start[m] <= g) l = m + 1; else h = m; }
    if (l == lo) return r;
    uint64_t hs = 0; uint32_t cnt = 0, t0 = 0;
    for (uint64_t k = T.seg_off[l - 1]; k < T.seg_off[l]; k++) {
        const uint32_t t = T.seg_ids[k];
        if (r0.aligned && !tx_compatible(b, T, r0, t, strand_mode)) continue;
        if (r1.aligned && !tx_compatible(b, T, r1, t, strand_mode)) continue;
        if (out && cnt < cap) out[cnt] = t;
        if (!cnt) t0 = t;
        hs = tx_hash_step(hs, t); cnt++;
    }
    if (!cnt) return r;
    r.outcome = TX_COUNTED; r.size = cnt; r.hash = tx_hash_end(hs, cnt);
    if (r0.aligned && r1.aligned) {
        const unsigned long long a = lo0 < lo1 ? lo0 : lo1, z = hi0 > hi1 ? hi0 : hi1;
        r.has_fl = 1u; r.fl = tx_toff(T, t0, z - 1ull) + 1ull - tx_toff(T, t0, a);
    }
    return r;
}

// ---- items (list, count): the classes of a table, or the counted units of a batch's pool (cnt == null: 1 each); two sources side by side ----
struct TxItems { const uint64_t *off; const uint32_t *ids; const uint64_t *cnt; uint64_t n; };
struct TxTwo { TxItems a, b; };
TX_HD const uint32_t *tx_item(const TxTwo &s, uint64_t i, uint64_t &len, uint64_t &cnt)
{
    const TxItems &q = i < s.a.n ? s.a : s.b;
    const uint64_t j = i < s.a.n ? i : i - s.a.n;
    const uint64_t o = q.off[j];
    len = q.off[j + 1] - o; cnt = q.cnt ? q.cnt[j] : 1ull;
    return q.ids + o;
}
TX_HD uint64_t tx_item_hash(const TxTwo &s, uint64_t i)
{
    uint64_t len, cnt, h = 0;
    const uint32_t *p = tx_item(s, i, len, cnt);
    for (uint64_t k = 0; k < len; k++) h = tx_hash_step(h, p[k]);
    return tx_hash_end(h, len);
}
// sorted place j: 0 when its item's list equals its predecessor's, else the list's length (a head); collision: equal keys over unequal lists
TX_HD uint32_t tx_head(const TxTwo &s, const uint64_t *keys, const int64_t *vals, uint64_t j, bool &collision)
{
    uint64_t len, cnt;
    const uint32_t *p = tx_item(s, (uint64_t)vals[j], len, cnt);
    if (!j || keys[j] != keys[j - 1]) return (uint32_t)len;
    uint64_t plen, pcnt;
    const uint32_t *q = tx_item(s, (uint64_t)vals[j - 1], plen, pcnt);
    bool same = len == plen;
    for (uint64_t k = 0; same && k < len; k++) same = p[k] == q[k];
    if (!same) collision = true;
    return same ? 0u : (uint32_t)len;
}

// ---- the arithmetic of a round: one IEEE double operation per line, never contracted ----
TX_HD unsigned long long tx_eff(unsigned long long L, unsigned long long mean) { return L >= mean ? L - mean + 1ull : L; }
TX_HD double tx_theta(unsigned long long S, unsigned long long eff)
{
#pragma clang fp contract(off)
    const double alpha = (double)S / 1048576.0;
    return alpha / (double)eff;
}
TX_HD double tx_add(double D, double theta)
{
#pragma clang fp contract(off)
    return D + theta;
}
TX_HD double tx_class_D(const uint32_t *ids, uint64_t len, const double *theta)
{
    double D = 0.0;
    for (uint64_t k = 0; k < len; k++) D = tx_add(D, theta[ids[k]]);
    return D;
}
TX_HD unsigned long long tx_share(double theta, double D, unsigned long long n)
{
#pragma clang fp contract(off)
    const double q = theta / D;
    const double x = (double)n * q;
    const double y = x * 1048576.0;
    return (unsigned long long)floor(y);
}
TX_HD bool tx_moved(unsigned long long S_new, unsigned long long S_old)      // what conv_r must not see
{
    const unsigned long long d = S_new > S_old ? S_new - S_old : S_old - S_new;
    return S_new >= TX_F && 100ull * d > S_new;
}

// ---- the flattening, on the host, once per annotation ----
struct TxFlat { std::vector<uint32_t> chr_first, seg_start, seg_ids; std::vector<uint64_t> seg_off; std::vector<TxTx> tx; std::vector<TxExon> ex; };
static inline void tx_merge_exons(const dg_rna_annot *a, const dg_rna_tx &t, std::vector<dg_rna_exon> &m)
{
    m.assign(a->exons + t.first_exon, a->exons + t.first_exon + t.n_exons);
    std::sort(m.begin(), m.end(), [](const dg_rna_exon &x, const dg_rna_exon &y) { return x.start != y.start ? x.start < y.start : x.end < y.end; });
    size_t n = 0;
    for (size_t k = 1; k < m.size(); k++) { if (m[k].start <= m[n].end) { if (m[k].end > m[n].end) m[n].end = m[k].end; } else m[++n] = m[k]; }
    m.resize(n + 1);
}
// false with a text that names the first bad transcript
static inline bool tx_flatten(int n_chr, const dg_rna_annot *a, TxFlat &o, char *err, size_t err_len)
{
    o = TxFlat();
    o.chr_first.assign((size_t)(n_chr > 0 ? n_chr : 0) + 1, 0u);
    if (!rm_validate(n_chr, a, err, err_len)) return false;
    struct Ev { uint64_t key; uint32_t t; };                                    // (chromosome, position, start behind end), transcript
    std::vector<Ev> ev;
    std::vector<dg_rna_exon> m;
    for (uint32_t i = 0; i < a->n_tx; i++) {
        const dg_rna_tx &t = a->tx[i];
        tx_merge_exons(a, t, m);
        uint32_t before = 0;
        const uint64_t first = o.ex.size();
        for (const dg_rna_exon &e : m) {
            o.ex.push_back(TxExon{e.start, e.end, before}); before += e.end - e.start;
            ev.push_back(Ev{(uint64_t)(uint32_t)t.chr << 33 | (uint64_t)e.start << 1 | 1u, i}); ev.push_back(Ev{(uint64_t)(uint32_t)t.chr << 33 | (uint64_t)e.end << 1, i});
        }
        o.tx.push_back(TxTx{t.chr, t.strand, (uint32_t)m.size(), before, first});
    }
    std::sort(ev.begin(), ev.end(), [](const Ev &x, const Ev &y) { return x.key < y.key; });
    std::set<uint32_t> act;
    size_t k = 0;
    o.seg_off.push_back(0);
    for (int c = 0; c < n_chr; c++) {
        o.chr_first[(size_t)c] = (uint32_t)o.seg_start.size();
        bool first = true;
        while (k < ev.size() && (int)(ev[k].key >> 33) == c) {
            const uint64_t pos = ev[k].key >> 1;
            for (; k < ev.size() && ev[k].key >> 1 == pos; k++) { if (ev[k].key & 1u) act.insert(ev[k].t); else act.erase(ev[k].t); }
            const size_t prev_at = first ? 0 : (size_t)o.seg_off[o.seg_off.size() - 2], prev_n = first ? 0 : o.seg_ids.size() - prev_at;
            if (!first && prev_n == act.size() && std::equal(act.begin(), act.end(), o.seg_ids.begin() + (ptrdiff_t)prev_at)) continue;
            if (o.seg_start.size() >= 0xFFFFFFF0ull) { snprintf(err, err_len, "the annotation gives more segments than the table holds"); return false; }
            o.seg_start.push_back((uint32_t)(pos & 0xFFFFFFFFull)); o.seg_ids.insert(o.seg_ids.end(), act.begin(), act.end()); o.seg_off.push_back(o.seg_ids.size());
            first = false;
        }
    }
    o.chr_first[(size_t)n_chr] = (uint32_t)o.seg_start.size();
    return true;
}

// ---- a class table on the host: the exact class building (what a build with colliding hashes falls back to; the CPU suite's table) ----
struct TxHostTab { std::vector<uint64_t> off, cnt; std::vector<uint32_t> ids; };
static inline void tx_build_host(const TxTwo &s, TxHostTab &o)
{
    std::map<std::vector<uint32_t>, uint64_t> cls;
    for (uint64_t i = 0; i < s.a.n + s.b.n; i++) {
        uint64_t len, cnt;
        const uint32_t *p = tx_item(s, i, len, cnt);
        cls[std::vector<uint32_t>(p, p + len)] += cnt;
    }
    o.off.assign(1, 0ull); o.cnt.clear(); o.ids.clear();
    for (const auto &kv : cls) { o.ids.insert(o.ids.end(), kv.first.begin(), kv.first.end()); o.off.push_back(o.ids.size()); o.cnt.push_back(kv.second); }
}
// what dg_tx_add checks: null, or what is wrong with the table
static inline const char *tx_bad_table(const uint64_t *off, const uint32_t *ids, const uint64_t *cnt, size_t n_classes, uint32_t n_tx, size_t &where)
{
    where = 0;
    if (!n_classes) return nullptr;
    if (!off || !ids || !cnt) return "a table with classes needs its three arrays";
    if (off[0] != 0ull) return "off[0] is not 0";
    unsigned long long total = 0;
    for (size_t i = 0; i < n_classes; i++) {
        where = i;
        if (off[i + 1] <= off[i]) return "a class's list is empty or its offsets decrease";
        for (uint64_t k = off[i]; k < off[i + 1]; k++) {
            if (ids[k] >= n_tx) return "a transcript id is outside the annotation";
            if (k > off[i] && ids[k] <= ids[k - 1]) return "a class's list is not ascending";
        }
        if (total + cnt[i] < total) return "the counts do not fit 64 bits";
        total += cnt[i];
    }
    return nullptr;
}

// ---- the text, on the host: integers and 128-bit products only ----
static const char *const TX_WORD_NAMES[16] = {"units", "unmapped", "multimapping", "incompatible", "counted", "classes", "members", "active", "rounds", "converged",
                                              "fl_sum", "fl_n", "frag_mean", "strand_mode", "reserved0", "reserved1"};
// words: S[n_tx] and the 16 summary words; len: L_t per transcript
static inline std::string tx_format(const uint64_t *words, uint32_t n_tx, const uint32_t *len, const char *const *names)
{
    std::string o;
    char line[640];
    const uint64_t *w = words + n_tx;
    for (int i = 0; i < 16; i++) { snprintf(line, sizeof line, "# %s\t%llu\n", TX_WORD_NAMES[i], (unsigned long long)w[i]); o += line; }
    o += "transcript_id\tlength\teff_length\test_counts\ttpm\n";
    std::vector<unsigned __int128> rate(n_tx);
    unsigned __int128 R = 0;
    for (uint32_t t = 0; t < n_tx; t++) { const unsigned long long eff = tx_eff(len[t], w[12]); rate[t] = eff ? (unsigned __int128)words[t] * 1024u / eff : 0; R += rate[t]; }
    for (uint32_t t = 0; t < n_tx; t++) {
        const unsigned long long est = (unsigned long long)((unsigned __int128)words[t] * 1000u / TX_F);
        const unsigned long long tpm = R ? (unsigned long long)(rate[t] * 1000000000ull / R) : 0ull;
        snprintf(line, sizeof line, "%.500s\t%u\t%llu\t%llu.%03llu\t%llu.%03llu\n", names[t], len[t], tx_eff(len[t], w[12]), est / 1000ull, est % 1000ull, tpm / 1000ull, tpm % 1000ull);
        o += line;
    }
    return o;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TX_THREADS)
k_tx_count(const GcBatch b, const TxTable T, unsigned long long n_units, uint32_t strand_mode, uint64_t hash_mask, uint32_t *__restrict__ size, uint64_t *__restrict__ hash,
           unsigned long long *__restrict__ wg_line, unsigned long long *__restrict__ tile_sz, unsigned long long *__restrict__ tile_items)
{
    __shared__ unsigned long long s_line[TX_THREADS / TX_WAVE][8];
    const unsigned long long u = (unsigned long long)blockIdx.x * TX_THREADS + threadIdx.x;
    const int lane = (int)(threadIdx.x & (TX_WAVE - 1)), wave = (int)(threadIdx.x / TX_WAVE);
    const bool valid = u < n_units;
    TxUnit r{TX_UNMAPPED, 0u, 0u, 0ull, 0ull};
    if (valid) { r = tx_unit(b, T, u, strand_mode, nullptr, 0u); size[u] = r.size; hash[u] = r.hash & hash_mask; }
    const unsigned long long n0 = (unsigned long long)__popcll(__ballot(valid && r.outcome == TX_UNMAPPED)), n1 = (unsigned long long)__popcll(__ballot(valid && r.outcome == TX_MULTI));
    const unsigned long long n2 = (unsigned long long)__popcll(__ballot(valid && r.outcome == TX_INCOMPAT)), n3 = (unsigned long long)__popcll(__ballot(valid && r.outcome == TX_COUNTED));
    const unsigned long long nf = (unsigned long long)__popcll(__ballot(valid && r.has_fl));
    const unsigned long long fl = d_wave_sum<unsigned long long>(valid && r.has_fl ? r.fl : 0ull), sz = d_wave_sum<unsigned long long>(valid ? (unsigned long long)r.size : 0ull);
    if (lane == 0) {
        unsigned long long *l = s_line[wave];
        l[0] = n0 + n1 + n2 + n3; l[1] = n0; l[2] = n1; l[3] = n2; l[4] = n3; l[5] = fl; l[6] = nf; l[7] = sz;
    }
    __syncthreads();
    if (threadIdx.x < 8u) {
        unsigned long long v = 0;
        for (int w = 0; w < TX_THREADS / TX_WAVE; w++) v += s_line[w][threadIdx.x];
        if (threadIdx.x < 7u) wg_line[(unsigned long long)blockIdx.x * 8ull + threadIdx.x] = v; else { wg_line[(unsigned long long)blockIdx.x * 8ull + 7ull] = 0ull; tile_sz[blockIdx.x] = v; }
        if (threadIdx.x == 4u) tile_items[blockIdx.x] = v;
    }
}

// one workgroup: words[0..8) = the lines of n_wg workgroups summed (248 = 31 x 8 lanes keep their word of the line); tile_sz and tile_items scanned in place,
// totals[0] = the pool's ids, totals[1] = its items
__global__ void __launch_bounds__(WG_THREADS)
k_tx_top(const unsigned long long *__restrict__ wg_line, uint32_t n_wg, unsigned long long *__restrict__ words, unsigned long long *tile_sz, unsigned long long *tile_items,
         unsigned long long *__restrict__ totals)
{
    __shared__ unsigned long long s_part[248];
    __shared__ unsigned long long s_wave[WG_THREADS / 64];
    if (threadIdx.x < 248u) {
        unsigned long long v = 0;
        for (unsigned long long i = threadIdx.x; i < (unsigned long long)n_wg * 8ull; i += 248ull) v += wg_line[i];
        s_part[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x < 8u) {
        unsigned long long sum = 0;
        for (int j = 0; j < 31; j++) sum += s_part[threadIdx.x + 8 * j];
        words[threadIdx.x] = sum;
    }
    const unsigned long long a = d_tiles_exclusive<unsigned long long>(tile_sz, n_wg, 1, s_wave);
    const unsigned long long c = d_tiles_exclusive<unsigned long long>(tile_items, n_wg, 1, s_wave);
    if (threadIdx.x == 0) { totals[0] = a; totals[1] = c; }
}

// item_off has n_items + 1 words, pool n_ids, keys n_items (n_items, n_ids: k_tx_top's totals)
__global__ void __launch_bounds__(TX_THREADS)
k_tx_write(const GcBatch b, const TxTable T, unsigned long long n_units, uint32_t strand_mode, const uint32_t *__restrict__ size, const uint64_t *__restrict__ hash,
           const unsigned long long *__restrict__ tile_sz, const unsigned long long *__restrict__ tile_items, unsigned long long n_items, unsigned long long n_ids,
           uint64_t *__restrict__ item_off, uint32_t *__restrict__ pool, uint64_t *__restrict__ keys)
{
    __shared__ unsigned long long s_wave[TX_THREADS / 64];
    const unsigned long long u = (unsigned long long)blockIdx.x * TX_THREADS + threadIdx.x;
    const bool valid = u < n_units;
    const unsigned long long sz = valid ? (unsigned long long)size[u] : 0ull;
    unsigned long long all;
    const unsigned long long at = tile_sz[blockIdx.x] + d_wg_exclusive<unsigned long long>(sz, all, s_wave);
    const unsigned long long item = tile_items[blockIdx.x] + d_wg_exclusive<unsigned long long>(sz ? 1ull : 0ull, all, s_wave);
    if (sz && item < n_items && at + sz <= n_ids) {
        item_off[item] = at; keys[item] = hash[u];
        (void)tx_unit(b, T, u, strand_mode, pool + at, (uint32_t)sz);
    }
    if (u == 0) item_off[n_items] = n_ids;
}

__global__ void __launch_bounds__(256)
k_tx_hash(const TxTwo s, unsigned long long n, unsigned long long first, uint64_t hash_mask, uint64_t *__restrict__ keys, int64_t *__restrict__ vals)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i >= n) return;
    vals[i] = (int64_t)i;
    if (i >= first) return;                           // (the pool's keys are k_tx_write's)
    keys[i] = tx_item_hash(s, i) & hash_mask;
}

// status[2] |= 1 where two neighbours have one key and unequal lists
__global__ void __launch_bounds__(256)
k_tx_heads(const TxTwo s, unsigned long long n, const uint64_t *__restrict__ keys, const int64_t *__restrict__ vals, uint32_t *__restrict__ head, uint32_t *__restrict__ sz, uint32_t *__restrict__ status)
{
    const unsigned long long j = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (j >= n) return;
    bool collision = false;
    const uint32_t len = tx_head(s, keys, vals, j, collision);
    head[j] = len ? 1u : 0u; sz[j] = len;
    if (collision) status[2] = 1u;
}

// head_ex / sz_ex: the exclusive sums of head and sz; cnt is zero before the launch
__global__ void __launch_bounds__(256)
k_tx_csr(const TxTwo s, unsigned long long n, const int64_t *__restrict__ vals, const uint32_t *__restrict__ sz, const uint32_t *__restrict__ head_ex, const uint32_t *__restrict__ sz_ex,
         unsigned long long n_classes, unsigned long long n_members, uint64_t *__restrict__ off, uint32_t *__restrict__ ids, unsigned long long *__restrict__ cnt)
{
    const unsigned long long j = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const bool valid = j < n;
    uint64_t len = 0, mine = 0; unsigned long long cls = 0;
    bool head = false;
    if (valid) {
        const uint32_t *p = tx_item(s, (uint64_t)vals[j], len, mine);
        head = sz[j] != 0u;
        cls = (unsigned long long)head_ex[j] + (head ? 1ull : 0ull) - 1ull;
        const unsigned long long at = sz_ex[j];
        if (head && cls < n_classes && at + len <= n_members) { off[cls] = at; for (unsigned long long k = 0; k < len; k++) ids[at + k] = p[k]; }
    }
    if (j == 0) off[n_classes] = n_members;
    // the counts of a run: places are consecutive in a wave, so a run is a stretch of lanes; its first lane adds the stretch's sum
    const unsigned long long first = __ballot(valid && (head || lane == 0));
    unsigned long long incl = valid ? (unsigned long long)mine : 0ull;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long up = __shfl_up(incl, o, 64); if (lane >= o) incl += up; }
    const unsigned long long above = lane == 63 ? 0ull : first >> (lane + 1);
    const int last = above ? lane + __ffsll((long long)above) - 1 : 63;
    const unsigned long long upto = __shfl(incl, last, 64);
    if (valid && (head || lane == 0) && cls < n_classes) atomicAdd(cnt + cls, upto - (incl - (unsigned long long)mine));
}

__global__ void __launch_bounds__(256)
k_tx_active(const uint32_t *__restrict__ ids, unsigned long long n_members, uint32_t n_tx, uint32_t *__restrict__ active)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i < n_members && ids[i] < n_tx) active[ids[i]] = 1u;
}
// one workgroup: out[0] = M, the active transcripts; out[1] = N, the sum of the counts
__global__ void __launch_bounds__(WG_THREADS)
k_tx_em_prep(const uint32_t *__restrict__ active, uint32_t n_tx, const unsigned long long *__restrict__ cnt, unsigned long long n_classes, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long s_wave[WG_THREADS / 64];
    unsigned long long m = 0, n = 0, all_m, all_n;
    for (unsigned long long i = threadIdx.x; i < n_tx; i += WG_THREADS) m += active[i];
    for (unsigned long long i = threadIdx.x; i < n_classes; i += WG_THREADS) n += cnt[i];
    (void)d_wg_exclusive<unsigned long long>(m, all_m, s_wave);
    (void)d_wg_exclusive<unsigned long long>(n, all_n, s_wave);
    if (threadIdx.x == 0) { out[0] = all_m; out[1] = all_n; }
}
__global__ void __launch_bounds__(256)
k_tx_start(const TxTx *__restrict__ tx, uint32_t n_tx, const uint32_t *__restrict__ active, unsigned long long start, unsigned long long mean, unsigned long long *__restrict__ S,
           unsigned long long *__restrict__ S2, uint32_t *__restrict__ eff, double *__restrict__ theta)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tx) return;
    const unsigned long long e = tx_eff(tx[t].len, mean), s = active[t] ? start : 0ull;
    eff[t] = (uint32_t)e; S[t] = s; S2[t] = 0ull; theta[t] = tx_theta(s, e);
}
__global__ void __launch_bounds__(256)
k_tx_em(const uint64_t *__restrict__ off, const uint32_t *__restrict__ ids, const unsigned long long *__restrict__ cnt, unsigned long long n_classes, const double *__restrict__ theta,
        unsigned long long *__restrict__ S2)
{
    const unsigned long long c = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const bool valid = c < n_classes;
    const unsigned long long o = valid ? off[c] : 0ull, len = valid ? off[c + 1] - o : 0ull, n = valid ? cnt[c] : 0ull;
    if (valid && len <= TX_LONG_LIST) {
        const uint32_t *p = ids + o;
        const double D = tx_class_D(p, len, theta);
        if (D != 0.0)
            for (uint64_t k = 0; k < len; k++) {
                const unsigned long long add = tx_share(theta[p[k]], D, n);
                if (add) atomicAdd(S2 + p[k], add);
            }
    }
    // the long lists, one after the other, by the whole wave (all 64 lanes are here: no lane has left).  64 members' theta are loaded side by side; D is still
    // added one member after the other in ascending order, by every lane alike from the shuffled values, so it is the sum of the definition; then a share per lane
    unsigned long long todo = __ballot(valid && len > TX_LONG_LIST);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const unsigned long long wo = __shfl(o, src, 64), wlen = __shfl(len, src, 64), wn = __shfl(n, src, 64);
        const uint32_t *p = ids + wo;
        double D = 0.0;
        for (unsigned long long base = 0; base < wlen; base += 64ull) {
            const unsigned long long k = base + (unsigned long long)lane;
            const double th = k < wlen ? theta[p[k]] : 0.0;
            const int m = wlen - base < 64ull ? (int)(wlen - base) : 64;
            for (int i = 0; i < m; i++) D = tx_add(D, __shfl(th, i, 64));
        }
        if (D == 0.0) continue;
        for (unsigned long long k = (unsigned long long)lane; k < wlen; k += 64ull) {
            const unsigned long long add = tx_share(theta[p[k]], D, wn);
            if (add) atomicAdd(S2 + p[k], add);
        }
    }
}
// S' becomes S, theta follows, S' is zero again; conv[workgroup] = 1 when one of its transcripts moved
__global__ void __launch_bounds__(256)
k_tx_theta(uint32_t n_tx, const uint32_t *__restrict__ eff, unsigned long long *__restrict__ S, unsigned long long *__restrict__ S2, double *__restrict__ theta, uint32_t *__restrict__ conv)
{
    __shared__ uint32_t s_any[256 / 64];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    bool moved = false;
    if (t < n_tx) {
        const unsigned long long now = S2[t];
        moved = tx_moved(now, S[t]);
        S[t] = now; S2[t] = 0ull; theta[t] = tx_theta(now, eff[t]);
    }
    const unsigned long long any = __ballot(moved);
    if ((threadIdx.x & 63u) == 0u) s_any[threadIdx.x >> 6] = any ? 1u : 0u;
    __syncthreads();
    if (threadIdx.x == 0) conv[blockIdx.x] = s_any[0] | s_any[1] | s_any[2] | s_any[3];
}
__global__ void __launch_bounds__(WG_THREADS)
k_tx_conv(const uint32_t *__restrict__ conv, uint32_t n_wg, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long s_wave[WG_THREADS / 64];
    unsigned long long m = 0, all;
    for (uint32_t i = threadIdx.x; i < n_wg; i += WG_THREADS) m += conv[i];
    (void)d_wg_exclusive<unsigned long long>(m, all, s_wave);
    if (threadIdx.x == 0) out[2] = all;
}
#endif
#endif
