// dg_rnametrics.h -- RNA-seq metrics of the coordinate-sorted BAM: which share of the aligned bases falls on coding sequence, UTR, introns, intergenic sequence and
// rRNA, whether the library is stranded and which way, and the coverage profile from the transcripts' 5' ends to their 3' ends, built in HBM next to the sort
// (dg_bamsort.h).  It is the first stage that joins an annotation to the sorted array: the flattening of dg_genecount.h (a segment table per chromosome, a binary
// search and a walk), the event path of dg_coverage.h (k_cv_count, k_cv_emit, the radix sort, k_cv_depth) and the one record reader of dg_bamrec.h.  What Picard
// CollectRnaSeqMetrics (RSeQC read_distribution.py, infer_experiment.py, geneBody_coverage.py) computes from the finished file on one core.  The reference program
// has no such output: an opt-in extension, read-only on the sorted array.
//
// THE DEFINITION.  No Picard or RSeQC exists where this project is built and tested: this text is what the tests pin (tests/rnametrics_inputs.py is its sequential twin).
//
// Annotation.  dg_rna_annot: n_tx >= 1 transcripts dg_rna_tx { chr, strand (0 +, 1 -), flags (DG_RNA_TX_RIBOSOMAL), cds_start, cds_end, n_exons, first_exon } and
//   their exons dg_rna_exon { start, end }, 0-based half-open on the chromosome.  Valid: 0 <= chr < n_chr; strand 0 or 1; no flag bit but DG_RNA_TX_RIBOSOMAL;
//   n_exons >= 1 and [first_exon, first_exon + n_exons) inside the exon array; every exon start < end (<= 2^32 - 1); cds_start <= cds_end (equal: no CDS).  Anything
//   else is DG_ERR_ARG, the text names the first bad transcript.  Exons of a transcript may come in any order, may overlap and may touch: rm_flatten (host, once)
//   sorts them and merges those that overlap or touch.  The transcript's span is [first start, last end), its length L the sum of the merged exons; it is
//   eligible when L >= 100.
//   class(p) of base p of chromosome c is the maximum over every transcript on c whose span holds p of: 4 RIBOSOMAL p in an exon of a flagged transcript; 3 CODING
//   p in an exon and cds_start <= p < cds_end; 2 UTR p in an exon otherwise (a transcript without CDS is all UTR, as Picard counts it); 1 INTRONIC p in the span
//   but in no exon of that transcript; 0 INTERGENIC when no span holds p.  strands(p) is the OR of 1 << strand over the transcripts whose span holds p.
//   The segment table: per chromosome ascending breakpoints, per segment (class, strands), neighbouring segments with equal pairs merged, the segment behind the
//   last span (0, 0); *n_segments its size, *n_eligible the number of eligible transcripts.
// Records.  A record of the sorted array is counted exactly as the coverage track counts it (cv_record of dg_coverage.h, no strand selection) under exclude_flags
//   and min_mapq; its blocks are the coverage track's (M, =, X ops with L > 0; D and N move the position).  A block end above 2^32 - 1 on a counted record:
//   DG_ERR_RANGE, the text names the record's index, no words are left behind.  s = (flag >> 4 & 1) ^ (flag >> 7 & 1).
// Words, u64 in one flat array (dg_bam_rna_offsets gives the sections' first words):
//   BA[5]    every base of every block of every counted record: + 1 at class(p); a block on a chromosome without segments, or outside them, is class 0.
//   RC[5]    per counted record + 1 at the highest class any of its blocks touches.
//   ST[4]    per counted record, b = OR of strands over every segment its blocks touch: b == 0 ST[3] (intergenic); b == 3 ST[2] (ambiguous); otherwise ST[0]
//            (sense) when s == (b == 2), else ST[1] (antisense).  A second mate already counts for the opposite strand through s.
//   BC[3][100]  the gene-body profile.  depth(c, g) = the number of (counted record, block) pairs on c with start <= g < end; it ignores strand.  For an eligible
//            transcript sample b (0 .. 99) sits at transcript offset o_b = floor((2 b + 1) L / 200), offsets running 5' to 3': over the merged exons from the left
//            for strand 0, from the right (L - 1 - o_b from the left) for strand 1; the offset mapped through the exons' prefix lengths is a genomic g, and
//            d_b = depth(chr, g).  S = the sum of d_b.  The transcript contributes when S >= max(min_cov, 1); then BC[0][b] += d_b, BC[1][b] += (d_b > 0) and
//            BC[2][b] += floor(d_b * 100000 / S): its profile in per mille of its own mean (Picard's normalization), in integers.
//   SN[16]   0 records, 1 counted, 2 blocks, 3 aligned bases (= the sum of BA), 4 transcripts, 5 eligible, 6 contributing, 7 segments, 8 .. 15 zero.
// The words are a function of the record SET and the annotation: not of order, grid, batch split, ordinals, contexts or growth history.  Every word is a sum of
// non-negative integers; the depth at a position is the sum of the deltas of every event in front of it, whatever the order inside a run of equal keys.
// Text (rm_format, on the host, integers only, 128-bit products): "SN\tname\tvalue", "BA\tclass\tbases\tppm" (ppm = bases 10^6 / aligned), "RC\tclass\trecords",
//   "ST\tname\trecords", "BC\tbin\tdepth\tcovered\tnormalized"; behind the eight SN words four derived ones, floored, 0 when the denominator is 0: sense_ppm =
//   ST[0] 10^6 / (ST[0] + ST[1]); five_prime_milli = the sum of BC[2][0 .. 9] / (10 contributing); three_prime_milli the same over bins 90 .. 99;
//   five_to_three_milli = 1000 x the sum of BC[2][0 .. 9] / the sum of BC[2][90 .. 99].
//
//   k_rm_class      lane = sorted record, the pass that touches every record: head, filter and CIGAR walk (bam_cigar_walk through cv_blocks); per block the segment
//                   that holds its start by binary search, then a walk while seg_start < block end (gc_touch's shape), the overlap with each segment added to
//                   the lane's five base counts.  Persistent grid; a lane keeps its sixteen sums in registers (every index is a constant once the loops are
//                   unrolled), the waves sum them at the end, the workgroup leaves one line (cv_block_partials).  No atomic.
//   k_rm_top        one workgroup: the lines of all workgroups summed into BA, RC, ST and SN
//   (events)        k_cv_count, k_cv_top, k_cv_emit, the radix sort, k_cv_depth and k_tiles_top of the coverage track, under this stage's filter, in buffers of
//                   its own: depth(c, g) is the scanned delta at the last event with key <= c << 32 | g, one upper-bound search (rm_upper2, rm_depth_at)
//   k_rm_body       a wave = an eligible transcript: lane l takes samples l and l + 64, their two searches step by step together (rm_upper2); offset to exon (binary search in the prefix lengths) to g to depth; the
//                   wave's sum S, the contribution test, and the three rows into the workgroup's 301 words of LDS; one line per workgroup at the end
//   k_rm_body_top   a wave = a word: the workgroups' lines summed into BC and SN.contributing
// Everything a lane decides is host-callable: rm_touch, rm_record, rm_st_row, rm_upper2, rm_depth_at, rm_sample_offset, rm_sample_pos, rm_contributes, rm_norm;
// tests/native/rnametrics_checks.hip runs them on the CPU lane by lane.  DG_RNA_MAX_GROUPS (read at dg_init) caps both grids: a test hook.
#ifndef DG_RNAMETRICS_H
#define DG_RNAMETRICS_H
#include "dg_coverage.h"
#include <stdio.h>
#include <algorithm>
#include <string>
#include <vector>

#define RM_HD __host__ __device__ __forceinline__
#define RM_THREADS 256               // records per workgroup trip of k_rm_class (dg_bam_rna_granules [0])
#define RM_TX_PER_WG (RM_THREADS / 64) // transcripts per workgroup trip of k_rm_body: a wave each (dg_bam_rna_granules [1])
#define RM_GROUPS 2048               // the largest grid
#define RM_BINS 100
#define RM_MIN_LEN 100u              // a transcript of fewer bases is not eligible
#define RM_PLANES 16                 // k_rm_class's line: BA[5], RC[5], ST[4], counted, blocks
#define RM_BODY_LINE 304             // k_rm_body's line: BC[3][100], contributing (301 words, padded)
static_assert(RM_THREADS == CV_THREADS, "k_rm_class leaves its line through cv_block_partials");
static_assert(RM_BODY_LINE % RM_TX_PER_WG == 0 && RM_BODY_LINE > 3 * RM_BINS, "k_rm_body_top: a wave per word of the line, whole workgroups");
enum { RM_INTERGENIC = 0, RM_INTRONIC, RM_UTR, RM_CODING, RM_RIBOSOMAL, RM_CLASSES };
enum { RM_SN_RECORDS = 0, RM_SN_COUNTED, RM_SN_BLOCKS, RM_SN_ALIGNED, RM_SN_TX, RM_SN_ELIGIBLE, RM_SN_CONTRIB, RM_SN_SEGMENTS };
__host__ __device__ constexpr size_t rm_off_ba() { return 0; }
__host__ __device__ constexpr size_t rm_off_rc() { return 5; }
__host__ __device__ constexpr size_t rm_off_st() { return 10; }
__host__ __device__ constexpr size_t rm_off_bc() { return 14; }
__host__ __device__ constexpr size_t rm_off_sn() { return 14 + 3 * RM_BINS; }
__host__ __device__ constexpr size_t rm_words() { return rm_off_sn() + 16; }

// the segment table: segment i of chromosome c (chr_first[c] <= i < chr_first[c + 1]) begins at seg_start[i] and ends where the next begins (the last one, (0, 0),
// never ends); seg_cs[i] = class | strands << 8
struct RmTable { const uint32_t *chr_first, *seg_start, *seg_cs; int n_chr; };
// an eligible transcript and its merged exons (ascending; before = the transcript bases to the exon's left)
struct RmTx { int32_t chr; uint32_t strand, len, n_ex; uint64_t first; };
struct RmExon { uint32_t start, end, before; };

// what a record's blocks touch
struct RmAcc { uint64_t ba[RM_CLASSES]; uint32_t top, bits; };
// the block [s, e) against the segments [lo, hi) of its chromosome: the overlap with every segment to the segment's class, the rest to class 0
RM_HD void rm_touch(const RmTable &t, uint32_t lo, uint32_t hi, uint64_t s, uint64_t e, RmAcc &a)
{
    uint64_t inside = 0;
    if (lo != hi) {
        uint32_t l = lo, h = hi;                        // the first segment that begins behind s
        while (l < h) { const uint32_t m = l + (h - l) / 2; if ((uint64_t)t.seg_start[m] <= s) l = m + 1; else h = m; }
        for (uint32_t i = l > lo ? l - 1 : lo; i < hi && (uint64_t)t.seg_start[i] < e; i++) {
            const uint64_t from = (uint64_t)t.seg_start[i] > s ? (uint64_t)t.seg_start[i] : s;
            const uint64_t to = i + 1 < hi && (uint64_t)t.seg_start[i + 1] < e ? (uint64_t)t.seg_start[i + 1] : e;
            const uint32_t cs = t.seg_cs[i], cls = cs & 7u;
#pragma unroll
            for (uint32_t k = 0; k < RM_CLASSES; k++) a.ba[k] += cls == k ? to - from : 0ull;
            if (cls > a.top) a.top = cls;
            a.bits |= cs >> 8 & 3u;
            inside += to - from;
        }
    }
    a.ba[0] += (e - s) - inside;
}
RM_HD uint32_t rm_st_row(uint32_t flag, uint32_t bits)
{
    const uint32_t s = (flag >> 4 & 1u) ^ (flag >> 7 & 1u);
    if (bits == 0u) return 3u;
    if (bits == 3u) return 2u;
    return s == (bits == 2u ? 1u : 0u) ? 0u : 1u;
}
// the record that starts (with its block_size) at rec, `avail` bytes of the array behind rec
struct RmRec { bool counted, bad; uint32_t blocks, st; RmAcc acc; };
struct RmSink {
    const RmTable &t; uint32_t lo, hi; RmAcc &a; bool &bad;
    RM_HD void operator()(uint32_t, uint64_t s, uint64_t e) { if (e > CV_MAX_POS) bad = true; rm_touch(t, lo, hi, s, e, a); }
};
RM_HD RmRec rm_record(const unsigned char *rec, uint64_t avail, const RmTable &t, const CvFilter &f)
{
    RmRec o; o.bad = false; o.blocks = 0; o.st = 3u; o.acc.top = 0; o.acc.bits = 0;
#pragma unroll
    for (int k = 0; k < RM_CLASSES; k++) o.acc.ba[k] = 0;
    const BamHead h = bam_head(rec, avail);
    const CvRec r = cv_record(h, t.n_chr, f);
    o.counted = r.counted;
    if (!r.counted) return o;
    RmSink sink{t, t.chr_first[r.refid], t.chr_first[r.refid + 1], o.acc, o.bad};
    o.blocks = cv_blocks(rec, r, sink);
    o.st = rm_st_row(h.flag, o.acc.bits);
    return o;
}
// c0, c1 = the numbers of sorted events with a key <= k0, <= k1: two upper-bound searches, one step of each per trip, so that a lane's two samples wait for
// their loads together and not one after the other (every trip is a dependent load).  Not measured apart: k_rm_body takes 0.03 ms over 4540 transcripts.
RM_HD void rm_upper2(const uint64_t *keys, uint32_t n_ev, uint64_t k0, uint64_t k1, uint32_t &c0, uint32_t &c1)
{
    c0 = 0; c1 = 0;
    if (!n_ev) return;
    uint64_t step = 1;
    while (step <= (uint64_t)n_ev / 2) step <<= 1;      // the largest power of two <= n_ev
    for (; step; step >>= 1) {
        const uint64_t a = c0 + step, b = c1 + step;
        const bool ta = a <= n_ev && keys[a - 1] <= k0, tb = b <= n_ev && keys[b - 1] <= k1;
        if (ta) c0 = (uint32_t)a;
        if (tb) c1 = (uint32_t)b;
    }
}
// the scanned delta (dep_base: k_cv_depth's sums, scanned) at the last of `count` events; 0 in front of the first
RM_HD uint32_t rm_depth_at(const uint32_t *incl, const uint32_t *dep_base, uint32_t count) { return count ? dep_base[(count - 1u) / CV_THREADS] + incl[count - 1u] : 0u; }
RM_HD uint32_t rm_sample_offset(uint32_t b, uint32_t len) { return (uint32_t)((2ull * b + 1ull) * len / 200ull); }
// the genomic position of sample b of transcript x, ex its merged exons
RM_HD uint32_t rm_sample_pos(const RmTx &x, const RmExon *ex, uint32_t b)
{
    uint32_t o = rm_sample_offset(b, x.len);
    if (x.strand) o = x.len - 1u - o;
    uint32_t l = 0, h = x.n_ex;                         // the exons that begin at or in front of transcript offset o: at least the first
    while (l < h) { const uint32_t m = l + (h - l) / 2; if (ex[m].before <= o) l = m + 1; else h = m; }
    const RmExon e = ex[l ? l - 1u : 0u];
    return e.start + (o - e.before);
}
RM_HD bool rm_contributes(uint64_t S, uint64_t min_cov) { return S >= (min_cov > 1ull ? min_cov : 1ull); }
RM_HD uint64_t rm_norm(uint32_t d, uint64_t S) { return (uint64_t)d * 100000ull / S; }      // (d < 2^32: the product stays below 2^49)

// ---- the flattening, on the host, once per annotation ----
struct RmFlat {
    std::vector<uint32_t> chr_first, seg_start, seg_cs; std::vector<RmTx> tx; std::vector<RmExon> ex;      // tx: the eligible ones
};
// the annotation's validity rules (dg_rna_set_annotation's and dg_tx_set_annotation's): false with a text that names the first bad transcript
static inline bool rm_validate(int n_chr, const dg_rna_annot *a, char *err, size_t err_len)
{
    if (n_chr < 1 || !a || a->n_tx < 1u || !a->tx || (a->n_exons && !a->exons)) { snprintf(err, err_len, "the annotation needs at least one chromosome and one transcript (%d chromosomes, %u transcripts)", n_chr, a ? a->n_tx : 0u); return false; }
    for (uint32_t i = 0; i < a->n_tx; i++) {
        const dg_rna_tx &t = a->tx[i];
        const char *what = t.chr < 0 || t.chr >= n_chr ? "its chromosome is outside the index" : t.strand > 1u ? "its strand is neither 0 nor 1"
                           : (t.flags & ~(uint32_t)DG_RNA_TX_RIBOSOMAL) ? "its flags hold a bit that is not DG_RNA_TX_RIBOSOMAL" : t.n_exons < 1u ? "it has no exon"
                           : (t.first_exon > (uint64_t)a->n_exons || (uint64_t)t.n_exons > (uint64_t)a->n_exons - t.first_exon) ? "its exons lie outside the exon array"
                           : t.cds_start > t.cds_end ? "cds_start <= cds_end does not hold" : nullptr;
        if (!what)
            for (uint32_t k = 0; k < t.n_exons && !what; k++) if (!(a->exons[t.first_exon + k].start < a->exons[t.first_exon + k].end)) what = "an exon's start < end does not hold";
        if (what) { snprintf(err, err_len, "transcript %u (chr %d, strand %u, flags 0x%x, CDS [%u, %u), %u exons from %llu): %s", i, t.chr, t.strand, t.flags, t.cds_start, t.cds_end, t.n_exons, (unsigned long long)t.first_exon, what); return false; }
    }
    return true;
}
// false with a text that names the first bad transcript
static inline bool rm_flatten(int n_chr, const dg_rna_annot *a, RmFlat &o, char *err, size_t err_len)
{
    o.chr_first.assign((size_t)(n_chr > 0 ? n_chr : 0) + 1, 0u); o.seg_start.clear(); o.seg_cs.clear(); o.tx.clear(); o.ex.clear();
    if (!rm_validate(n_chr, a, err, err_len)) return false;
    // events (chromosome, position): which 0 the span (class 1 and the strand), 2 .. 4 an exon piece of that class
    struct Ev { uint64_t key; int32_t which, delta; uint32_t strand; };
    std::vector<Ev> ev;
    std::vector<dg_rna_exon> m;
    for (uint32_t i = 0; i < a->n_tx; i++) {
        const dg_rna_tx &t = a->tx[i];
        m.assign(a->exons + t.first_exon, a->exons + t.first_exon + t.n_exons);
        std::sort(m.begin(), m.end(), [](const dg_rna_exon &x, const dg_rna_exon &y) { return x.start != y.start ? x.start < y.start : x.end < y.end; });
        size_t n = 0;
        for (size_t k = 1; k < m.size(); k++) { if (m[k].start <= m[n].end) { if (m[k].end > m[n].end) m[n].end = m[k].end; } else m[++n] = m[k]; }
        m.resize(n + 1);
        const uint64_t c = (uint64_t)(uint32_t)t.chr << 32;
        auto piece = [&](uint32_t s, uint32_t e, int32_t which) { if (s < e) { ev.push_back(Ev{c | s, which, 1, t.strand}); ev.push_back(Ev{c | e, which, -1, t.strand}); } };
        piece(m.front().start, m.back().end, 0);
        uint64_t len = 0;
        for (const dg_rna_exon &e : m) {
            len += e.end - e.start;
            if (t.flags & DG_RNA_TX_RIBOSOMAL) { piece(e.start, e.end, RM_RIBOSOMAL); continue; }
            const uint32_t cs = std::min(std::max(t.cds_start, e.start), e.end), ce = std::min(std::max(t.cds_end, e.start), e.end);      // the CDS inside the exon: [cs, ce)
            piece(e.start, cs, RM_UTR); piece(cs, ce, RM_CODING); piece(ce, e.end, RM_UTR);
        }
        if (len >= RM_MIN_LEN) {
            o.tx.push_back(RmTx{t.chr, t.strand, (uint32_t)len, (uint32_t)m.size(), (uint64_t)o.ex.size()});
            uint32_t before = 0;
            for (const dg_rna_exon &e : m) { o.ex.push_back(RmExon{e.start, e.end, before}); before += e.end - e.start; }
        }
    }
    std::sort(ev.begin(), ev.end(), [](const Ev &x, const Ev &y) { return x.key < y.key; });
    size_t k = 0;
    for (int c = 0; c < n_chr; c++) {
        o.chr_first[(size_t)c] = (uint32_t)o.seg_start.size();
        long long act[RM_CLASSES] = {0, 0, 0, 0, 0}, str[2] = {0, 0};
        uint32_t prev = 0;                              // (0, 0) in front of the first span
        while (k < ev.size() && (int)(ev[k].key >> 32) == c) {
            const uint64_t key = ev[k].key;
            for (; k < ev.size() && ev[k].key == key; k++) {
                if (ev[k].which == 0) { act[RM_INTRONIC] += ev[k].delta; str[ev[k].strand] += ev[k].delta; }
                else act[ev[k].which] += ev[k].delta;
            }
            uint32_t cls = 0;
            for (uint32_t q = 1; q < RM_CLASSES; q++) if (act[q] > 0) cls = q;
            const uint32_t now = cls | ((str[0] > 0 ? 1u : 0u) | (str[1] > 0 ? 2u : 0u)) << 8;
            if (now != prev) {
                if (o.seg_start.size() >= 0xFFFFFFF0ull) { snprintf(err, err_len, "the annotation gives more segments than the table holds"); return false; }
                o.seg_start.push_back((uint32_t)key); o.seg_cs.push_back(now); prev = now;
            }
        }
    }
    o.chr_first[(size_t)n_chr] = (uint32_t)o.seg_start.size();
    return true;
}

// ---- the text, on the host: integers only ----
static inline void rm_format(const uint64_t *w, std::string &o)
{
    static const char *const sn_names[8] = {"records", "counted", "blocks", "aligned_bases", "transcripts", "eligible_transcripts", "contributing_transcripts", "segments"};
    static const char *const cls_names[RM_CLASSES] = {"intergenic", "intronic", "utr", "coding", "ribosomal"};
    static const char *const st_names[4] = {"sense", "antisense", "ambiguous", "intergenic"};
    const uint64_t *ba = w + rm_off_ba(), *rc = w + rm_off_rc(), *st = w + rm_off_st(), *bc = w + rm_off_bc(), *sn = w + rm_off_sn();
    auto line = [&o](const char *tag, const char *name) { o += tag; o.push_back('\t'); o += name; };
    auto num = [&o](unsigned long long v) { char b[24]; int n = 0; do { b[n++] = (char)('0' + v % 10); v /= 10; } while (v); o.push_back('\t'); while (n) o.push_back(b[--n]); };
    for (int k = 0; k < 8; k++) { line("SN", sn_names[k]); num(sn[k]); o.push_back('\n'); }
    unsigned __int128 five = 0, three = 0;
    for (int b = 0; b < 10; b++) { five += bc[2 * RM_BINS + b]; three += bc[2 * RM_BINS + 90 + b]; }
    auto div = [](unsigned __int128 a, unsigned __int128 d) { return d ? (unsigned long long)(a / d) : 0ull; };
    line("SN", "sense_ppm"); num(div((unsigned __int128)st[0] * 1000000u, (unsigned __int128)st[0] + st[1])); o.push_back('\n');
    line("SN", "five_prime_milli"); num(div(five, (unsigned __int128)sn[RM_SN_CONTRIB] * 10u)); o.push_back('\n');
    line("SN", "three_prime_milli"); num(div(three, (unsigned __int128)sn[RM_SN_CONTRIB] * 10u)); o.push_back('\n');
    line("SN", "five_to_three_milli"); num(div(five * 1000u, three)); o.push_back('\n');
    for (int k = 0; k < RM_CLASSES; k++) { line("BA", cls_names[k]); num(ba[k]); num(div((unsigned __int128)ba[k] * 1000000u, sn[RM_SN_ALIGNED])); o.push_back('\n'); }
    for (int k = 0; k < RM_CLASSES; k++) { line("RC", cls_names[k]); num(rc[k]); o.push_back('\n'); }
    for (int k = 0; k < 4; k++) { line("ST", st_names[k]); num(st[k]); o.push_back('\n'); }
    for (int b = 0; b < RM_BINS; b++) { o += "BC"; num((unsigned)b); num(bc[b]); num(bc[RM_BINS + b]); num(bc[2 * RM_BINS + b]); o.push_back('\n'); }
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RM_THREADS)
k_rm_class(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, const RmTable t,
           const CvFilter f, uint64_t *__restrict__ part /* RM_PLANES planes x workgroups */)
{
    __shared__ unsigned long long s_part[RM_PLANES * (RM_THREADS / 64)];
    unsigned long long v[RM_PLANES];
#pragma unroll
    for (int p = 0; p < RM_PLANES; p++) v[p] = 0ull;
    for (uint64_t base = (uint64_t)blockIdx.x * RM_THREADS; base < n; base += (uint64_t)gridDim.x * RM_THREADS) {
        const uint64_t i = base + threadIdx.x;
        if (i >= n) continue;
        const uint64_t at = bam_rec_start(dst_off, tile_base, (uint32_t)i);
        if (at >= n_raw) continue;
        const RmRec r = rm_record(sorted + at, n_raw - at, t, f);
        if (!r.counted || r.bad) continue;              // (a record out of range ends the call: k_cv_count names it)
#pragma unroll
        for (uint32_t k = 0; k < RM_CLASSES; k++) { v[k] += r.acc.ba[k]; v[5 + k] += r.acc.top == k ? 1ull : 0ull; }
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) v[10 + k] += r.st == k ? 1ull : 0ull;
        v[14] += 1ull; v[15] += r.blocks;
    }
    cv_block_partials(v, RM_PLANES, s_part, part);
}

// one workgroup: the planes of n_wg workgroups summed into BA, RC, ST and SN; the annotation's numbers beside them
__global__ void __launch_bounds__(RM_THREADS)
k_rm_top(const uint64_t *__restrict__ part, uint32_t n_wg, unsigned long long n_records, unsigned long long n_tx, unsigned long long n_eligible, unsigned long long n_segments,
         unsigned long long *__restrict__ words)
{
    __shared__ unsigned long long s_w[RM_PLANES][RM_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (int p = 0; p < RM_PLANES; p++) {
        unsigned long long acc = 0;
        for (uint32_t g = threadIdx.x; g < n_wg; g += RM_THREADS) acc += part[(size_t)p * n_wg + g];
        acc = d_wave_sum(acc);
        if (lane == 0u) s_w[p][wv] = acc;
    }
    __syncthreads();
    if (threadIdx.x < RM_PLANES) {
        const uint32_t p = threadIdx.x;
        unsigned long long a = 0;
        for (uint32_t k = 0; k < RM_THREADS / 64; k++) a += s_w[p][k];
        if (p < 14u) words[p] = a;                      // BA, RC and ST lie side by side from word 0 on
        else words[rm_off_sn() + (p == 14u ? RM_SN_COUNTED : RM_SN_BLOCKS)] = a;
    }
    if (threadIdx.x == 64u) {
        unsigned long long aligned = 0;
        for (uint32_t p = 0; p < RM_CLASSES; p++) for (uint32_t k = 0; k < RM_THREADS / 64; k++) aligned += s_w[p][k];
        unsigned long long *sn = words + rm_off_sn();
        sn[RM_SN_RECORDS] = n_records; sn[RM_SN_ALIGNED] = aligned; sn[RM_SN_TX] = n_tx; sn[RM_SN_ELIGIBLE] = n_eligible; sn[RM_SN_SEGMENTS] = n_segments;
    }
}
static_assert(rm_off_ba() == 0 && rm_off_rc() == 5 && rm_off_st() == 10 && rm_off_bc() == 14, "k_rm_top writes planes 0 .. 13 to words 0 .. 13");

__global__ void __launch_bounds__(RM_THREADS)
k_rm_body(const RmTx *__restrict__ tx, const RmExon *__restrict__ ex, uint32_t n_eligible, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ incl,
          const uint32_t *__restrict__ dep_base, uint32_t n_ev, unsigned long long min_cov, unsigned long long *__restrict__ line /* RM_BODY_LINE planes x workgroups */)
{
    __shared__ unsigned long long s_bc[RM_BODY_LINE];
    for (uint32_t k = threadIdx.x; k < RM_BODY_LINE; k += RM_THREADS) s_bc[k] = 0ull;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (uint64_t i = (uint64_t)blockIdx.x * RM_TX_PER_WG + wv; i < n_eligible; i += (uint64_t)gridDim.x * RM_TX_PER_WG) {      // (i is the same for all lanes of a wave)
        const RmTx x = tx[i];
        const RmExon *e = ex + x.first;
        const bool two = lane + 64u < RM_BINS;          // (a lane without a second sample looks its first one up twice: the same loads)
        uint32_t c0, c1;
        rm_upper2(keys, n_ev, cv_key(x.chr, rm_sample_pos(x, e, lane)), cv_key(x.chr, rm_sample_pos(x, e, two ? lane + 64u : lane)), c0, c1);
        const uint32_t d0 = rm_depth_at(incl, dep_base, c0), d1 = two ? rm_depth_at(incl, dep_base, c1) : 0u;
        const unsigned long long S = d_wave_sum((unsigned long long)d0 + d1);
        if (!rm_contributes(S, min_cov)) continue;
        if (d0) { atomicAdd(&s_bc[lane], (unsigned long long)d0); atomicAdd(&s_bc[RM_BINS + lane], 1ull); const unsigned long long q = rm_norm(d0, S); if (q) atomicAdd(&s_bc[2 * RM_BINS + lane], q); }
        if (d1) { atomicAdd(&s_bc[lane + 64u], (unsigned long long)d1); atomicAdd(&s_bc[RM_BINS + lane + 64u], 1ull); const unsigned long long q = rm_norm(d1, S); if (q) atomicAdd(&s_bc[2 * RM_BINS + lane + 64u], q); }
        if (lane == 0u) atomicAdd(&s_bc[3 * RM_BINS], 1ull);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < RM_BODY_LINE; k += RM_THREADS) line[(size_t)k * gridDim.x + blockIdx.x] = s_bc[k];
}

// a wave = one of the 301 words: its plane of n_wg workgroups summed into BC or SN.contributing (RM_BODY_LINE / 4 workgroups).  (The first shape, one workgroup
// whose threads each walked a word through all lines one load after the other, took 0.5 ms over 1135 lines: as long as everything else of the stage together.)
__global__ void __launch_bounds__(RM_THREADS)
k_rm_body_top(const unsigned long long *__restrict__ line, uint32_t n_wg, unsigned long long *__restrict__ words)
{
    const uint32_t lane = threadIdx.x & 63u, k = blockIdx.x * RM_TX_PER_WG + (threadIdx.x >> 6);
    if (k > 3u * RM_BINS) return;                       // (a whole wave)
    unsigned long long a = 0;
    for (uint32_t g = lane; g < n_wg; g += 64u) a += line[(size_t)k * n_wg + g];
    a = d_wave_sum(a);
    if (lane == 0u) words[k < 3u * RM_BINS ? rm_off_bc() + k : rm_off_sn() + RM_SN_CONTRIB] = a;
}
#endif
#endif
