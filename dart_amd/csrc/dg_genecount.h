// dg_genecount.h -- gene-level read counts on the device: the units of the batch that has just been mapped (mates 2i and 2i + 1 are still neighbours, their
// reports, CIGARs and MAPQ are in HBM) are counted per gene in a table that stays in HBM across batches and is merged at the end of the job, the position
// dg_batch_accumulate_sj takes for junctions.  Modelled on `htseq-count --mode union` with the layout of STAR's ReadsPerGene.out.tab; neither tool is run
// anywhere: the definition below is what the tests pin (tests/genecount_inputs.py is its sequential twin).
//
// Annotation.  n_genes >= 1 genes and n_exons >= 0 exons (chr, start, end, strand, gene): 0 <= chr < n_chr; start < end <= 2^32 - 1, 0-based half-open on the
//   chromosome; strand 0 (+) or 1 (-); 0 <= gene < n_genes.  Anything else is DG_ERR_ARG, the text names the first bad exon.  Exons may arrive in any order,
//   may overlap and may repeat.  A gene covers a base on a strand when one of its exons does.  For every base there are three gene sets: `any` (every covering
//   gene), `plus` (covering genes whose exon strand is +), `minus` (those whose exon strand is -).  Each set gives a label: GC_NONE (0xFFFFFFFF) for the empty
//   set, the gene's index for exactly one gene, GC_AMBIG (0xFFFFFFFE) for two or more.  gc_flatten (host, once per job, O(exons log exons)) turns the
//   annotation into a segment table per chromosome: ascending breakpoints, per segment the three labels, neighbouring segments with three equal labels merged,
//   the segment behind a chromosome's last exon GC_NONE.  The table is uploaded once and kept with the index, shared by its clones.
// A read's alignment.  Read k is aligned when reads[k].score > 0 and it has a report j >= best that the SAM formatter would show: aln_score > 0 in pair mode
//   (k < n_pair_mode), aln_score == score otherwise (sam.py::format_records).  Its alignment is the first such report, the first SAM line the read prints.
// A read's strand.  s = (flag >> 4 & 1) ^ (flag >> 7 & 1) of that report: the coverage track's rule, a second mate counts for the opposite strand.
// A read's blocks.  p = pos - 1 (the report's pos is 1-based); op 0, 7 or 8 of length L > 0 is a block [p, p + L), then p += L; op 2 or 3 moves p and makes
//   no block; every other op changes nothing.  A read with pos < 1 or chr outside [0, n_chr) has no blocks.
// A unit.  Reads 2i, 2i + 1 form one unit for 2i + 1 < n_pair_mode (even, at most n_reads, the meaning it has for dg_batch_format_sam); every read from
//   n_pair_mode on is a unit of its own.
// A unit's outcome, decided in this order:
//   1. no read of the unit is aligned: N_unmapped;
//   2. an aligned read of the unit has mapq < min_mapq: N_multimapping (DART's MAPQ takes the values 0, 1, 2, 3 and 50; `dart` passes 4, the -unique rule);
//   3. otherwise, for each of three columns, the labels of every segment that every block of every aligned read of the unit touches are combined; a block on a
//      chromosome without segments, or outside them, contributes GC_NONE.  Column 0 (unstranded) reads `any`; column 1 (forward, htseq-count -s yes) reads
//      `plus` when the read's s == 0 and `minus` otherwise; column 2 (reverse) reads the opposite label.  Each read uses its own s.  Combine: NONE + x = x,
//      g + g = g, g + h = AMBIG for g != h, AMBIG + x = AMBIG.  Result g: the unit counts once for gene g in that column (two mates in one gene count once);
//      NONE: N_noFeature of that column; AMBIG: N_ambiguous of that column.  A unit in case 1 or 2 adds to all three columns of its row.
// Counts.  uint64_t counts[4 + n_genes][3]; rows 0-3 are N_unmapped, N_multimapping, N_noFeature, N_ambiguous, row 4 + g is gene g.  Every column sums to the
//   number of units counted.  The table is a function of the multiset of units: not of their order, the batch split, the grid, the contexts or the merges.
// Text (made by the host, STAR's layout): "N_unmapped\t%llu\t%llu\t%llu\n" ... "N_ambiguous...", then "name\tc0\tc1\tc2\n" per gene in the caller's order.
//
// Everything without atomics -- the show rule, the strand, the block walk, the segment look-up (binary search for the segment that holds a block's start, then
// a walk while seg_start < block end), the combine operator -- is __host__ __device__ and shared with the CPU suite (tests/native/genecount_checks.hip).
//   k_gc_count   lane = unit: reads the unit's one or two dg_read_out, their alignment reports, CIGAR ops and the segment table, and has one row per column.
//                Gene rows: equal rows of a wave are combined first (as k_sj_insert combines equal keys), the leader adds the lane count with one agent-scope
//                64-bit atomic -- real data puts a large share of a batch on a handful of genes.  The four N_* rows never see an atomic: ballots per wave,
//                summed per workgroup through LDS, one 12-word line per workgroup
//   k_gc_top     one workgroup: the lines of all workgroups added to rows 0-3 of the table
//   k_gc_add     one table added to another (merge, host counts folded in)
// No lane reads outside the arrays it was given: report and CIGAR ranges that leave them count as "not aligned" / "no blocks".
#ifndef DG_GENECOUNT_H
#define DG_GENECOUNT_H
#include "../../include/dartgpu.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <map>
#include <vector>

#define GC_HD __host__ __device__ __forceinline__
#define GC_THREADS 256           // units per workgroup of k_gc_count (dg_gene_granules [0])
#define GC_WAVE 64               // the lanes whose equal rows are combined (dg_gene_granules [1])
#define GC_NONE 0xFFFFFFFFu
#define GC_AMBIG 0xFFFFFFFEu
#define GC_MAX_GENES 0x7FFFFFF0u
enum { GC_ROW_UNMAPPED = 0, GC_ROW_MULTI, GC_ROW_NOFEATURE, GC_ROW_AMBIG, GC_ROW_GENE0 };

// the segment table: segment i of chromosome c (chr_first[c] <= i < chr_first[c + 1]) begins at seg_start[i] and ends where the next begins (the last one, all
// GC_NONE, never ends); seg_lab[3 i + 0 / 1 / 2] = any / plus / minus
struct GcTable { const uint32_t *chr_first, *seg_start, *seg_lab; int n_chr; };
// the records of a batch, as dg_batch_run leaves them or as the caller of dg_gene_count_records holds them
struct GcBatch { const dg_read_out *ro; const dg_report_out *po; const uint32_t *cig; unsigned long long n_reports, n_ops; int n_reads, n_pair_mode; uint32_t min_mapq; };

GC_HD uint32_t gc_combine(uint32_t a, uint32_t b) { return a == GC_NONE ? b : (b == GC_NONE || a == b) ? a : GC_AMBIG; }
GC_HD uint32_t gc_row(uint32_t label) { return label == GC_NONE ? (uint32_t)GC_ROW_NOFEATURE : label == GC_AMBIG ? (uint32_t)GC_ROW_AMBIG : (uint32_t)GC_ROW_GENE0 + label; }
GC_HD int gc_strand(int flag) { return (flag >> 4 & 1) ^ (flag >> 7 & 1); }
GC_HD unsigned long long gc_units(int n_reads, int n_pair_mode) { return (unsigned long long)(n_pair_mode / 2) + (unsigned long long)(n_reads - n_pair_mode); }
// the reads of unit u: first, and how many (1 or 2)
GC_HD int gc_unit_first(int n_pair_mode, unsigned long long u, int &n) { const unsigned long long h = (unsigned long long)(n_pair_mode / 2); n = u < h ? 2 : 1; return u < h ? (int)(2 * u) : (int)(u - h) + n_pair_mode; }

// the read's alignment: the index of its first shown report inside the report array, or -1
GC_HD long long gc_alignment(const GcBatch &b, int k)
{
    const dg_read_out r = b.ro[k];
    if (r.score <= 0 || r.n_rep <= 0 || r.rep_off < 0 || r.best < 0) return -1;
    if ((unsigned long long)r.rep_off + (unsigned long long)r.n_rep > b.n_reports) return -1;
    const bool pair = k < b.n_pair_mode;
    for (int j = r.best; j < r.n_rep; j++) {
        const int as = b.po[r.rep_off + j].aln_score;
        if (pair ? as > 0 : as == r.score) return (long long)r.rep_off + j;
    }
    return -1;
}

// the labels of every segment of [lo, hi) that the block [s, e) touches, combined into the three columns of a read of strand `strand`
GC_HD void gc_touch(const GcTable &t, uint32_t lo, uint32_t hi, unsigned long long s, unsigned long long e, int strand, uint32_t &a0, uint32_t &a1, uint32_t &a2)
{
    if (lo == hi) return;
    uint32_t l = lo, h = hi;                        // the first segment that begins behind s
    while (l < h) { const uint32_t m = l + (h - l) / 2; if ((unsigned long long)t.seg_start[m] <= s) l = m + 1; else h = m; }
    for (uint32_t i = l > lo ? l - 1 : lo; i < hi && (unsigned long long)t.seg_start[i] < e; i++) {
        const uint32_t any = t.seg_lab[3 * (size_t)i], plus = t.seg_lab[3 * (size_t)i + 1], minus = t.seg_lab[3 * (size_t)i + 2];
        a0 = gc_combine(a0, any); a1 = gc_combine(a1, strand ? minus : plus); a2 = gc_combine(a2, strand ? plus : minus);
    }
}

// the blocks of report `at`
GC_HD void gc_read_blocks(const GcBatch &b, const GcTable &t, long long at, uint32_t &a0, uint32_t &a1, uint32_t &a2)
{
    const dg_report_out p = b.po[at];
    if (p.pos < 1 || p.chr < 0 || p.chr >= t.n_chr) return;
    if ((unsigned long long)p.cigar_off + (unsigned long long)p.n_cigar > b.n_ops) return;
    const uint32_t lo = t.chr_first[p.chr], hi = t.chr_first[p.chr + 1];
    const int strand = gc_strand(p.flag);
    unsigned long long q = (unsigned long long)p.pos - 1ull;
    for (uint32_t k = 0; k < p.n_cigar; k++) {
        const uint32_t w = b.cig[(size_t)p.cigar_off + k], op = w & 15u, len = w >> 4;
        if (op == 0u || op == 7u || op == 8u) { if (len) gc_touch(t, lo, hi, q, q + len, strand, a0, a1, a2); q += len; }
        else if (op == 2u || op == 3u) q += len;
    }
}

// unit u's row in each of the three columns
GC_HD void gc_unit_rows(const GcBatch &b, const GcTable &t, unsigned long long u, uint32_t &r0, uint32_t &r1, uint32_t &r2)
{
    int n;
    const int k0 = gc_unit_first(b.n_pair_mode, u, n);
    const long long at0 = gc_alignment(b, k0), at1 = n == 2 ? gc_alignment(b, k0 + 1) : -1;
    if (at0 < 0 && at1 < 0) { r0 = r1 = r2 = GC_ROW_UNMAPPED; return; }
    if ((at0 >= 0 && (long long)b.ro[k0].mapq < (long long)b.min_mapq) || (at1 >= 0 && (long long)b.ro[k0 + 1].mapq < (long long)b.min_mapq)) { r0 = r1 = r2 = GC_ROW_MULTI; return; }
    uint32_t a0 = GC_NONE, a1 = GC_NONE, a2 = GC_NONE;
    if (at0 >= 0) gc_read_blocks(b, t, at0, a0, a1, a2);
    if (at1 >= 0) gc_read_blocks(b, t, at1, a0, a1, a2);
    r0 = gc_row(a0); r1 = gc_row(a1); r2 = gc_row(a2);
}

// what dg_gene_count_records checks before anything is counted: -1, or the first read whose ranges leave the arrays
static inline long long gc_first_bad_read(const dg_read_out *ro, int n_reads, const dg_report_out *po, size_t n_reports, size_t n_ops)
{
    for (int k = 0; k < n_reads; k++) {
        const dg_read_out &r = ro[k];
        if (r.rep_off < 0 || r.n_rep < 0 || (unsigned long long)r.rep_off + (unsigned long long)r.n_rep > n_reports) return k;
        if (r.score > 0 && (r.best < 0 || r.best >= r.n_rep)) return k;
        for (int j = 0; j < r.n_rep; j++) {
            const dg_report_out &p = po[r.rep_off + j];
            if ((unsigned long long)p.cigar_off + (unsigned long long)p.n_cigar > n_ops) return k;
        }
    }
    return -1;
}

// The flattening: exons -> chr_first [n_chr + 1], seg_start [n_seg], seg_lab [3 n_seg].  Returns false with a text that names the first bad exon.
static inline bool gc_flatten(int n_chr, uint32_t n_genes, size_t n_exons, const dg_gene_exon *ex, std::vector<uint32_t> &chr_first, std::vector<uint32_t> &seg_start,
                              std::vector<uint32_t> &seg_lab, char *err, size_t err_len)
{
    chr_first.assign((size_t)(n_chr > 0 ? n_chr : 0) + 1, 0u); seg_start.clear(); seg_lab.clear();
    if (n_chr < 1 || n_genes < 1u || n_genes > GC_MAX_GENES || (n_exons && !ex)) { snprintf(err, err_len, "the annotation needs at least one chromosome and one gene (%d chromosomes, %u genes)", n_chr, n_genes); return false; }
    for (size_t i = 0; i < n_exons; i++) {
        const dg_gene_exon &e = ex[i];
        const char *what = e.chr < 0 || e.chr >= n_chr ? "its chromosome is outside the index" : !(e.start < e.end) ? "start < end does not hold" : e.strand > 1u ? "its strand is neither 0 nor 1"
                           : e.gene >= n_genes ? "its gene is outside [0, n_genes)" : nullptr;
        if (what) { snprintf(err, err_len, "exon %zu (chr %d, [%u, %u), strand %u, gene %u): %s", i, e.chr, e.start, e.end, e.strand, e.gene, what); return false; }
    }
    // events (chromosome, position, exon), an exon's end in front of another's start at one position; the active genes of each class with their multiplicity
    struct Ev { uint64_t key; uint32_t exon; };
    std::vector<Ev> ev; ev.reserve(2 * n_exons);
    for (size_t i = 0; i < n_exons; i++) {
        ev.push_back(Ev{(uint64_t)ex[i].chr << 33 | (uint64_t)ex[i].start << 1 | 1u, (uint32_t)i});
        ev.push_back(Ev{(uint64_t)ex[i].chr << 33 | (uint64_t)ex[i].end << 1, (uint32_t)i});
    }
    std::sort(ev.begin(), ev.end(), [](const Ev &a, const Ev &b) { return a.key < b.key; });
    std::map<uint32_t, uint32_t> act[3];
    auto label = [](const std::map<uint32_t, uint32_t> &m) { return m.empty() ? GC_NONE : m.size() == 1 ? m.begin()->first : GC_AMBIG; };
    size_t k = 0;
    for (int c = 0; c < n_chr; c++) {
        chr_first[(size_t)c] = (uint32_t)seg_start.size();
        uint32_t prev[3] = {GC_NONE, GC_NONE, GC_NONE}; bool first = true;
        while (k < ev.size() && (int)(ev[k].key >> 33) == c) {
            const uint64_t pos = ev[k].key >> 1;
            for (; k < ev.size() && ev[k].key >> 1 == pos; k++) {
                const dg_gene_exon &e = ex[ev[k].exon];
                for (int cls : {0, 1 + (int)e.strand}) {
                    if (ev[k].key & 1u) act[cls][e.gene]++;
                    else { auto it = act[cls].find(e.gene); if (--it->second == 0u) act[cls].erase(it); }
                }
            }
            const uint32_t now[3] = {label(act[0]), label(act[1]), label(act[2])};
            if (first || now[0] != prev[0] || now[1] != prev[1] || now[2] != prev[2]) {
                if (seg_start.size() >= 0xFFFFFFF0ull) { snprintf(err, err_len, "the annotation gives more segments than the table holds"); return false; }
                seg_start.push_back((uint32_t)(pos & 0xFFFFFFFFull)); seg_lab.insert(seg_lab.end(), now, now + 3);
                prev[0] = now[0]; prev[1] = now[1]; prev[2] = now[2]; first = false;
            }
        }
    }
    chr_first[(size_t)n_chr] = (uint32_t)seg_start.size();
    return true;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
// one column's row of every lane of the wave: gene rows are combined and added by their leaders; returns to lane r < 4 how many lanes have the N_* row r
// (wave-uniform ballots, no atomic)
__device__ __forceinline__ uint32_t gc_wave_add(unsigned long long *counts, int col, bool valid, uint32_t row, int lane)
{
    const uint32_t t0 = (uint32_t)__popcll(__ballot(valid && row == 0u)), t1 = (uint32_t)__popcll(__ballot(valid && row == 1u));
    const uint32_t t2 = (uint32_t)__popcll(__ballot(valid && row == 2u)), t3 = (uint32_t)__popcll(__ballot(valid && row == 3u));
    unsigned long long todo = __ballot(valid && row >= (uint32_t)GC_ROW_GENE0);          // (the loop and everything in it is wave-uniform: `todo` is a ballot)
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lrow = (uint32_t)__shfl((int)row, leader, GC_WAVE);
        const unsigned long long m = __ballot(valid && row == lrow);
        if (lane == leader) __hip_atomic_fetch_add(counts + 3ull * lrow + (unsigned)col, (unsigned long long)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        todo &= ~m;
    }
    return lane == 0 ? t0 : lane == 1 ? t1 : lane == 2 ? t2 : t3;
}

__global__ void __launch_bounds__(GC_THREADS)
k_gc_count(const GcBatch b, const GcTable t, unsigned long long n_units, unsigned long long *counts, unsigned long long n_rows, unsigned long long *__restrict__ wg_line)
{
    __shared__ uint32_t s_tally[GC_THREADS / GC_WAVE][12];
    const unsigned long long u = (unsigned long long)blockIdx.x * GC_THREADS + threadIdx.x;
    const int lane = (int)(threadIdx.x & (GC_WAVE - 1)), wave = (int)(threadIdx.x / GC_WAVE);
    uint32_t r0 = 0, r1 = 0, r2 = 0;
    bool valid = u < n_units;
    if (valid) gc_unit_rows(b, t, u, r0, r1, r2);
    if ((unsigned long long)r0 >= n_rows || (unsigned long long)r1 >= n_rows || (unsigned long long)r2 >= n_rows) valid = false;      // (a label outside the table it is counted in: never written)
    const uint32_t n0 = gc_wave_add(counts, 0, valid, r0, lane), n1 = gc_wave_add(counts, 1, valid, r1, lane), n2 = gc_wave_add(counts, 2, valid, r2, lane);
    if (lane < 4) { s_tally[wave][3 * lane] = n0; s_tally[wave][3 * lane + 1] = n1; s_tally[wave][3 * lane + 2] = n2; }
    __syncthreads();
    if (threadIdx.x < 12u) {
        unsigned long long v = 0;
        for (int w = 0; w < GC_THREADS / GC_WAVE; w++) v += s_tally[w][threadIdx.x];
        wg_line[(unsigned long long)blockIdx.x * 12ull + threadIdx.x] = v;
    }
}

// rows 0-3 of the table += the lines of n_wg workgroups (one workgroup; 252 = 21 x 12 lanes keep their word of the line)
__global__ void __launch_bounds__(256)
k_gc_top(const unsigned long long *__restrict__ wg_line, unsigned long long n_wg, unsigned long long *counts)
{
    __shared__ unsigned long long s_part[252];
    unsigned long long v = 0;
    if (threadIdx.x < 252u) {
        for (unsigned long long i = threadIdx.x; i < n_wg * 12ull; i += 252ull) v += wg_line[i];
        s_part[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x < 12u) {
        unsigned long long sum = 0;
        for (int j = 0; j < 21; j++) sum += s_part[threadIdx.x + 12 * j];
        counts[threadIdx.x] += sum;
    }
}

__global__ void __launch_bounds__(256)
k_gc_add(unsigned long long *__restrict__ dst, const unsigned long long *__restrict__ src, unsigned long long n)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i < n) dst[i] += src[i];
}
#endif
#endif
