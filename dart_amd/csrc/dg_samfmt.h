// dg_samfmt.h -- SAM text on the device: the records a batch left in HBM -> the bytes OutputPairedAlignments / OutputSingledAlignments
// (Mapping.cpp:208-369) print for them.  The rules are those of format_views (host/fast_fastq.h) and sam.py::format_records, restated once
// in __host__ __device__ functions that the two kernels below and the CPU suite (tests/native/sam_checks.hip) share:
//   k_sam_len     lane = read: the byte length of the read's text and the three counters; every workgroup leaves the exclusive scan of its
//                 256 lengths and their sum
//   k_tiles_top   (dg_wgscan.h) one workgroup: exclusive scan of the workgroup sums (64 bit), the total
//   k_sam_write   wave = read: name, bases and qualities are copied (or reverse-complemented / reversed) lane beside lane; the numeric
//                 fields of a line are composed by lane 0 into LDS and stored from there by the wave
// Every byte's place follows from the scanned lengths alone, so the text is the same whatever the grid.
#ifndef DG_SAMFMT_H
#define DG_SAMFMT_H
#include "../../include/dartgpu.h"
#include "dg_wgscan.h"

#define SAM_HD __host__ __device__ __forceinline__

// everything a line is made of; the record arrays as dg_batch_run leaves them, the reads as the pipeline keeps them (mate 2 stored
// reverse-complemented, its qualities reversed)
struct SamBatch {
    const dg_read_out *ro; const dg_report_out *po; const uint32_t *cig;
    const uint32_t *seq_off; const uint16_t *rlen; const unsigned char *seq;
    const uint32_t *hdr_off; const char *hdr;
    const uint32_t *qual_off; const char *qual;            // qual == nullptr: FASTA, the quality column is '*'
    const uint32_t *chr_off; const char *chr;
    const uint32_t *qlen;                                  // the printed length of every read's quality if it is known already (k_sam_len leaves it for k_sam_write), else nullptr
    int n_reads, n_pair_mode, unique_only, multi;
};

// a byte sink with a capacity: bytes past it are counted, not stored (cap 0: a pure length count; cap ~0u: straight to memory)
struct SamSink {
    char *p; uint32_t n, cap;
    SAM_HD void ch(char c) { if (n < cap) p[n] = c; n++; }
    SAM_HD void lit(const char *s) { while (*s) ch(*s++); }
};

SAM_HD int sam_dec_width(unsigned long long u) { int w = 1; while (u >= 10) { u /= 10; w++; } return w; }
// u < 10^10 in decimal, at least `min_digits` wide: the digits are peeled off from the low end into a BCD word (no array: nothing for scratch memory)
SAM_HD void sam_put_u10(SamSink &o, unsigned long long u, int min_digits)
{
    unsigned long long bcd = 0; int n = 0;
    do { bcd = (bcd << 4) | (u % 10); u /= 10; n++; } while (u || n < min_digits);
    for (; n > 0; n--) { o.ch((char)('0' + (int)(bcd & 15))); bcd >>= 4; }
}
// decimal as printf("%d") / TextBuf::num print it: '-' and the magnitude
SAM_HD void sam_put_num(SamSink &o, long long v)
{
    const unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
    if (v < 0) o.ch('-');
    if (u >= 10000000000ull) { sam_put_u10(o, u / 10000000000ull, 1); sam_put_u10(o, u % 10000000000ull, 10); }
    else sam_put_u10(o, u, 1);
}
// comp_base (tools.cpp:3-17): everything but ACGTacgt becomes N, lower case maps to upper
SAM_HD char sam_comp_base(char c)
{
    switch (c) {
    case 'A': case 'a': return 'T';
    case 'C': case 'c': return 'G';
    case 'G': case 'g': return 'C';
    case 'T': case 't': return 'A';
    default: return 'N';
    }
}

// what is fixed per read
struct SamRead {
    bool is_pair, mate2;
    const dg_read_out *r; const dg_report_out *rp, *mp;
    const char *h; const unsigned char *s; const char *q;
    uint32_t hl, sl, ql, sl_mate;
};
SAM_HD SamRead sam_read_begin(const SamBatch &b, int k)
{
    SamRead e;
    e.is_pair = k < b.n_pair_mode; e.mate2 = e.is_pair && (k & 1);
    e.r = b.ro + k; e.rp = b.po + e.r->rep_off;
    e.mp = e.is_pair ? b.po + b.ro[k ^ 1].rep_off : nullptr;
    e.h = b.hdr + b.hdr_off[k]; e.hl = b.hdr_off[k + 1] - b.hdr_off[k];
    e.s = b.seq + b.seq_off[k]; e.sl = b.rlen[k]; e.sl_mate = e.is_pair ? b.rlen[k ^ 1] : 0u;
    e.q = nullptr; e.ql = 0;
    if (b.qual) {                       // the reference prints the stored quality as a C string: it ends at its first NUL byte
        e.q = b.qual + b.qual_off[k];
        if (b.qlen) e.ql = b.qlen[k];
        else {
            const uint32_t full = b.qual_off[k + 1] - b.qual_off[k];
            uint32_t z = 0;
            while (z < full && e.q[z] != 0) z++;
            e.ql = z;
        }
    }
    return e;
}
#define SAM_LINE_UNMAPPED (-1)
#define SAM_LINE_NONE (-2)
// the first line of a read: SAM_LINE_UNMAPPED, SAM_LINE_NONE (-unique hides it), or sam_line_next from `best`
SAM_HD int sam_line_next(const SamBatch &b, const SamRead &e, int j)
{
    for (; j < e.r->n_rep; j++) {
        const int as = e.rp[j].aln_score;
        if (e.is_pair ? as > 0 : as == e.r->score) return j;
        if (e.is_pair && !b.multi) break;
    }
    return SAM_LINE_NONE;
}
SAM_HD int sam_line_first(const SamBatch &b, const SamRead &e)
{
    if (e.r->score == 0) return SAM_LINE_UNMAPPED;
    if (b.unique_only && !(e.r->mapq > 3)) return SAM_LINE_NONE;
    return sam_line_next(b, e, e.r->best);
}
SAM_HD int sam_line_after(const SamBatch &b, const SamRead &e, int j)
{
    if (j < 0 || !b.multi) return SAM_LINE_NONE;
    return sam_line_next(b, e, j + 1);
}
// print the reverse complement of the stored read, and its quality reversed
SAM_HD bool sam_line_alt(const SamRead &e, int j) { return j >= 0 && (e.mate2 ? e.rp[j].bdir == 1 : e.rp[j].bdir == 0); }
// the mate fields apply: the report's partner exists and is shown itself
SAM_HD bool sam_line_mated(const SamRead &e, int j)
{
    if (j < 0 || !e.is_pair) return false;
    const int pj = e.rp[j].paired_idx;
    return pj != -1 && e.mp[pj].aln_score > 0;
}
// between the name and the bases: FLAG .. TLEN with their tabs
SAM_HD void sam_line_mid(const SamBatch &b, const SamRead &e, int j, SamSink &o)
{
    if (j < 0) { o.ch('\t'); sam_put_num(o, e.rp[0].flag); o.lit("\t*\t0\t0\t*\t*\t0\t0\t"); return; }
    const dg_report_out &pr = e.rp[j];
    o.ch('\t'); sam_put_num(o, pr.flag); o.ch('\t');
    for (uint32_t i = b.chr_off[pr.chr]; i < b.chr_off[pr.chr + 1]; i++) o.ch(b.chr[i]);
    o.ch('\t'); sam_put_num(o, (long long)pr.pos); o.ch('\t'); sam_put_num(o, e.r->mapq); o.ch('\t');
    for (uint32_t c = 0; c < pr.n_cigar; c++) { const uint32_t op = b.cig[pr.cigar_off + c]; sam_put_num(o, op >> 4); o.ch((op & 15) < 5 ? "MIDNS"[op & 15] : '?'); }
    if (sam_line_mated(e, j)) {
        const dg_report_out &mr = e.mp[pr.paired_idx];
        const dg_report_out &a = e.mate2 ? mr : pr, &bb = e.mate2 ? pr : mr;
        const int l1 = (int)(e.mate2 ? e.sl_mate : e.sl), l2 = (int)(e.mate2 ? e.sl : e.sl_mate);
        int dist = (int)(bb.pos - a.pos + (a.bdir ? l2 : 0 - l1));         // 32 bit, as the reference's int
        if (e.mate2) dist = (int)(0u - (unsigned)dist);
        o.lit("\t=\t"); sam_put_num(o, (long long)mr.pos); o.ch('\t'); sam_put_num(o, dist); o.ch('\t');
    } else o.lit("\t*\t0\t0\t");
}
// behind the qualities: the tags and the line end
SAM_HD void sam_line_tail(const SamRead &e, int j, SamSink &o)
{
    if (j < 0) { o.lit("\tAS:i:0\tXS:i:0\n"); return; }
    o.lit("\tNM:i:"); sam_put_num(o, e.r->mis_num); o.lit("\tAS:i:"); sam_put_num(o, e.r->score); o.lit("\tXS:i:"); sam_put_num(o, e.r->sub_score);
    const int t = e.rp[j].sj_type;
    if (t != -1) o.lit(((t == 0 || t == 2) != e.mate2) ? " XS:A:+" : " XS:A:-");
    o.ch('\n');
}
SAM_HD uint32_t sam_qual_len(const SamBatch &b, const SamRead &e) { return b.qual ? e.ql : 1u; }
SAM_HD uint64_t sam_line_len(const SamBatch &b, const SamRead &e, int j)
{
    SamSink o{nullptr, 0, 0};
    sam_line_mid(b, e, j, o); sam_line_tail(e, j, o);
    return (uint64_t)e.hl + o.n + e.sl + 1u + sam_qual_len(b, e);
}
// one read in pass 1: the length of its text; ct[0] unmapped, ct[1] unique (mapq == 50), ct[2] paired (+2 for mate 1's best line with a shown mate)
SAM_HD uint64_t sam_read_len(const SamBatch &b, int k, uint32_t ct[3], uint32_t *ql = nullptr)
{
    const SamRead e = sam_read_begin(b, k);
    if (ql) *ql = e.ql;
    uint64_t len = 0;
    if (e.r->score == 0) ct[0]++;
    else if (!b.unique_only || e.r->mapq > 3) { if (e.r->mapq == 50) ct[1]++; }
    for (int j = sam_line_first(b, e); j != SAM_LINE_NONE; j = sam_line_after(b, e, j)) {
        len += sam_line_len(b, e, j);
        if (j >= 0 && !e.mate2 && j == e.r->best && sam_line_mated(e, j)) ct[2] += 2;
    }
    return len;
}
// one read's text, byte by byte (the CPU suite's writer, and what k_sam_write's cooperative copies must equal); returns the bytes written
SAM_HD uint64_t sam_read_text(const SamBatch &b, int k, char *out)
{
    const SamRead e = sam_read_begin(b, k);
    uint64_t n = 0;
    for (int j = sam_line_first(b, e); j != SAM_LINE_NONE; j = sam_line_after(b, e, j)) {
        const bool alt = sam_line_alt(e, j);
        for (uint32_t i = 0; i < e.hl; i++) out[n++] = e.h[i];
        SamSink o{out + n, 0, 0xFFFFFFFFu};
        sam_line_mid(b, e, j, o); n += o.n;
        for (uint32_t i = 0; i < e.sl; i++) out[n++] = alt ? sam_comp_base((char)e.s[e.sl - 1 - i]) : (char)e.s[i];
        out[n++] = '\t';
        if (!b.qual) out[n++] = '*';
        else for (uint32_t i = 0; i < e.ql; i++) out[n++] = alt ? e.q[e.ql - 1 - i] : e.q[i];
        SamSink t{out + n, 0, 0xFFFFFFFFu};
        sam_line_tail(e, j, t); n += t.n;
    }
    return n;
}

// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
#define SAM_LEN_THREADS 256
static_assert(SAM_LEN_THREADS == WG_THREADS, "k_sam_len and k_bam_len scan with d_wg_exclusive");
#define SAM_MID_STAGE 192        // bytes of LDS for a line's FLAG .. TLEN (a line with more -- hundreds of CIGAR ops, a long chromosome name -- is written by lane 0 alone)
#define SAM_TAIL_STAGE 64        // the tags never exceed 59 bytes
static_assert(3 * 11 + 3 * 6 + 7 + 1 <= SAM_TAIL_STAGE, "the tags fit their staging area");

// stat[0] total bytes (k_tiles_top), stat[1..3] the counters
__global__ void __launch_bounds__(SAM_LEN_THREADS)
k_sam_len(const SamBatch b, uint64_t *__restrict__ read_off, uint32_t *__restrict__ qlen_out, uint64_t *__restrict__ tile_sum, unsigned long long *__restrict__ stat)
{
    __shared__ uint64_t s_wave[SAM_LEN_THREADS / 64];
    __shared__ uint32_t s_ct[3];
    const int k = (int)(blockIdx.x * SAM_LEN_THREADS + threadIdx.x);
    if (threadIdx.x < 3) s_ct[threadIdx.x] = 0;
    uint32_t ct[3] = {0, 0, 0};
    uint32_t ql = 0;
    const uint64_t len = k < b.n_reads ? sam_read_len(b, k, ct, &ql) : 0ull;
    uint64_t all;
    const uint64_t ex = d_wg_exclusive<uint64_t>(len, all, s_wave);
    if (k < b.n_reads) { read_off[k] = ex; qlen_out[k] = ql; }
#pragma unroll
    for (int i = 0; i < 3; i++) if (ct[i]) atomicAdd(&s_ct[i], ct[i]);
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
    if (threadIdx.x < 3 && s_ct[threadIdx.x]) atomicAdd(&stat[1 + threadIdx.x], (unsigned long long)s_ct[threadIdx.x]);
}

// One wave per workgroup, one workgroup per read (no loop over reads: what is fixed per read then lives in scalar registers for that read only, and
// the kernel needs no spills).  The read index is the same in every lane, so which lines exist and where they start is decided by all lanes
// alike; lane 0 composes the numeric fields.  Nothing is written when the text does not fit `cap`
// (the host grows the buffer and launches this kernel alone again).
__global__ void __launch_bounds__(64)
k_sam_write(const SamBatch b, const uint64_t *__restrict__ read_off, const uint64_t *__restrict__ tile_base, const unsigned long long *__restrict__ stat,
            unsigned long long cap, char *__restrict__ out)
{
    __shared__ char s_mid[SAM_MID_STAGE];
    __shared__ char s_tail[SAM_TAIL_STAGE];
    __shared__ uint32_t s_n[2];
    if (stat[0] > cap) return;
    const uint32_t lane = threadIdx.x;
    const int k = (int)blockIdx.x;
    if (k < b.n_reads) {
        const SamRead e = sam_read_begin(b, k);
        char *dst = out + read_off[k] + tile_base[k / SAM_LEN_THREADS];
        for (int j = sam_line_first(b, e); j != SAM_LINE_NONE; j = sam_line_after(b, e, j)) {
            const bool alt = sam_line_alt(e, j);
            __syncthreads();                                   // the previous line's staged bytes have been read
            if (lane == 0) {
                // into the staging area; a line whose fields outgrow it goes straight to its place in the text, by this lane alone (the plain path)
                SamSink m{s_mid, 0, SAM_MID_STAGE};
#pragma nounroll
                for (int plain = 0; plain < 2; plain++) {
                    sam_line_mid(b, e, j, m);
                    if (m.n <= m.cap) break;
                    m = SamSink{dst + e.hl, 0, 0xFFFFFFFFu};
                }
                SamSink t{s_tail, 0, SAM_TAIL_STAGE};
                sam_line_tail(e, j, t);
                s_n[0] = m.n; s_n[1] = t.n;
            }
            for (uint32_t i = lane; i < e.hl; i += 64) dst[i] = e.h[i];
            __syncthreads();
            const uint32_t mid_n = s_n[0], tail_n = s_n[1];
            char *p = dst + e.hl;
            if (mid_n <= SAM_MID_STAGE) { for (uint32_t i = lane; i < mid_n; i += 64) p[i] = s_mid[i]; }
            p += mid_n;
            if (alt) { for (uint32_t i = lane; i < e.sl; i += 64) p[i] = sam_comp_base((char)e.s[e.sl - 1 - i]); }
            else { for (uint32_t i = lane; i < e.sl; i += 64) p[i] = (char)e.s[i]; }
            p += e.sl;
            if (lane == 0) p[0] = '\t';
            p++;
            if (!b.qual) { if (lane == 0) p[0] = '*'; p++; }
            else {
                if (alt) { for (uint32_t i = lane; i < e.ql; i += 64) p[i] = e.q[e.ql - 1 - i]; }
                else { for (uint32_t i = lane; i < e.ql; i += 64) p[i] = e.q[i]; }
                p += e.ql;
            }
            for (uint32_t i = lane; i < tail_n; i += 64) p[i] = s_tail[i];       // (three numbers of at most 11 characters and 26 fixed ones: the tags always fit)
            dst = p + tail_n;
        }
    }
}
#endif
