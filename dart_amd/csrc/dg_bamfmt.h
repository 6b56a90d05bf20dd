// dg_bamfmt.h -- BAM records on the device: the records a batch left in HBM -> the uncompressed BAM records of `-bo`.
// A record is defined by the host writer: the bytes BamWriter::sam_line_to_bam (host/bam_writer.h) produces for the SAM line dg_samfmt.h prints for
// that (read, report) -- no bytes for a line the writer refuses.  The text is never built: which lines exist and what FLAG, POS, MAPQ, the mate
// fields, TLEN, NM, AS and XS are comes from dg_samfmt.h's per-read functions; this file restates what the writer makes of them
// (names without tab or newline and the index's chromosome names -- distinct, not empty, neither "*" nor "=" -- as this program prints them):
//   k_bam_len     lane = read: the bytes of all its records, the SAM formatter's three counters, records written and lines refused; every
//                 workgroup leaves the exclusive scan of its 256 lengths and their sum
//   k_tiles_top   (dg_wgscan.h) one workgroup: the scan of the workgroup sums, the total
//   k_bam_write   wave = read: lane i on byte i of the name, the packed bases and the qualities, lane c on CIGAR op c; lane 0 composes the 36
//                 fixed bytes and the tags in LDS, the wave stores them
// Every byte's place follows from the scanned lengths alone, so the array is the same whatever the grid.
#ifndef DG_BAMFMT_H
#define DG_BAMFMT_H
#include "dg_samfmt.h"

// htslib's seq_nt16_table as sam_parse1 applies it: "=ACMGRSVTWYHKDBN", lower case folded, everything else (a '-', a NUL) 15
SAM_HD uint32_t bam_base_code(char c)
{
    switch (c >= 'a' && c <= 'z' ? (char)(c - 32) : c) {
    case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7;
    case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14;
    default: return 15;
    }
}
// SAM specification 5.3 (hts_reg2bin, min_shift 14, 5 levels) in 64 bits
SAM_HD uint32_t bam_reg2bin(long long beg, long long end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}
SAM_HD void bam_put32(unsigned char *p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24); }
// an integer tag in the smallest type that holds it, by the writer's rule: a printed '-' takes the signed types, everything else the unsigned ones
SAM_HD uint32_t bam_tag_width(int v) { return v < 0 ? (v >= -128 ? 1u : v >= -32768 ? 2u : 4u) : (v <= 255 ? 1u : v <= 65535 ? 2u : 4u); }
SAM_HD uint32_t bam_put_tag(unsigned char *p, char a, char b, int v)
{
    const uint32_t w = bam_tag_width(v);
    p[0] = (unsigned char)a; p[1] = (unsigned char)b;
    p[2] = (unsigned char)(v < 0 ? (w == 1 ? 'c' : w == 2 ? 's' : 'i') : (w == 1 ? 'C' : w == 2 ? 'S' : 'I'));
    for (uint32_t i = 0; i < w; i++) p[3 + i] = (unsigned char)((uint32_t)v >> (8 * i));
    return 3u + w;
}
#define BAM_FIXED 36             // block_size and the 32 bytes up to the name
#define BAM_TAGS_MAX 21          // three tags of at most 3 + 4 bytes

// the printed base / quality byte i of a line (alt: the reverse complement of the stored read, its quality reversed)
SAM_HD char bam_base_at(const SamRead &e, bool alt, uint32_t i) { return alt ? sam_comp_base((char)e.s[e.sl - 1 - i]) : (char)e.s[i]; }
SAM_HD char bam_qual_at(const SamRead &e, bool alt, uint32_t i) { return alt ? e.q[e.ql - 1 - i] : e.q[i]; }
// l_seq: the printed bases, none when the column is the single byte '*'
SAM_HD uint32_t bam_line_lseq(const SamRead &e, bool alt) { return e.sl == 1 && bam_base_at(e, alt, 0) == '*' ? 0u : e.sl; }
// the quality column is '*': FASTA input, or a printed quality that is this one byte
SAM_HD bool bam_line_no_qual(const SamBatch &b, const SamRead &e) { return !b.qual || (e.ql == 1 && e.q[0] == '*'); }
SAM_HD uint32_t bam_line_ncigar(const SamRead &e, int j) { return j < 0 ? 0u : e.rp[j].n_cigar; }
SAM_HD uint32_t bam_line_tags(const SamRead &e, int j, unsigned char *t)
{
    uint32_t n = 0;
    if (j < 0) { n += bam_put_tag(t + n, 'A', 'S', 0); n += bam_put_tag(t + n, 'X', 'S', 0); return n; }
    n += bam_put_tag(t + n, 'N', 'M', e.r->mis_num); n += bam_put_tag(t + n, 'A', 'S', e.r->score); n += bam_put_tag(t + n, 'X', 'S', e.r->sub_score);
    return n;
}
// the bytes of a line's record with its block_size field; 0: the writer refuses the line (a name of 0 or more than 254 bytes, a printed quality whose
// length differs from l_seq, a CIGAR op the formatter prints as '?')
SAM_HD uint32_t bam_line_size(const SamBatch &b, const SamRead &e, int j)
{
    if (e.hl == 0 || e.hl > 254) return 0;
    const uint32_t l_seq = bam_line_lseq(e, sam_line_alt(e, j));
    if (!bam_line_no_qual(b, e) && e.ql != l_seq) return 0;
    const uint32_t nc = bam_line_ncigar(e, j);
    for (uint32_t c = 0; c < nc; c++) if ((b.cig[e.rp[j].cigar_off + c] & 15u) >= 5u) return 0;
    const uint32_t tags = j < 0 ? 8u : 9u + bam_tag_width(e.r->mis_num) + bam_tag_width(e.r->score) + bam_tag_width(e.r->sub_score);
    return BAM_FIXED + e.hl + 1u + 4u * nc + (l_seq + 1u) / 2u + l_seq + tags;
}
// block_size .. tlen
SAM_HD void bam_line_fixed(const SamBatch &b, const SamRead &e, int j, uint32_t size, unsigned char *o)
{
    const uint32_t l_seq = bam_line_lseq(e, sam_line_alt(e, j));
    int refid = -1, mrefid = -1, flag = e.rp[0].flag, mapq = 0, tlen = 0;
    long long pos = -1, mpos = -1, rlen = 0;
    uint32_t nc = 0;
    if (j >= 0) {
        const dg_report_out &pr = e.rp[j];
        refid = pr.chr; flag = pr.flag; mapq = e.r->mapq; pos = (long long)pr.pos - 1; nc = pr.n_cigar;
        for (uint32_t c = 0; c < nc; c++) { const uint32_t op = b.cig[pr.cigar_off + c]; if ((op & 15u) == 0 || (op & 15u) == 2 || (op & 15u) == 3) rlen += (long long)(op >> 4); }
        if (sam_line_mated(e, j)) {                            // (TLEN as sam_line_mid prints it)
            const dg_report_out &mr = e.mp[pr.paired_idx];
            const dg_report_out &a = e.mate2 ? mr : pr, &bb = e.mate2 ? pr : mr;
            const int l1 = (int)(e.mate2 ? e.sl_mate : e.sl), l2 = (int)(e.mate2 ? e.sl : e.sl_mate);
            int dist = (int)(bb.pos - a.pos + (a.bdir ? l2 : 0 - l1));
            if (e.mate2) dist = (int)(0u - (unsigned)dist);
            mrefid = refid; mpos = (long long)mr.pos - 1; tlen = dist;
        }
    }
    if (nc == 0) flag |= 4;                                    // (sam_parse1: a line without CIGAR is marked unmapped)
    const uint32_t bin = bam_reg2bin(pos, pos + (rlen > 0 ? rlen : 1));
    bam_put32(o, size - 4u);
    bam_put32(o + 4, (uint32_t)refid); bam_put32(o + 8, (uint32_t)pos);
    bam_put32(o + 12, (bin << 16) | ((uint32_t)(mapq & 0xff) << 8) | (e.hl + 1u));
    bam_put32(o + 16, ((uint32_t)flag << 16) | (nc & 0xffffu));
    bam_put32(o + 20, l_seq); bam_put32(o + 24, (uint32_t)mrefid); bam_put32(o + 28, (uint32_t)mpos); bam_put32(o + 32, (uint32_t)tlen);
}
SAM_HD unsigned char bam_seq_byte(const SamRead &e, bool alt, uint32_t l_seq, uint32_t i)
{
    const uint32_t hi = bam_base_code(bam_base_at(e, alt, 2 * i)), lo = 2 * i + 1 < l_seq ? bam_base_code(bam_base_at(e, alt, 2 * i + 1)) : 0u;
    return (unsigned char)(hi << 4 | lo);
}
// one read in pass 1: the bytes of its records; ct as sam_read_len counts them, rr[0] records written, rr[1] lines refused
SAM_HD uint64_t bam_read_len(const SamBatch &b, int k, uint32_t ct[3], uint32_t rr[2], uint32_t *ql = nullptr)
{
    uint32_t q = 0;
    (void)sam_read_len(b, k, ct, &q);                          // the counters, and the printed length of the quality
    if (ql) *ql = q;
    SamBatch b2 = b; b2.qual = nullptr;                        // (not measured a second time)
    SamRead e = sam_read_begin(b2, k);
    if (b.qual) { e.q = b.qual + b.qual_off[k]; e.ql = q; }
    uint64_t len = 0;
    for (int j = sam_line_first(b, e); j != SAM_LINE_NONE; j = sam_line_after(b, e, j)) {
        const uint32_t sz = bam_line_size(b, e, j);
        len += sz;
        rr[sz ? 0 : 1]++;
    }
    return len;
}
// one read's records, byte by byte (the CPU suite's writer, and what k_bam_write's cooperative stores must equal); returns the bytes written
SAM_HD uint64_t bam_read_records(const SamBatch &b, int k, unsigned char *out)
{
    const SamRead e = sam_read_begin(b, k);
    uint64_t n = 0;
    for (int j = sam_line_first(b, e); j != SAM_LINE_NONE; j = sam_line_after(b, e, j)) {
        const uint32_t sz = bam_line_size(b, e, j);
        if (!sz) continue;
        const bool alt = sam_line_alt(e, j);
        const uint32_t l_seq = bam_line_lseq(e, alt), nc = bam_line_ncigar(e, j);
        unsigned char *p = out + n;
        bam_line_fixed(b, e, j, sz, p); p += BAM_FIXED;
        for (uint32_t i = 0; i < e.hl; i++) *p++ = (unsigned char)e.h[i];
        *p++ = 0;
        for (uint32_t c = 0; c < nc; c++) { bam_put32(p, b.cig[e.rp[j].cigar_off + c]); p += 4; }
        for (uint32_t i = 0; i < (l_seq + 1u) / 2u; i++) *p++ = bam_seq_byte(e, alt, l_seq, i);
        const bool nq = bam_line_no_qual(b, e);
        for (uint32_t i = 0; i < l_seq; i++) *p++ = nq ? (unsigned char)0xff : (unsigned char)(bam_qual_at(e, alt, i) - 33);
        p += bam_line_tags(e, j, p);
        n += sz;
    }
    return n;
}

// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
// stat[0] total bytes (k_tiles_top), stat[1..3] the SAM formatter's counters, stat[4] records written, stat[5] lines refused
__global__ void __launch_bounds__(SAM_LEN_THREADS)
k_bam_len(const SamBatch b, uint64_t *__restrict__ read_off, uint32_t *__restrict__ qlen_out, uint64_t *__restrict__ tile_sum, unsigned long long *__restrict__ stat)
{
    __shared__ uint64_t s_wave[SAM_LEN_THREADS / 64];
    __shared__ uint32_t s_ct[5];
    const int k = (int)(blockIdx.x * SAM_LEN_THREADS + threadIdx.x);
    if (threadIdx.x < 5) s_ct[threadIdx.x] = 0;
    uint32_t ct[3] = {0, 0, 0}, rr[2] = {0, 0};
    uint32_t ql = 0;
    const uint64_t len = k < b.n_reads ? bam_read_len(b, k, ct, rr, &ql) : 0ull;
    uint64_t all;
    const uint64_t ex = d_wg_exclusive<uint64_t>(len, all, s_wave);
    if (k < b.n_reads) { read_off[k] = ex; qlen_out[k] = ql; }
#pragma unroll
    for (int i = 0; i < 3; i++) if (ct[i]) atomicAdd(&s_ct[i], ct[i]);
#pragma unroll
    for (int i = 0; i < 2; i++) if (rr[i]) atomicAdd(&s_ct[3 + i], rr[i]);
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
    if (threadIdx.x < 5 && s_ct[threadIdx.x]) atomicAdd(&stat[1 + threadIdx.x], (unsigned long long)s_ct[threadIdx.x]);
}

// One wave per workgroup, one workgroup per read, as k_sam_write.  Nothing is written when the records do not fit `cap` (the host grows the buffer
// and launches this kernel alone again).
__global__ void __launch_bounds__(64)
k_bam_write(const SamBatch b, const uint64_t *__restrict__ read_off, const uint64_t *__restrict__ tile_base, const unsigned long long *__restrict__ stat,
            unsigned long long cap, unsigned char *__restrict__ out)
{
    __shared__ unsigned char s_fix[BAM_FIXED];
    __shared__ unsigned char s_tags[BAM_TAGS_MAX + 3];
    __shared__ uint32_t s_n;
    if (stat[0] > cap) return;
    const uint32_t lane = threadIdx.x;
    const int k = (int)blockIdx.x;
    if (k < b.n_reads) {
        const SamRead e = sam_read_begin(b, k);
        unsigned char *dst = out + read_off[k] + tile_base[k / SAM_LEN_THREADS];
        const bool nq = bam_line_no_qual(b, e);
        for (int j = sam_line_first(b, e); j != SAM_LINE_NONE; j = sam_line_after(b, e, j)) {
            const uint32_t sz = bam_line_size(b, e, j);
            if (!sz) continue;
            const bool alt = sam_line_alt(e, j);
            const uint32_t l_seq = bam_line_lseq(e, alt), nc = bam_line_ncigar(e, j);
            __syncthreads();                                   // the previous record's staged bytes have been read
            if (lane == 0) { bam_line_fixed(b, e, j, sz, s_fix); s_n = bam_line_tags(e, j, s_tags); }
            unsigned char *p = dst + BAM_FIXED;
            for (uint32_t i = lane; i < e.hl; i += 64) p[i] = (unsigned char)e.h[i];
            if (lane == 0) p[e.hl] = 0;
            p += e.hl + 1u;
            for (uint32_t c = lane; c < nc; c += 64) bam_put32(p + 4u * c, b.cig[e.rp[j].cigar_off + c]);
            p += 4u * nc;
            for (uint32_t i = lane; i < (l_seq + 1u) / 2u; i += 64) p[i] = bam_seq_byte(e, alt, l_seq, i);
            p += (l_seq + 1u) / 2u;
            if (nq) { for (uint32_t i = lane; i < l_seq; i += 64) p[i] = 0xff; }
            else { for (uint32_t i = lane; i < l_seq; i += 64) p[i] = (unsigned char)(bam_qual_at(e, alt, i) - 33); }
            p += l_seq;
            __syncthreads();
            if (lane < BAM_FIXED) dst[lane] = s_fix[lane];
            if (lane < s_n) p[lane] = s_tags[lane];
            dst += sz;
        }
    }
}
#endif
