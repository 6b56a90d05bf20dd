// dg_qc.h -- alignment QC of the coordinate-sorted BAM: the flag summary, per-chromosome counts, MAPQ, insert-size and read-length histograms and the per-cycle
// base / quality / error tables, built in HBM next to the sort (dg_bamsort.h).  After dg_bam_sort_finish the device holds the records with their flags (the
// duplicate marks of dg_bam_markdup_finish included), MAPQ and mate fields, CIGARs, 4-bit bases and quality bytes, and the reference itself as the index's 2-bit
// text: what `samtools flagstat`, `idxstats` and `stats` and Picard CollectInsertSizeMetrics compute from the file, read back and inflated, on one core.  The
// reference program has no such output: an opt-in extension, read-only on the sorted array.
//
// THE DEFINITION.  No samtools exists where this project is built and tested: this text is what the tests pin (tests/qc_inputs.py is its sequential twin).
//
// Per sorted record its fields, CIGAR, bases and qualities as bam_head of dg_bamrec.h gives them.
// All counters are u64 words in one flat array, the sections in this order; DG_QC_CYCLES = 512, DG_QC_ISIZE = 8001, DG_QC_INDEL = 65.
//   whole    36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq <= 4 + block_size, and that size <= the bytes the array holds from the record's start.
//            A record that is not whole adds 1 to SN.malformed and takes part in nothing else.  primary: flag & 0x900 == 0.  mapped: flag & 4 clear.
//   FS[2][16]  the flag summary, first index flag >> 9 & 1 (QC fail), every whole record: 0 total, 1 primary, 2 secondary (0x100), 3 supplementary (0x800 without
//            0x100), 4 duplicates (0x400), 5 primary duplicates, 6 mapped, 7 primary mapped; rows 8 .. 15 primary records with flag & 1 only: 8 paired, 9 read1
//            (0x40), 10 read2 (0x80), 11 properly paired (0x2 and mapped), 12 mapped with the mate mapped (0x8 clear), 13 singletons (mapped, 0x8 set), 14 a row-12
//            record with next_refID != refID, 15 a row-14 record with mapq >= 5.
//   CH[n_chr + 1][2]  t = refID when 0 <= refID < n_chr, else n_chr: column 0 mapped, column 1 unmapped whole records (a placed unmapped mate lands on its
//            chromosome, the rest in row n_chr).
//   MQ[256]  primary mapped records by mapq.
//   IS[3][8001]  each pair once: a primary mapped record with flag & 1 set, flag & 8 clear, flag & 0x40 set, next_refID == refID and tlen != 0; bin
//            min(|tlen|, 8000), |tlen| in 64 bits.  a = flag >> 4 & 1, b = flag >> 5 & 1: a == b is row 2 (other); else f, r = the forward and the reverse mate's
//            position ((pos, next_pos) when a is 0, (next_pos, pos) when a is 1): f <= r row 0 (inward), f > r row 1 (outward).
//   RL[2][512]  primary whole records, mapped or not, by k = flag >> 7 & 1; bin min(l_seq, 511).
//   profiled a whole record for which pu_record (dg_pileup.h) gives PU_COUNTED under the call's exclude_flags and min_mapq (defaults 0x904, 0); one that passes
//            that filter but comes out PU_LEFT_OUT or PU_RANGE adds 1 to SN.left_out, and no error is raised for it.
//   PC[2][12][512]  every stored base i of a profiled record: class k = flag >> 7 & 1, cycle c = min(s ? l_seq - 1 - i : i, 511) with s = flag >> 4 & 1 (sequencing
//            order; row 511 collects every later cycle).  Columns 0 .. 4 the base as sequenced, A C G T other: nibbles 1, 2, 4, 8 are A, C, G, T, complemented
//            when s is set; an '=' nibble inside M / = / X is the reference base, complemented when s is set; everything else ('=' inside I or S too) is other.
//            5 the quality byte (0xff adds 0); 6 aligned (the base lies in an M / = / X op); 7 mismatch: aligned, and the allele by pileup's rule (nibble 1 / 2 / 4 /
//            8 = A / C / G / T, '=' = the reference base, anything else = N) differs from d_refchar at its position; 8 inserted; 9 soft-clipped; 10 insertions: + 1
//            at the cycle of the first stored base of every I op with len > 0; 11 deletions: + 1 for every D op with len > 0 at the cycle of stored base
//            max(q, 1) - 1, q the read offset at the op.
//   ID[2][65]  profiled records: an I op of length L > 0 in [0][min(L, 64)], a D op in [1][min(L, 64)]; index 0 stays 0.
//   SN[32]   0 records, 1 malformed, 2 profiled, 3 left_out, 4 bases (the l_seq of primary whole records), 5 profiled bases, 6 aligned, 7 mismatches, 8 inserted
//            bases, 9 deleted bases (D lengths), 10 clipped, 11 N ops (len > 0, as for I and D), 12 skipped bases (N lengths), 13 bases without quality (0xff),
//            14 quality sum, 15 pairs counted in IS, 16 .. 31 zero.  (5 .. 14 over profiled records.)
// The tables are a function of the record SET: not of order, grid, batch split, ordinals, contexts or growth history.  Every word is a sum of non-negative integers,
// one term per record, base or op, and each term depends on its own record (and the reference) alone; the kernels add the terms with integer atomics, in LDS
// and in HBM, and integer sums modulo 2^64 do not depend on the order or the grouping of the additions.
// Text (qc_format, on the host, integers only): "SN\tname\tvalue", "FS\tname\tpassed\tfailed", "CH\tname\tlength\tmapped\tunmapped" (the last row `*`, length 0),
//   "MQ\tq\tn", "IS\tsize\tinward\toutward\tother", "RL\tlen\tfirst\tlast", "PC\tclass\tcycle+1\tA\tC\tG\tT\tother\tquality\taligned\tmismatch\tinserted\tclipped\t
//   insertions\tdeletions" (class: first, last), "ID\tlen\tins\tdel".  MQ, IS, RL and ID print the rows with a non-zero count, PC per class the rows up to the
//   last one with a non-zero count.  Behind the sixteen SN words four derived values, floored, 0 when the denominator is 0: error_ppm = mismatches 10^6 / aligned,
//   mean_quality_milli = quality sum 1000 / (profiled bases - bases without quality), insert_mean_milli over the IS bins below 8000 (all three rows),
//   insert_median = the smallest size whose cumulative count over all three rows reaches (pairs + 1) / 2.  Products are taken in 128 bits.
//
//   k_qc_flag   lane = sorted record: FS, MQ, RL and SN 0, 1, 4, 15 into the workgroup's LDS (u32 counters: a workgroup sees fewer than 2^32 records and adds at
//               most 1 per record to a cell; SN is 64-bit), IS straight to HBM (24003 bins: too large for LDS beside the rest, and spread thin), CH to HBM with
//               one add per distinct (chromosome, column) of a wave -- the array is sorted, a wave mostly has one.  Persistent grid, one flush at the end.
//   k_qc_cycle  a group of QC_GROUP = 16 lanes (a quarter of a wave) = sorted record, the pass that dominates: PC, ID and the rest of SN.  A lane takes
//               QC_LANE_BASES = 4 consecutive bases of a step of QC_STEP = 64: its four quality bytes and its two bytes of nibbles come out of aligned dwords,
//               funnel-shifted past the record's odd alignment as k_bs_gather does, so a group reads a step's 64 quality bytes and 32 base bytes as whole
//               lines.  The CIGAR is uniform over the group: every lane runs the same loop over the ops that reach into the step (a cursor keeps the first of
//               them from step to step) and keeps the op class and reference position of each of its bases; the reference bases are byte loads of pac,
//               neighbouring lanes neighbouring bytes.  Lane j & 15 handles op j's insertion / deletion / N terms.  The workgroup's PC table lies in LDS
//               column-major ((class x 12 + column) x 512 + cycle): a group's adds to neighbouring cycles fall into neighbouring banks.  LDS counters are
//               32-bit: between two flushes a workgroup runs QC_FLUSH_TRIPS = 32 trips of 16 records, and a record of more than QC_BIG = 16384 bases adds its
//               per-base terms straight to HBM, so a cell grows by at most 32 x 16 x 16384 x 255 = 2.14e9 < 2^32 (the quality column, by up to 255 a base; every
//               other column by 1 a base or op, 65535 ops a record at the most).  A flush adds the non-zero cells to the global words and zeroes them.
//               Persistent grid of at most QC_GROUPS workgroups (DG_QC_MAX_GROUPS caps it: a test hook).
//               Why a quarter wave and not the whole wave the duplicate marking's note asks for: the whole wave was built and measured first.  A 2x101 record
//               fills 26 of 64 lanes, and a record costs a chain of dependent fetches (its place, its fixed fields, its CIGAR, its bases and qualities, the
//               text) whatever the width; with the 48 KB table 12 waves fit a CU, so 12 records were in flight per CU and the pass ran at 7.00 ms.  Four
//               records a wave keep 48 in flight and every lane busy on reads of 64 bases or more; nothing else changed.
// Everything a lane decides is host-callable: qc_head, qc_tables, qc_op_event, qc_seek, qc_quad, qc_fetch4, qc_base (the cycle, the columns and the value of one
// base); tests/native/qc_checks.hip runs them on the CPU lane by lane.
// Measured (profiles/qc/qc_rate.json; one MI355X, 2.0 M records of 2x101 in 432 MB, device time from events, median of 10 behind 2 warm-ups, all over the same
// sorted array in the same run): k_qc_cycle 3.29 (3.28-3.30) ms = 131 GB/s of the array, against the yardstick k_md_rec (dg_markdup.h, lane = record over the same bytes)
// at 3.57 (3.54-3.65) ms = 121 GB/s: 0.92 of its time.  The whole-wave form of the same kernel, in a run of its own: 7.00 ms = 61.8 GB/s against k_md_rec at 3.65 ms, 1.92 of its time.  k_qc_flag 0.85 ms; the
// allele counts' counting walk 0.44 ms; the BGZF kernels 17.7 ms.
#ifndef DG_QC_H
#define DG_QC_H
#include "dg_pileup.h"
#include <string>
#include <vector>

#define QC_HD __host__ __device__ __forceinline__
#define QC_WG 256                    // threads per workgroup of both kernels: 256 records, or 4 waves = 4 records (dg_bam_qc_granules [0])
#define QC_LANE_BASES 4              // consecutive bases of a lane (dg_bam_qc_granules [1])
#define QC_GROUP 16                  // lanes that share a record in k_qc_cycle: a quarter of a wave (see the header: why not the whole wave)
#define QC_STEP (QC_GROUP * QC_LANE_BASES) // bases of a group's step (dg_bam_qc_granules [2])
#define QC_FLUSH_TRIPS 32            // trips of a workgroup between two flushes of its LDS tables (dg_bam_qc_granules [3])
#define QC_BIG 16384u                // a record of more bases adds its per-base terms straight to the global words (dg_bam_qc_granules [4])
#define QC_GROUPS 1024               // the largest grid
#define QC_PC_WORDS (2 * 12 * DG_QC_CYCLES)
static_assert(DG_QC_CYCLES == 512 && DG_QC_ISIZE == 8001 && DG_QC_INDEL == 65, "the definition's limits");
static_assert(64 % QC_GROUP == 0 && (unsigned long long)QC_FLUSH_TRIPS * (QC_WG / QC_GROUP) * QC_BIG * 255ull < (1ull << 32), "the quality column of the LDS table cannot wrap between two flushes");

// the sections' first words for n_chr chromosomes
QC_HD size_t qc_off_fs() { return 0; }
QC_HD size_t qc_off_ch() { return 32; }
QC_HD size_t qc_off_mq(int n_chr) { return 32 + 2 * ((size_t)n_chr + 1); }
QC_HD size_t qc_off_is(int n_chr) { return qc_off_mq(n_chr) + 256; }
QC_HD size_t qc_off_rl(int n_chr) { return qc_off_is(n_chr) + 3 * (size_t)DG_QC_ISIZE; }
QC_HD size_t qc_off_pc(int n_chr) { return qc_off_rl(n_chr) + 2 * (size_t)DG_QC_CYCLES; }
QC_HD size_t qc_off_id(int n_chr) { return qc_off_pc(n_chr) + QC_PC_WORDS; }
QC_HD size_t qc_off_sn(int n_chr) { return qc_off_id(n_chr) + 2 * (size_t)DG_QC_INDEL; }
QC_HD size_t qc_words(int n_chr) { return qc_off_sn(n_chr) + 32; }
enum { QC_SN_RECORDS = 0, QC_SN_MALFORMED, QC_SN_PROFILED, QC_SN_LEFT_OUT, QC_SN_BASES, QC_SN_PROF_BASES, QC_SN_ALIGNED, QC_SN_MISMATCH, QC_SN_INSERTED, QC_SN_DELETED, QC_SN_CLIPPED,
       QC_SN_N_OPS, QC_SN_SKIPPED, QC_SN_NOQUAL, QC_SN_QUAL_SUM, QC_SN_PAIRS };

// the fixed fields of the record that starts (with its block_size) at rec, `avail` bytes of the array behind rec
struct QcHead { bool whole; uint32_t flag, mapq, l_seq; int32_t refid, pos, next_refid, next_pos, tlen; };
QC_HD QcHead qc_head(const unsigned char *rec, uint64_t avail)
{
    const BamHead b = bam_head(rec, avail);
    QcHead h; h.flag = b.flag; h.mapq = b.mapq; h.l_seq = b.l_seq; h.refid = b.refid; h.pos = b.pos; h.next_refid = b.next_refid; h.next_pos = b.next_pos; h.tlen = b.tlen;
    h.whole = b.ok && b.aux_at <= b.block && b.aux_at <= avail;          // the computed length against the stored size and against the array
    return h;
}
QC_HD uint32_t qc_is_bin(int32_t tlen) { const int64_t t = (int64_t)tlen; const uint64_t a = (uint64_t)(t < 0 ? -t : t); return (uint32_t)(a < (uint64_t)DG_QC_ISIZE - 1 ? a : (uint64_t)DG_QC_ISIZE - 1); }
QC_HD uint32_t qc_is_row(const QcHead &h)
{
    const uint32_t a = h.flag >> 4 & 1u, b = h.flag >> 5 & 1u;
    if (a == b) return 2u;
    const int32_t f = a ? h.next_pos : h.pos, r = a ? h.pos : h.next_pos;
    return f <= r ? 0u : 1u;
}
// the per-record tables of a record (whole or not): s.sn(word, value), s.fs(fail, row), s.ch(t, column), s.mq(q), s.is(row, bin), s.rl(k, bin), one call per term
template <class S>
QC_HD void qc_tables(const QcHead &h, int n_chr, S &s)
{
    s.sn(QC_SN_RECORDS, 1);
    if (!h.whole) { s.sn(QC_SN_MALFORMED, 1); return; }
    const uint32_t fl = h.flag, fail = fl >> 9 & 1u;
    const bool primary = !(fl & 0x900u), mapped = !(fl & 4u);
    s.fs(fail, 0);
    if (primary) s.fs(fail, 1);
    if (fl & 0x100u) s.fs(fail, 2); else if (fl & 0x800u) s.fs(fail, 3);
    if (fl & 0x400u) { s.fs(fail, 4); if (primary) s.fs(fail, 5); }
    if (mapped) { s.fs(fail, 6); if (primary) s.fs(fail, 7); }
    if (primary && (fl & 1u)) {
        s.fs(fail, 8);
        if (fl & 0x40u) s.fs(fail, 9);
        if (fl & 0x80u) s.fs(fail, 10);
        if ((fl & 2u) && mapped) s.fs(fail, 11);
        if (mapped && !(fl & 8u)) { s.fs(fail, 12); if (h.next_refid != h.refid) { s.fs(fail, 14); if (h.mapq >= 5u) s.fs(fail, 15); } }
        if (mapped && (fl & 8u)) s.fs(fail, 13);
    }
    s.ch(h.refid >= 0 && h.refid < n_chr ? (uint32_t)h.refid : (uint32_t)n_chr, mapped ? 0u : 1u);
    if (primary && mapped) s.mq(h.mapq);
    if (primary && mapped && (fl & 1u) && !(fl & 8u) && (fl & 0x40u) && h.next_refid == h.refid && h.tlen != 0) { s.is(qc_is_row(h), qc_is_bin(h.tlen)); s.sn(QC_SN_PAIRS, 1); }
    if (primary) { s.rl(fl >> 7 & 1u, h.l_seq < (uint32_t)DG_QC_CYCLES - 1 ? h.l_seq : (uint32_t)DG_QC_CYCLES - 1); s.sn(QC_SN_BASES, h.l_seq); }
}

// ---- a profiled record: the per-op terms, then base by base ----
QC_HD uint32_t qc_cycle(uint32_t i, uint32_t l_seq, uint32_t s) { const uint32_t c = s ? l_seq - 1u - i : i; return c < (uint32_t)DG_QC_CYCLES - 1 ? c : (uint32_t)DG_QC_CYCLES - 1; }
QC_HD bool qc_op_takes_read(uint32_t op) { return bam_op_takes_read(op); }      // (the name tests/native/qc_checks.hip calls it by)
// op (with len) at read offset q of a profiled record of class k: s.pc(k, column, cycle, 1), s.id(row, bin), s.sn(word, value)
template <class S>
QC_HD void qc_op_event(uint32_t op, uint32_t len, uint64_t q, uint32_t l_seq, uint32_t strand, uint32_t k, S &s)
{
    if (!len) return;
    const uint32_t bin = len < (uint32_t)DG_QC_INDEL - 1 ? len : (uint32_t)DG_QC_INDEL - 1;
    if (op == 1u) { s.pc(k, 10u, qc_cycle((uint32_t)q, l_seq, strand), 1u); s.id(0u, bin); }
    else if (op == 2u) { s.pc(k, 11u, qc_cycle((uint32_t)(q > 1 ? q : 1) - 1u, l_seq, strand), 1u); s.id(1u, bin); s.sn(QC_SN_DELETED, len); }
    else if (op == 3u) { s.sn(QC_SN_N_OPS, 1); s.sn(QC_SN_SKIPPED, len); }
}
// the first op that reaches behind read offset `from`, with the read offset and reference position at which it starts: wave-uniform, carried from step to step
struct QcCursor { uint32_t j; uint64_t q, p; };
QC_HD void qc_seek(const unsigned char *rec, const PuRec &r, QcCursor &c, uint64_t from)
{
    while (c.j < r.n_ops) {
        const uint32_t w = bs_le32(rec + r.cigar_at + 4ull * c.j), op = w & 15u, len = w >> 4;
        if (bam_op_takes_read(op) && c.q + len > from) break;
        if (bam_op_takes_read(op)) c.q += len;
        if (bam_op_takes_ref(op)) c.p += len;
        c.j++;
    }
}
// the op class (0 none, 1 aligned, 2 inserted, 3 clipped) and, for an aligned base, the reference position of bases b0 .. b0 + 3; end: the step's end.
// (every array index is a constant once the loops are unrolled: the four stay in registers)
struct QcQuad { uint32_t cls[QC_LANE_BASES]; uint64_t rp[QC_LANE_BASES]; };
QC_HD void qc_quad(const unsigned char *rec, const PuRec &r, const QcCursor &c, uint64_t b0, uint64_t end, QcQuad &out)
{
#pragma unroll
    for (int k = 0; k < QC_LANE_BASES; k++) { out.cls[k] = 0u; out.rp[k] = 0; }
    uint64_t q = c.q, p = c.p;
    for (uint32_t j = c.j; j < r.n_ops && q < end; j++) {
        const uint32_t w = bs_le32(rec + r.cigar_at + 4ull * j), op = w & 15u, len = w >> 4;
        if (bam_op_takes_read(op)) {
            const uint32_t cls = op == 1u ? 2u : op == 4u ? 3u : 1u;
#pragma unroll
            for (int k = 0; k < QC_LANE_BASES; k++) {
                const uint64_t i = b0 + (uint64_t)k;
                if (i >= q && i < q + len) { out.cls[k] = cls; out.rp[k] = p + (i - q); }
            }
            q += len;
        }
        if (bam_op_takes_ref(op)) p += len;
    }
}
// four bytes from p on, low byte first.  On the device two aligned dwords, funnel-shifted (k_bs_gather's way): up to 7 bytes behind p + 3 are read, which lie in
// the sorted array's allocation (a DBuf holds 64 elements more than asked for); the host reads the `n` bytes it may and no more
QC_HD uint32_t qc_load4(const unsigned char *p, uint32_t n)
{
#ifdef __HIP_DEVICE_COMPILE__
    (void)n;
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t *a = (const uint32_t *)(p - mis);
    const uint32_t lo = a[0];
    return mis ? lo >> (8u * mis) | a[1] << (32u - 8u * mis) : lo;
#else
    uint32_t v = 0;
    for (uint32_t k = 0; k < n && k < 4u; k++) v |= (uint32_t)p[k] << (8u * k);
    return v;
#endif
}
// the lane's four bases from b0 (a multiple of 4, below l_seq) on: nib = their nibbles, base k in bits 4 k .. 4 k + 3; qual = their quality bytes, base k in byte k
QC_HD void qc_fetch4(const unsigned char *rec, const PuRec &r, uint32_t b0, uint32_t &nib, uint32_t &qual)
{
    const uint32_t left = r.l_seq - b0, n = left < 4u ? left : 4u;
    const uint32_t w = qc_load4(rec + r.seq_at + (b0 >> 1), (n + 1u) / 2u);
    nib = (w >> 4 & 15u) | (w & 15u) << 4 | (w >> 12 & 15u) << 8 | (w >> 8 & 15u) << 12;
    qual = qc_load4(rec + r.seq_at + ((uint64_t)r.l_seq + 1) / 2 + b0, n);
}
QC_HD uint32_t qc_refcode(const DIndex &ix, int32_t refid, uint64_t rp) { return (uint32_t)d_nt4((unsigned char)d_refchar(ix, ix.chr_off[refid] + (int64_t)rp)) & 3u; }
// everything about one stored base: its cycle, its base column (0 .. 4), its op column (6, 8 or 9), whether it is a mismatch, its quality term
struct QcBase { uint32_t cycle, col, op_col, mismatch, qual, noqual; };
QC_HD QcBase qc_base(uint32_t i, uint32_t l_seq, uint32_t strand, uint32_t nib, uint32_t qual, uint32_t cls, uint32_t refcode)
{
    QcBase b;
    b.cycle = qc_cycle(i, l_seq, strand);
    const bool aligned = cls == 1u, onehot = nib == 1u || nib == 2u || nib == 4u || nib == 8u;
    const uint32_t code = nib == 1u ? 0u : nib == 2u ? 1u : nib == 4u ? 2u : 3u;
    if (onehot) { b.col = strand ? 3u - code : code; b.mismatch = aligned && code != refcode ? 1u : 0u; }
    else if (nib == 0u && aligned) { b.col = strand ? 3u - refcode : refcode; b.mismatch = 0u; }
    else { b.col = 4u; b.mismatch = aligned ? 1u : 0u; }
    b.op_col = aligned ? 6u : cls == 2u ? 8u : 9u;
    b.noqual = qual == 0xffu ? 1u : 0u; b.qual = b.noqual ? 0u : qual;
    return b;
}
// what a lane keeps of its bases' SN terms
struct QcLaneSums { unsigned long long bases, aligned, mism, inserted, clipped, noqual, qsum; };
// the lane's part of a step: bases b0 .. b0 + 3 of profiled record r (class k), their terms into s.pc and sums
template <class S>
QC_HD void qc_lane_step(const unsigned char *rec, const PuRec &r, const DIndex &ix, const QcCursor &c, uint64_t b0, uint64_t end, uint32_t k, S &s, QcLaneSums &sums)
{
    if (b0 >= (uint64_t)r.l_seq) return;
    QcQuad qd;
    qc_quad(rec, r, c, b0, end, qd);
    uint32_t nib, qual;
    qc_fetch4(rec, r, (uint32_t)b0, nib, qual);
#pragma unroll
    for (int t = 0; t < QC_LANE_BASES; t++) {
        const uint64_t i = b0 + (uint64_t)t;
        if (i >= (uint64_t)r.l_seq || qd.cls[t] == 0u) continue;
        const uint32_t refcode = qd.cls[t] == 1u ? qc_refcode(ix, r.refid, qd.rp[t]) : 0u;
        const QcBase b = qc_base((uint32_t)i, r.l_seq, r.s, nib >> (4 * t) & 15u, qual >> (8 * t) & 255u, qd.cls[t], refcode);
        s.pc(k, b.col, b.cycle, 1u);
        if (b.qual) s.pc(k, 5u, b.cycle, b.qual);
        s.pc(k, b.op_col, b.cycle, 1u);
        if (b.mismatch) s.pc(k, 7u, b.cycle, 1u);
        sums.bases++; sums.qsum += b.qual; sums.noqual += b.noqual; sums.mism += b.mismatch;
        if (b.op_col == 6u) sums.aligned++; else if (b.op_col == 8u) sums.inserted++; else sums.clipped++;
    }
}

// ---- the text, on the host: integers only ----
static inline void qc_put(std::string &o, unsigned long long v) { char b[24]; int n = 0; do { b[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) o.push_back(b[--n]); }
static inline unsigned long long qc_muldiv(unsigned long long a, unsigned long long m, unsigned long long d) { return d ? (unsigned long long)((unsigned __int128)a * m / d) : 0ull; }
// names: n_chr strings, lengths: n_chr values
static inline void qc_format(const uint64_t *w, int n_chr, const char *const *names, const int64_t *lengths, std::string &o)
{
    static const char *const sn_names[16] = {"records", "malformed", "profiled", "left_out", "bases", "profiled_bases", "aligned", "mismatches", "inserted_bases", "deleted_bases", "clipped",
                                             "n_ops", "skipped_bases", "bases_without_quality", "quality_sum", "pairs"};
    static const char *const fs_names[16] = {"total", "primary", "secondary", "supplementary", "duplicates", "primary_duplicates", "mapped", "primary_mapped", "paired", "read1", "read2",
                                             "properly_paired", "with_mate_mapped", "singletons", "mate_on_other_chr", "mate_on_other_chr_mapq5"};
    const uint64_t *fs = w + qc_off_fs(), *ch = w + qc_off_ch(), *mq = w + qc_off_mq(n_chr), *is = w + qc_off_is(n_chr), *rl = w + qc_off_rl(n_chr), *pc = w + qc_off_pc(n_chr),
                   *id = w + qc_off_id(n_chr), *sn = w + qc_off_sn(n_chr);
    auto line = [&o](const char *tag, const char *name) { o += tag; o.push_back('\t'); o += name; };
    auto num = [&o](unsigned long long v) { o.push_back('\t'); qc_put(o, v); };
    for (int k = 0; k < 16; k++) { line("SN", sn_names[k]); num(sn[k]); o.push_back('\n'); }
    unsigned __int128 is_sum = 0; unsigned long long is_n = 0, median = 0, run = 0;
    const unsigned long long pairs = sn[QC_SN_PAIRS], half = pairs / 2 + (pairs & 1);
    bool found = false;
    for (int b = 0; b < DG_QC_ISIZE; b++) {
        const unsigned long long n = is[b] + is[DG_QC_ISIZE + b] + is[2 * DG_QC_ISIZE + b];
        if (b < DG_QC_ISIZE - 1) { is_sum += (unsigned __int128)n * (unsigned)b; is_n += n; }
        run += n;
        if (!found && pairs && run >= half) { median = (unsigned long long)b; found = true; }
    }
    line("SN", "error_ppm"); num(qc_muldiv(sn[QC_SN_MISMATCH], 1000000ull, sn[QC_SN_ALIGNED])); o.push_back('\n');
    line("SN", "mean_quality_milli"); num(qc_muldiv(sn[QC_SN_QUAL_SUM], 1000ull, sn[QC_SN_PROF_BASES] - sn[QC_SN_NOQUAL])); o.push_back('\n');
    line("SN", "insert_mean_milli"); num(is_n ? (unsigned long long)(is_sum * 1000u / is_n) : 0ull); o.push_back('\n');
    line("SN", "insert_median"); num(median); o.push_back('\n');
    for (int k = 0; k < 16; k++) { line("FS", fs_names[k]); num(fs[k]); num(fs[16 + k]); o.push_back('\n'); }
    for (int t = 0; t <= n_chr; t++) { line("CH", t < n_chr ? names[t] : "*"); num(t < n_chr ? (unsigned long long)lengths[t] : 0ull); num(ch[2 * t]); num(ch[2 * t + 1]); o.push_back('\n'); }
    for (int q = 0; q < 256; q++) if (mq[q]) { o += "MQ"; num((unsigned)q); num(mq[q]); o.push_back('\n'); }
    for (int b = 0; b < DG_QC_ISIZE; b++)
        if (is[b] | is[DG_QC_ISIZE + b] | is[2 * DG_QC_ISIZE + b]) { o += "IS"; num((unsigned)b); num(is[b]); num(is[DG_QC_ISIZE + b]); num(is[2 * DG_QC_ISIZE + b]); o.push_back('\n'); }
    for (int b = 0; b < DG_QC_CYCLES; b++) if (rl[b] | rl[DG_QC_CYCLES + b]) { o += "RL"; num((unsigned)b); num(rl[b]); num(rl[DG_QC_CYCLES + b]); o.push_back('\n'); }
    for (int k = 0; k < 2; k++) {
        int last = -1;
        for (int c = 0; c < DG_QC_CYCLES; c++) for (int col = 0; col < 12; col++) if (pc[((size_t)k * 12 + col) * DG_QC_CYCLES + c]) last = c;
        for (int c = 0; c <= last; c++) {
            line("PC", k ? "last" : "first"); num((unsigned)c + 1u);
            for (int col = 0; col < 12; col++) num(pc[((size_t)k * 12 + col) * DG_QC_CYCLES + c]);
            o.push_back('\n');
        }
    }
    for (int b = 0; b < DG_QC_INDEL; b++) if (id[b] | id[DG_QC_INDEL + b]) { o += "ID"; num((unsigned)b); num(id[b]); num(id[DG_QC_INDEL + b]); o.push_back('\n'); }
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
struct QcFlagSink {                 // k_qc_flag's: LDS for the small tables, HBM for IS; the CH term is kept for the wave's joint add
    uint32_t *fs_, *mq_, *rl_; unsigned long long *sn_, *is_; uint32_t ch_key;
    __device__ __forceinline__ void sn(uint32_t w, unsigned long long v) { atomicAdd(&sn_[w], v); }
    __device__ __forceinline__ void fs(uint32_t fail, uint32_t row) { atomicAdd(&fs_[fail * 16u + row], 1u); }
    __device__ __forceinline__ void ch(uint32_t t, uint32_t col) { ch_key = 2u * t + col; }
    __device__ __forceinline__ void mq(uint32_t q) { atomicAdd(&mq_[q], 1u); }
    __device__ __forceinline__ void is(uint32_t row, uint32_t bin) { atomicAdd(&is_[(size_t)row * DG_QC_ISIZE + bin], 1ull); }
    __device__ __forceinline__ void rl(uint32_t k, uint32_t bin) { atomicAdd(&rl_[k * (uint32_t)DG_QC_CYCLES + bin], 1u); }
};
// the workgroup's non-zero LDS cells to the global words, and zeroed (between two barriers of the caller's)
template <typename T>
__device__ __forceinline__ void qc_flush(T *lds, uint32_t n, unsigned long long *out)
{
    for (uint32_t k = threadIdx.x; k < n; k += QC_WG) { const T v = lds[k]; if (v) { atomicAdd(&out[k], (unsigned long long)v); lds[k] = 0; } }
}

__global__ void __launch_bounds__(QC_WG)
k_qc_flag(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, int n_chr,
          unsigned long long *__restrict__ words)
{
    __shared__ uint32_t s_fs[32], s_mq[256], s_rl[2 * DG_QC_CYCLES];
    __shared__ unsigned long long s_sn[32];
    for (uint32_t k = threadIdx.x; k < 2 * DG_QC_CYCLES; k += QC_WG) { s_rl[k] = 0; if (k < 256) s_mq[k] = 0; if (k < 32) { s_fs[k] = 0; s_sn[k] = 0; } }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * QC_WG; base < n; base += (uint64_t)gridDim.x * QC_WG) {
        const uint64_t i = base + threadIdx.x;
        QcFlagSink s{s_fs, s_mq, s_rl, s_sn, words + qc_off_is(n_chr), 0xFFFFFFFFu};
        if (i < n) {
            const uint64_t at = bam_rec_start(dst_off, tile_base, (uint32_t)i);
            QcHead h = qc_head(sorted + (at < n_raw ? at : 0), at < n_raw ? n_raw - at : 0);
            qc_tables(h, n_chr, s);
        }
        // one add per distinct (chromosome, column) of the wave (every lane is here)
        for (unsigned long long left = __ballot(s.ch_key != 0xFFFFFFFFu); left;) {
            const int l = __ffsll(left) - 1;
            const uint32_t key = __shfl(s.ch_key, l, 64);
            const unsigned long long same = __ballot(s.ch_key == key);
            if ((int)lane == l) atomicAdd(&words[qc_off_ch() + key], (unsigned long long)__popcll(same));
            left &= ~same;
        }
    }
    __syncthreads();
    qc_flush(s_fs, 32u, words + qc_off_fs());
    qc_flush(s_mq, 256u, words + qc_off_mq(n_chr));
    qc_flush(s_rl, 2u * DG_QC_CYCLES, words + qc_off_rl(n_chr));
    qc_flush(s_sn, 32u, words + qc_off_sn(n_chr));
}

struct QcCycleSink {                // k_qc_cycle's: the workgroup's LDS tables; direct: the per-base terms of a record of more than QC_BIG bases go to the global words
    uint32_t *pc_, *id_; unsigned long long *sn_, *gpc; bool direct;
    __device__ __forceinline__ void pc(uint32_t k, uint32_t col, uint32_t cycle, uint32_t v)
    {
        const uint32_t at = (k * 12u + col) * (uint32_t)DG_QC_CYCLES + cycle;
        if (direct) atomicAdd(&gpc[at], (unsigned long long)v); else atomicAdd(&pc_[at], v);
    }
    __device__ __forceinline__ void id(uint32_t row, uint32_t bin) { atomicAdd(&id_[row * (uint32_t)DG_QC_INDEL + bin], 1u); }
    __device__ __forceinline__ void sn(uint32_t w, unsigned long long v) { atomicAdd(&sn_[w], v); }
};

__global__ void __launch_bounds__(QC_WG)
k_qc_cycle(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, const DIndex ix,
           const PuFilter f, unsigned long long *__restrict__ words)
{
    __shared__ uint32_t s_pc[QC_PC_WORDS], s_id[2 * DG_QC_INDEL];
    __shared__ unsigned long long s_sn[32];
    for (uint32_t k = threadIdx.x; k < QC_PC_WORDS; k += QC_WG) { s_pc[k] = 0; if (k < 2 * DG_QC_INDEL) s_id[k] = 0; if (k < 32) s_sn[k] = 0; }
    __syncthreads();
    const uint32_t lane = threadIdx.x & (QC_GROUP - 1u), grp = threadIdx.x / QC_GROUP;
    unsigned long long *gpc = words + qc_off_pc(ix.n_chr), *gid = words + qc_off_id(ix.n_chr), *gsn = words + qc_off_sn(ix.n_chr);
    QcLaneSums sums{0, 0, 0, 0, 0, 0, 0};
    uint32_t trips = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * (QC_WG / QC_GROUP); base < n; base += (uint64_t)gridDim.x * (QC_WG / QC_GROUP)) {
        const uint64_t i = base + grp;
        const uint64_t at = i < n ? bam_rec_start(dst_off, tile_base, (uint32_t)i) : n_raw;
        if (at < n_raw) {
            const unsigned char *rec = sorted + at;
            const QcHead h = qc_head(rec, n_raw - at);
            if (h.whole) {
                const PuRec r = pu_record(rec, n_raw - at, ix, f);
                QcCycleSink s{s_pc, s_id, s_sn, gpc, r.l_seq > QC_BIG};
                if ((r.state == PU_LEFT_OUT || r.state == PU_RANGE) && lane == 0u) s.sn(QC_SN_LEFT_OUT, 1);
                if (r.state == PU_COUNTED) {
                    const uint32_t k = h.flag >> 7 & 1u;
                    if (lane == 0u) s.sn(QC_SN_PROFILED, 1);
                    uint32_t j = 0;                                   // op j's terms are lane j & 15's
                    bam_cigar_walk(rec, r.cigar_at, r.n_ops, 0, [&](uint32_t op, uint32_t len, uint64_t, uint64_t q) {
                        if ((j++ & (QC_GROUP - 1u)) == lane) qc_op_event(op, len, q, r.l_seq, r.s, k, s);
                    });
                    QcCursor c{0u, 0ull, (uint64_t)r.pos};
                    for (uint64_t b = 0; b < (uint64_t)r.l_seq; b += QC_STEP) {
                        qc_seek(rec, r, c, b);
                        const uint64_t end = b + QC_STEP < (uint64_t)r.l_seq ? b + QC_STEP : (uint64_t)r.l_seq;
                        qc_lane_step(rec, r, ix, c, b + (uint64_t)lane * QC_LANE_BASES, end, k, s, sums);
                    }
                }
            }
        }
        if (++trips == QC_FLUSH_TRIPS) {          // (base, and with it the number of trips, is the same for all of the workgroup's groups)
            trips = 0;
            __syncthreads();
            qc_flush(s_pc, (uint32_t)QC_PC_WORDS, gpc);
            qc_flush(s_id, 2u * DG_QC_INDEL, gid);
            __syncthreads();
        }
    }
    if (sums.bases) atomicAdd(&s_sn[QC_SN_PROF_BASES], sums.bases);
    if (sums.aligned) atomicAdd(&s_sn[QC_SN_ALIGNED], sums.aligned);
    if (sums.mism) atomicAdd(&s_sn[QC_SN_MISMATCH], sums.mism);
    if (sums.inserted) atomicAdd(&s_sn[QC_SN_INSERTED], sums.inserted);
    if (sums.clipped) atomicAdd(&s_sn[QC_SN_CLIPPED], sums.clipped);
    if (sums.noqual) atomicAdd(&s_sn[QC_SN_NOQUAL], sums.noqual);
    if (sums.qsum) atomicAdd(&s_sn[QC_SN_QUAL_SUM], sums.qsum);
    __syncthreads();
    qc_flush(s_pc, (uint32_t)QC_PC_WORDS, gpc);
    qc_flush(s_id, 2u * DG_QC_INDEL, gid);
    qc_flush(s_sn, 32u, gsn);
}
#endif
#endif
