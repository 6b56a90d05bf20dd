// dg_bamrec.h -- the one reader of a BAM record in HBM, under every stage that reads records: the sort store (dg_bamsort.h), the index (dg_bamidx.h), coverage
// (dg_coverage.h), duplicate marking (dg_markdup.h), allele counts (dg_pileup.h), QC (dg_qc.h) and tags (dg_tags.h).  It knows the layout (SAM specification
// 4.2) and nothing of any stage: which records count, and what becomes of one that does not, is the stage's own policy over a BamHead.
//
// A record starts with block_size (u32); records are not aligned, so every field is read byte by byte, little endian:
//   refID i32 at 4, pos i32 at 8, l_read_name u8 at 12, mapq u8 at 13, bin u16 at 14 (never read: the index recomputes it), n_cigar_op u16 at 16, flag u16 at
//   18, l_seq u32 at 20, next_refID i32 at 24, next_pos i32 at 28, tlen i32 at 32; behind these BAM_FIXED = 36 bytes the name (l_read_name bytes with its NUL),
//   the CIGAR ops (u32: len << 4 | op), (l_seq + 1) / 2 bytes of packed bases (base i: the high nibble of its byte for even i), l_seq quality bytes, the aux area.
// bam_head is the only place that names a byte offset of the fixed part for reading.  Everything here is host-callable (tests/native/bamrec_checks.hip).
#ifndef DG_BAMREC_H
#define DG_BAMREC_H
#include "dg_bamfmt.h"

#define BR_HD __host__ __device__ __forceinline__
#define BS_THREADS 256           // records per workgroup of k_bs_len, whose scanned lengths place the sorted records (dg_bam_sort_granules [0])

BR_HD uint32_t bs_le32(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// The fixed fields of the record that starts (with its block_size) at rec, `avail` bytes of the array behind rec.  ok: avail >= BAM_FIXED; when it is false
// nothing is read and every field keeps the value below.  The offsets are 64 bit: no field of a damaged record makes them wrap.
//   size against the stages: coverage and the allele counts want cigar_at + 4 n_cigar resp. qual_at inside `size`, the marking aux_at; the index cuts the ops to
//   what fits in `size` and refuses nothing; QC's `whole` compares aux_at with `block` and with avail; the tags refuse block > avail; the sort key checks nothing.
struct BamHead {
    bool ok;
    int32_t refid, pos, next_refid, next_pos, tlen;
    uint32_t l_name, mapq, n_cigar, flag, l_seq;
    uint64_t block /* 4 + block_size, as stored */, size /* the bytes of the record that lie inside the array: block, at most avail */;
    uint64_t cigar_at, seq_at, qual_at, aux_at;
};
BR_HD BamHead bam_head(const unsigned char *rec, uint64_t avail)
{
    BamHead h; h.ok = avail >= BAM_FIXED;
    h.refid = -1; h.pos = -1; h.next_refid = -1; h.next_pos = -1; h.tlen = 0; h.l_name = 0; h.mapq = 0; h.n_cigar = 0; h.flag = 0; h.l_seq = 0;
    h.block = 0; h.size = 0; h.cigar_at = 0; h.seq_at = 0; h.qual_at = 0; h.aux_at = 0;
    if (!h.ok) return h;
    h.block = 4ull + (uint64_t)bs_le32(rec); h.size = h.block < avail ? h.block : avail;
    h.refid = (int32_t)bs_le32(rec + 4); h.pos = (int32_t)bs_le32(rec + 8);
    h.l_name = rec[12]; h.mapq = rec[13]; h.n_cigar = (uint32_t)rec[16] | (uint32_t)rec[17] << 8; h.flag = (uint32_t)rec[18] | (uint32_t)rec[19] << 8;
    h.l_seq = bs_le32(rec + 20);
    h.next_refid = (int32_t)bs_le32(rec + 24); h.next_pos = (int32_t)bs_le32(rec + 28); h.tlen = (int32_t)bs_le32(rec + 32);
    h.cigar_at = (uint64_t)BAM_FIXED + h.l_name; h.seq_at = h.cigar_at + 4ull * h.n_cigar;
    h.qual_at = h.seq_at + ((uint64_t)h.l_seq + 1) / 2; h.aux_at = h.qual_at + (uint64_t)h.l_seq;
    return h;
}

// ---- the CIGAR: M I D N S H P = X are ops 0 .. 8 ----
BR_HD bool bam_op_aligned(uint32_t op) { return op == 0u || op == 7u || op == 8u; }                                  // M, =, X: read and reference
BR_HD bool bam_op_takes_ref(uint32_t op) { return bam_op_aligned(op) || op == 2u || op == 3u; }                      // and D, N
BR_HD bool bam_op_takes_read(uint32_t op) { return bam_op_aligned(op) || op == 1u || op == 4u; }                     // and I, S
// The walk over n_ops ops at rec + cigar_at (the caller has seen that they lie inside the record): f(op, len, p, q) for each, p the reference position and q
// the read offset in front of the op; returns both behind the last op.  Started at pos = 0, p is the reference length.
struct BamAt { uint64_t p, q; };
template <class F>
BR_HD BamAt bam_cigar_walk(const unsigned char *rec, uint64_t cigar_at, uint64_t n_ops, uint64_t pos, F f)
{
    BamAt a; a.p = pos; a.q = 0;
    for (uint64_t j = 0; j < n_ops; j++) {
        const uint32_t c = bs_le32(rec + cigar_at + 4ull * j), op = c & 15u, len = c >> 4;
        f(op, len, a.p, a.q);
        if (bam_op_takes_ref(op)) a.p += len;
        if (bam_op_takes_read(op)) a.q += len;
    }
    return a;
}
struct BamNoOp { BR_HD void operator()(uint32_t, uint32_t, uint64_t, uint64_t) const {} };

// where sorted record i starts in the array: k_bs_len's offsets and the scanned per-tile sums
BR_HD uint64_t bam_rec_start(const uint64_t *dst_off, const uint64_t *tile_base, uint32_t i) { return tile_base[i / BS_THREADS] + dst_off[i]; }
#endif
