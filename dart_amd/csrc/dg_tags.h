// dg_tags.h -- MD, NM and ts on the records of the coordinate-sorted BAM: what `samtools calmd` writes into a finished file -- read back, inflated, one core,
// deflated again -- written in HBM behind dg_bam_sort_finish (and the duplicate marks) and in front of the first dg_bam_sort_compress.  The device holds the
// records with their 4-bit bases and CIGARs and the reference as the index's 2-bit text; dg_pileup.h has the sixteen-bases-a-step comparison.  This is the one
// stage that changes the records' SIZES behind the sort: per record a new length, a scan, a rewrite into a second array, and every later stage (marking,
// compression, index, coverage, allele counts, QC) is handed the new array in the shape dg_bam_sort_finish leaves.  The reference program has no such output: an
// opt-in extension.
//
// THE DEFINITION.  No samtools exists where this project is built and tested: this text is what the tests pin (tests/tags_inputs.py is its sequential twin).
//
// flags: DG_TAG_MD | DG_TAG_NM | DG_TAG_TS, at least one.  The new array holds the same records in the same order; each is copied byte for byte or rewritten.
//   eligible  pu_record of dg_pileup.h with exclude = 0, min_mapq = 0 gives PU_COUNTED (0 <= refID < n_chr; pos >= 0; flag & 4 clear; n_cigar_op > 0; the CIGAR
//             and the packed bases inside the record and the array; l_seq > 0; the CIGAR's read length == l_seq; pos + rlen <= chr_len[refID]), and: block_size
//             + 4 bytes lie inside the array, and the qualities inside the record: aux_at = 36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size
//             + 4.  Every other record -- a PU_RANGE one too -- is copied verbatim (stats[1]); the call does not fail on it.
//   aux walk  the aux area is [aux_at, block_size + 4): a sequence of tag[2] type value.  A c C: 1 byte.  s S: 2.  i I f: 4.  Z H: up to and including a NUL.
//             B: a subtype (c C s S i I f), a u32 count, count x the subtype's width.  An unknown type or subtype, fewer than three bytes left, or a value that
//             runs past the record's end: the aux area is unreadable and the record is copied verbatim (stats[2]).
//   new aux   the old one without every tag named MD, NM or ts WHOSE FLAG BIT IS SET (whatever its type; stats[3] counts them; one of those names whose bit
//             is clear stays where it is), then NM, MD, ts appended in that order, each only when selected.  What calmd leaves: delete, then append.
//   match     the pileup's rule: a read nibble matches the reference's 2-bit code r when it is 0 ('=') or equals 1 << r; every other nibble (N, IUPAC) is a
//             mismatch.  The op (M, = or X) plays no part.  The reference letter is "ACGT"[r]: what the index's text holds, so an N of the FASTA is whatever
//             base the indexer stored there.
//   MD        p = pos, run u = 0.  M, =, X: per base, a match is u++; a mismatch prints u in decimal, then the reference letter, u = 0.  D of length L > 0:
//             prints u, '^', the L reference letters, u = 0; p += L.  I, S: read bases only.  N: p += L.  H, P: nothing.  At the end u is printed.  So "A0C",
//             "10^AC0T5" and a leading "0" come out as htslib prints them.  The tag: 'M' 'D' 'Z', the text, NUL.
//   NM        mismatches + the sum of the I lengths + the sum of the D lengths: edit distance, as the SAM specification has it (the mapper's NM:i is its count
//             of mismatches).  The tag: 'N' 'M', then the smallest unsigned type: 'C' below 256, 'S' below 65536, else 'I' (bam_put_tag's rule).
//   ts        every N op of length L >= 4 at [p, p + L) is an intron: text[p], text[p + 1] .. text[p + L - 2], text[p + L - 1] of the FORWARD text.  GT..AG
//             and GC..AG vote '+', CT..AC and CT..GC vote '-' (the reference program's SpliceJunctionArr); anything else does not vote.  All votes equal and
//             at least one: the genomic strand g.  The tag: 't' 's' 'A', then g when flag & 16 is clear and the opposite sign when it is set -- minimap2's
//             convention: the transcript's strand RELATIVE TO THE READ AS ALIGNED.  XS:A is not used: a record holds a tag name once, and XS:i (the
//             sub-optimal score) has that name.  A rewritten record with at least one intron and no tag is tallied in stats[7]: no vote in the low word, votes
//             that disagree in the high word.  Without DG_TAG_TS stats[6] and stats[7] are 0.
//   fields    block_size is rewritten; no other fixed field changes (bin does not depend on tags).
//   stats     [0] records rewritten  [1] copied verbatim, not eligible  [2] copied verbatim, aux unreadable  [3] old tags removed  [4] mismatches and [5]
//             inserted + deleted bases of the rewritten records  [6] ts written  [7] introns without ts: no motif | conflict << 32
// The same records and flags give the same bytes whatever the grid, the batch split, the contexts or the growth history: a record's new bytes are a function of
// its old bytes and the text; its place follows from the scanned lengths.  A second call with the same flags removes what the first appended and appends the same
// again: the same bytes.  No kernel here uses an atomic.
//
// ONE walk (tg_walk) prints MD into one sink, TgPut, which counts when its capacity is 0 and stores when it has one, so the length a record was given and the bytes it gets agree by
// construction.  Runs of matches come out of the step's mismatch mask by bit scans (MD's size depends on the decimal digits of every run, not on a popcount).
//
//   k_tg_len     lane = sorted record: eligibility, the aux walk, the counting walk; the record's new size; the workgroup's exclusive scan and sum in the shape
//                k_bs_len leaves (k_cv_top scans the sums and adds up the counters' planes)
//   -- the one wait: the new array's size --
//   the write pass, two kernels that store disjoint bytes of every record:
//   k_tg_tail    lane = record: the same walk again, storing NM, MD, ts and block_size (a walk is a chain of dependent steps over one record: only a lane per
//                record keeps every lane of a wave walking, as in the length pass)
//   k_tg_copy    TG_LANES lanes = record: they copy the bytes that stay (the fixed fields to the qualities, the kept runs of the aux area; source and
//                destination unaligned: k_bs_gather's funnel shift)
// Memory: the new array and 8 bytes per record.  Everything a lane computes is host-callable: tests/native/tags_checks.hip runs it on the CPU.
#ifndef DG_TAGS_H
#define DG_TAGS_H
#include "dg_pileup.h"

#define TG_HD __host__ __device__ __forceinline__
#define TG_WG PU_WG                  // records per workgroup of k_tg_len (dg_bam_tags_granules [0])
#define TG_LANES 16                  // lanes per record of k_tg_copy (dg_bam_tags_granules [1])
#define TG_ALL (DG_TAG_MD | DG_TAG_NM | DG_TAG_TS)
static_assert(TG_WG == BS_THREADS, "k_tg_len leaves k_bs_len's per-workgroup offsets, and the tagged array is handed on in that shape");
static_assert(TG_WG % TG_LANES == 0, "whole records per workgroup of k_tg_copy");
// the call's small device state, 64-bit words: k_cv_top's outputs lie side by side
enum { TG_ST_BYTES = 0, TG_ST_RECS /* rewritten | not eligible << 32 */, TG_ST_AUX_TS /* aux unreadable | ts written << 32 */, TG_ST_REMOVED, TG_ST_MISM, TG_ST_INDEL, TG_ST_JUNK,
       TG_ST_NO_TS /* no motif | conflict << 32 */, TG_ST_WORDS = 8 };
enum { TG_REWRITE = 0, TG_NOT_ELIGIBLE, TG_AUX_BAD };

// ---- the aux area ----
TG_HD uint32_t tg_b_width(uint32_t sub) { return sub == 'c' || sub == 'C' ? 1u : sub == 's' || sub == 'S' ? 2u : sub == 'i' || sub == 'I' || sub == 'f' ? 4u : 0u; }
// the tag at rec + a of a record of `size` bytes: its bytes with name and type, 0: unreadable
TG_HD uint64_t tg_aux_len(const unsigned char *rec, uint64_t a, uint64_t size)
{
    if (a + 3 > size) return 0;
    const uint32_t ty = rec[a + 2];
    const uint64_t v = a + 3;
    uint64_t len;
    if (ty == 'A' || ty == 'c' || ty == 'C') len = 1;
    else if (ty == 's' || ty == 'S') len = 2;
    else if (ty == 'i' || ty == 'I' || ty == 'f') len = 4;
    else if (ty == 'Z' || ty == 'H') {
        uint64_t e = v;
        while (e < size && rec[e]) e++;
        if (e >= size) return 0;
        len = e - v + 1;
    } else if (ty == 'B') {
        if (v + 5 > size) return 0;
        const uint32_t w = tg_b_width(rec[v]);
        if (!w) return 0;
        len = 5ull + (uint64_t)w * bs_le32(rec + v + 1);
    } else return 0;
    return v + len <= size ? 3 + len : 0;
}
TG_HD bool tg_aux_goes(const unsigned char *tag, uint32_t flags)
{
    return ((flags & DG_TAG_MD) && tag[0] == 'M' && tag[1] == 'D') || ((flags & DG_TAG_NM) && tag[0] == 'N' && tag[1] == 'M') || ((flags & DG_TAG_TS) && tag[0] == 't' && tag[1] == 's');
}
// the walk over [aux_at, size): f.run(at, len) for every maximal run of bytes that stay, in order; false: unreadable (runs may have been handed out before)
template <class F>
TG_HD bool tg_aux_walk(const unsigned char *rec, uint64_t aux_at, uint64_t size, uint32_t flags, F &f)
{
    uint64_t a = aux_at, run_at = aux_at;
    while (a < size) {
        const uint64_t len = tg_aux_len(rec, a, size);
        if (!len) return false;
        if (tg_aux_goes(rec + a, flags)) { if (a > run_at) f.run(run_at, a - run_at); f.gone(); run_at = a + len; }
        a += len;
    }
    if (a > run_at) f.run(run_at, a - run_at);
    return true;
}
struct TgAuxCount { uint64_t kept; uint32_t removed; TG_HD void run(uint64_t, uint64_t len) { kept += len; } TG_HD void gone() { removed++; } };

// what becomes of the record that starts (with its block_size) at rec, `avail` bytes of the array behind rec
struct TgPlan { int kind; PuRec r; uint64_t size /* the record's bytes inside the array */, aux_at, kept /* aux bytes that stay */; uint32_t removed; };
TG_HD TgPlan tg_plan(const unsigned char *rec, uint64_t avail, const DIndex &ix, uint32_t flags)
{
    TgPlan p; p.kind = TG_NOT_ELIGIBLE; p.aux_at = 0; p.kept = 0; p.removed = 0;
    const BamHead h = bam_head(rec, avail);
    const uint64_t whole = avail >= 4 ? 4ull + (uint64_t)bs_le32(rec) : ~0ull;      // (of a record whose fixed part is cut short too: it is copied as far as it goes)
    p.size = whole <= avail ? whole : avail;
    const PuFilter all{0u, 0u};
    p.r = pu_record(rec, h, ix, all);
    if (whole > avail || p.r.state != PU_COUNTED) return p;                        // refused when block_size passes the array's end, not clamped
    p.aux_at = h.aux_at;
    if (p.aux_at > p.size) return p;
    TgAuxCount c{0, 0};
    if (!tg_aux_walk(rec, p.aux_at, p.size, flags, c)) { p.kind = TG_AUX_BAD; return p; }
    p.kind = TG_REWRITE; p.kept = c.kept; p.removed = c.removed;
    return p;
}

// ---- the appended tags ----
// bytes go to p[n] while n < cap; cap == 0 counts
struct TgPut {
    unsigned char *p; uint64_t n, cap; bool on;
    TG_HD void ch(uint32_t c) { if (on) { if (n < cap) p[n] = (unsigned char)c; n++; } }
};
TG_HD void tg_num(TgPut &o, uint32_t u)      // (a run is at most l_seq: 32 bits, and no 64-bit division on the device)
{
    uint32_t d = 1;
    while (u / d >= 10u) d *= 10u;
    for (; d; d /= 10u) o.ch('0' + u / d % 10u);
}
TG_HD uint32_t tg_letter(uint32_t code) { return 0x54474341u >> (8u * (code & 3u)) & 0xFFu; }
TG_HD uint32_t tg_text(const DIndex &ix, int64_t g) { return (uint32_t)d_nt4((unsigned char)d_refchar(ix, g)) & 3u; }
// an intron's vote: 1 '+', 2 '-', 0 none.  a, b: the codes of its first two bases, c, d: of its last two (A C G T = 0 1 2 3)
TG_HD uint32_t tg_motif(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t m = a << 6 | b << 4 | c << 2 | d;
    if (m == (2u << 6 | 3u << 4 | 0u << 2 | 2u) || m == (2u << 6 | 1u << 4 | 0u << 2 | 2u)) return 1u;      // GT..AG, GC..AG
    if (m == (1u << 6 | 3u << 4 | 0u << 2 | 1u) || m == (1u << 6 | 3u << 4 | 2u << 2 | 1u)) return 2u;      // CT..AC, CT..GC
    return 0u;
}
struct TgTally { uint64_t mism, ins, del; uint32_t votes /* bit 0: a '+', bit 1: a '-' */, introns; };
// The walk of a rewritten record: MD's text (without name, type and NUL) into o; what NM and ts need comes back.
TG_HD TgTally tg_walk(const unsigned char *rec, const PuRec &r, const DIndex &ix, TgPut &o)
{
    TgTally t; t.mism = 0; t.ins = 0; t.del = 0; t.votes = 0; t.introns = 0;
    const unsigned char *seq = rec + r.seq_at;
    const int64_t g0 = ix.chr_off[r.refid];
    uint32_t u = 0;
    bam_cigar_walk(rec, r.cigar_at, r.n_ops, (uint64_t)r.pos, [&](uint32_t op, uint32_t len, uint64_t p, uint64_t q) {
        if (bam_op_aligned(op)) {
            for (uint32_t k = 0; k < len; k += PU_STEP) {
                const uint32_t n = len - k < PU_STEP ? len - k : PU_STEP, ref = pu_ref16(ix, g0 + (int64_t)(p + k));
                const PuStep st = pu_compare16(pu_nibbles16(seq, r.l_seq, (uint32_t)q + k), ref, n);
                uint32_t prev = 0;
                for (uint32_t m = st.mis; m;) {
                    const uint32_t z = pu_clz(m), b = z >> 1;                    // base b of the step: bit 30 - 2 b
                    m &= ~(0x80000000u >> z);
                    tg_num(o, u + (b - prev)); o.ch(tg_letter(ref >> (30u - 2u * b)));
                    u = 0; prev = b + 1u; t.mism++;
                }
                u += n - prev;
            }
        } else if (op == 2u && len) {
            tg_num(o, u); o.ch('^');
            for (uint32_t i = 0; i < len; i++) o.ch(tg_letter(tg_text(ix, g0 + (int64_t)(p + i))));
            u = 0; t.del += len;
        } else if (op == 3u && len >= 4u) {
            const int64_t g = g0 + (int64_t)p;
            const uint32_t v = tg_motif(tg_text(ix, g), tg_text(ix, g + 1), tg_text(ix, g + (int64_t)len - 2), tg_text(ix, g + (int64_t)len - 1));
            t.votes |= v; t.introns++;
        } else if (op == 1u) t.ins += len;
    });
    tg_num(o, u);
    return t;
}
TG_HD uint32_t tg_nm_width(uint64_t nm) { return nm < 256u ? 1u : nm < 65536u ? 2u : 4u; }
// NM, MD, ts of a rewritten record at p (at most cap bytes are stored; cap == 0: sizes only)
struct TgTail { uint64_t bytes, nm, mism, indel; uint32_t ts /* 0, '+', '-' */, no_motif, conflict; };
TG_HD TgTail tg_tail(const unsigned char *rec, const PuRec &r, const DIndex &ix, uint32_t flags, unsigned char *p, uint64_t cap)
{
    const bool md = (flags & DG_TAG_MD) != 0u, nm_on = (flags & DG_TAG_NM) != 0u;
    TgTail out; TgTally t; TgPut o{p, 0, cap, true};
    uint32_t w = 1u;                                   // NM's width is known behind the walk that prints MD behind it: almost always one byte; else once more
    for (;;) {
        o.n = nm_on ? 3ull + w : 0ull; o.on = md;
        o.ch('M'); o.ch('D'); o.ch('Z');
        t = tg_walk(rec, r, ix, o);
        o.ch(0u);
        out.nm = t.mism + t.ins + t.del;
        const uint32_t need = tg_nm_width(out.nm);
        if (!nm_on || need == w) break;
        if (!md || cap == 0) { o.n += need - w; w = need; break; }
        w = need;
    }
    o.on = true;
    if (nm_on) {
        TgPut h{p, 0, cap, true};
        h.ch('N'); h.ch('M'); h.ch(w == 1u ? 'C' : w == 2u ? 'S' : 'I');
        for (uint32_t i = 0; i < w; i++) h.ch((uint32_t)(out.nm >> (8u * i)) & 0xFFu);
    }
    out.ts = 0; out.no_motif = 0; out.conflict = 0;
    if (flags & DG_TAG_TS) {
        if (t.votes == 1u || t.votes == 2u) {
            out.ts = ((t.votes == 1u) != (r.s != 0u)) ? '+' : '-';
            o.ch('t'); o.ch('s'); o.ch('A'); o.ch(out.ts);
        } else if (t.introns) { if (t.votes) out.conflict = 1; else out.no_motif = 1; }
    }
    out.bytes = o.n; out.mism = t.mism; out.indel = t.ins + t.del;
    return out;
}

// ---- the copy of the bytes that stay ----
// lane `lane` of TG_LANES: its part of len bytes from s to d, both unaligned.  On the device k_bs_gather's way: the destination is brought to a dword boundary
// with single bytes, then one aligned dword per lane and trip, funnel-shifted from two aligned dwords of the source (up to 3 bytes behind s + len are read:
// they lie in the sorted array's allocation, which is padded); the last 0..3 bytes go singly.  The host copies the same bytes one by one.
TG_HD void tg_copy(unsigned char *d, const unsigned char *s, uint64_t len, uint32_t lane)
{
#ifdef __HIP_DEVICE_COMPILE__
    uint64_t head = (4u - (uint32_t)((uintptr_t)d & 3u)) & 3u;
    if (head > len) head = len;
    if (lane < head) d[lane] = s[lane];
    s += head; d += head;
    const uint64_t rem = len - head, nd = rem >> 2;
    const uint32_t tail = (uint32_t)rem & 3u, mis = (uint32_t)((uintptr_t)s & 3u), sh = mis * 8u;
    const uint32_t *sa = (const uint32_t *)(s - mis);
    uint32_t *da = (uint32_t *)d;
    if (sh == 0) { for (uint64_t j = lane; j < nd; j += TG_LANES) da[j] = sa[j]; }
    else { for (uint64_t j = lane; j < nd; j += TG_LANES) da[j] = sa[j] >> sh | sa[j + 1] << (32u - sh); }
    if (lane < tail) d[4u * nd + lane] = s[4u * nd + lane];
#else
    for (uint64_t j = lane; j < len; j += TG_LANES) d[j] = s[j];
#endif
}
struct TgAuxCopy {                   // k_tg_copy's aux walk: every run that stays goes behind the last one
    unsigned char *dst; const unsigned char *rec; uint64_t n, cap; uint32_t lane;
    TG_HD void run(uint64_t at, uint64_t len) { if (n + len <= cap) tg_copy(dst + n, rec + at, len, lane); n += len; }
    TG_HD void gone() {}
};
// The record at rec in the new array, in two parts that store disjoint bytes: dst is the record's place, cap the bytes of the array from there on.
// tg_write_new: what ONE lane stores of a rewritten record -- NM, MD, ts behind the bytes that stay, and block_size; returns the record's new size.
TG_HD uint64_t tg_write_new(const unsigned char *rec, const TgPlan &p, const DIndex &ix, uint32_t flags, unsigned char *dst, uint64_t cap)
{
    if (p.kind != TG_REWRITE) return p.size;
    const uint64_t tail_at = p.aux_at + p.kept;
    const TgTail t = tg_tail(rec, p.r, ix, flags, dst + (tail_at <= cap ? tail_at : cap), tail_at <= cap ? cap - tail_at : 0);
    const uint64_t size = tail_at + t.bytes;
    if (cap >= 4) for (int k = 0; k < 4; k++) dst[k] = (unsigned char)((size - 4) >> (8 * k));
    return size;
}
// tg_write_stay: lane `lane` of TG_LANES, its part of the bytes that stay: the whole record when it is copied verbatim, else the fixed fields behind block_size up
// to the qualities and the kept runs of the aux area
TG_HD void tg_write_stay(const unsigned char *rec, const TgPlan &p, uint32_t flags, unsigned char *dst, uint64_t cap, uint32_t lane)
{
    if (p.kind != TG_REWRITE) { if (p.size <= cap) tg_copy(dst, rec, p.size, lane); return; }
    if (p.aux_at <= cap) tg_copy(dst + 4, rec + 4, p.aux_at - 4, lane);
    TgAuxCopy a{dst, rec, p.aux_at, cap, lane};
    (void)tg_aux_walk(rec, p.aux_at, p.size, flags, a);
}
// both parts as lane `lane` of a record's TG_LANES sees them (lane 0 takes the single lane's part too): what the CPU checks run, lane by lane
TG_HD uint64_t tg_write_record(const unsigned char *rec, uint64_t avail, const DIndex &ix, uint32_t flags, unsigned char *dst, uint64_t cap, uint32_t lane)
{
    const TgPlan p = tg_plan(rec, avail, ix, flags);
    tg_write_stay(rec, p, flags, dst, cap, lane);
    return lane == 0u ? tg_write_new(rec, p, ix, flags, dst, cap) : 0;
}
// the length pass's view of the same record
struct TgLen { uint64_t size; int kind; uint32_t removed; TgTail t; };
TG_HD TgLen tg_len_record(const unsigned char *rec, uint64_t avail, const DIndex &ix, uint32_t flags)
{
    const TgPlan p = tg_plan(rec, avail, ix, flags);
    TgLen l; l.kind = p.kind; l.size = p.size; l.removed = 0;
    l.t.bytes = 0; l.t.nm = 0; l.t.mism = 0; l.t.indel = 0; l.t.ts = 0; l.t.no_motif = 0; l.t.conflict = 0;
    if (p.kind != TG_REWRITE) return l;
    l.t = tg_tail(rec, p.r, ix, flags, nullptr, 0);
    l.size = p.aux_at + p.kept + l.t.bytes; l.removed = p.removed;
    return l;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TG_WG)
k_tg_len(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, const DIndex ix,
         uint32_t flags, uint64_t *__restrict__ new_off, uint64_t *__restrict__ tile_sum, uint64_t *__restrict__ part /* 5 planes */, uint64_t *__restrict__ part2 /* 1 plane */)
{
    __shared__ uint64_t s_wave[TG_WG / 64];
    __shared__ unsigned long long s_part[5 * (TG_WG / 64)], s_part2[TG_WG / 64];
    const uint32_t i = blockIdx.x * TG_WG + threadIdx.x;
    uint64_t mine = 0, recs = 0, aux_ts = 0, removed = 0, mism = 0, indel = 0, no_ts = 0;
    if (i < n) {
        const uint64_t at = bam_rec_start(dst_off, tile_base, i);
        if (at < n_raw) {
            const TgLen l = tg_len_record(sorted + at, n_raw - at, ix, flags);
            mine = l.size;
            if (l.kind == TG_NOT_ELIGIBLE) recs = 1ull << 32;
            else if (l.kind == TG_AUX_BAD) aux_ts = 1;
            else {
                recs = 1; removed = l.removed; mism = l.t.mism; indel = l.t.indel;
                if (l.t.ts) aux_ts = 1ull << 32;
                no_ts = (uint64_t)l.t.no_motif | (uint64_t)l.t.conflict << 32;
            }
        }
    }
    uint64_t all;
    const uint64_t ex = d_wg_exclusive(mine, all, s_wave);
    if (i < n) new_off[i] = ex;
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
    const unsigned long long v[5] = {recs, aux_ts, removed, mism, indel};
    cv_block_partials(v, 5, s_part, part);
    const unsigned long long v2[1] = {no_ts};
    cv_block_partials(v2, 1, s_part2, part2);
}

// new_off, new_base: k_tg_len's places and its sums, scanned; `out` holds out_bytes.  Lane = record: the walk, as full as the length pass's, and the few bytes it prints
__global__ void __launch_bounds__(TG_WG)
k_tg_tail(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, const DIndex ix,
          uint32_t flags, const uint64_t *__restrict__ new_off, const uint64_t *__restrict__ new_base, unsigned long long out_bytes, unsigned char *__restrict__ out)
{
    const uint32_t i = blockIdx.x * TG_WG + threadIdx.x;
    if (i >= n) return;
    const uint64_t at = bam_rec_start(dst_off, tile_base, i), to = new_base[blockIdx.x] + new_off[i];
    if (at >= n_raw || to >= out_bytes) return;
    const TgPlan p = tg_plan(sorted + at, n_raw - at, ix, flags);
    (void)tg_write_new(sorted + at, p, ix, flags, out + to, out_bytes - to);
}

// TG_LANES lanes = record: the bytes that stay.  `out` is dword aligned
__global__ void __launch_bounds__(TG_WG)
k_tg_copy(const unsigned char *__restrict__ sorted, const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ tile_base, uint32_t n, unsigned long long n_raw, const DIndex ix,
          uint32_t flags, const uint64_t *__restrict__ new_off, const uint64_t *__restrict__ new_base, unsigned long long out_bytes, unsigned char *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & (TG_LANES - 1u);
    const uint64_t i = (uint64_t)blockIdx.x * (TG_WG / TG_LANES) + threadIdx.x / TG_LANES;
    if (i >= n) return;
    const uint64_t at = bam_rec_start(dst_off, tile_base, (uint32_t)i), to = new_base[i / TG_WG] + new_off[i];
    if (at >= n_raw || to >= out_bytes) return;
    const TgPlan p = tg_plan(sorted + at, n_raw - at, ix, flags);
    tg_write_stay(sorted + at, p, flags, out + to, out_bytes - to, lane);
}
#endif
#endif
