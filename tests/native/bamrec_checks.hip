// tests/native/bamrec_checks.hip -- the record reader of dart_amd/csrc/dg_bamrec.h run on the CPU over crafted records, each at every `avail` from 0 to its
// length + 4, and what every stage function that sits on it returns for the same bytes.
// usage: bamrec_checks <input> <output.txt>
//   input       i64 n_chr, chr_len (every chromosome's), n_records; per record i64 length and its bytes (padded to 8).  Behind a record the array goes on with
//               four bytes 0xEE; a case is the first `avail` bytes of that.
//   output.txt  per (record, avail) one line each, all numbers decimal (64-bit values unsigned):
//     head  ok refid pos l_name mapq n_cigar flag l_seq next_refid next_pos tlen block size cigar_at seq_at qual_at aux_at
//     walk  n_ops, then op len p q per op, then p q behind the last: the ops that fit in `size`, from (uint64_t)pos
//     key   bs_key (avail >= 36 only)            chk   bs_record_check's code and size
//     bi    refid pos beg end rlen bin placed mapped
//     cv    counted refid pos cigar_at n_ops, then its blocks' start and end when counted (exclude 0x704)
//     md    examined candidate bad E h score, and md_name_len (avail >= 36 only)
//     pu    state refid pos n_ops l_seq s cigar_at seq_at rlen (exclude 0, min_mapq 0)
//     qc    whole flag mapq l_seq refid pos next_refid next_pos tlen
//     tg    kind size aux_at kept removed (all three tags)
#include "../../dart_amd/csrc/dg_bamidx.h"
#include "../../dart_amd/csrc/dg_markdup.h"
#include "../../dart_amd/csrc/dg_qc.h"
#include "../../dart_amd/csrc/dg_tags.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "bamrec_checks: %s failed (line %d)\n", #x, __LINE__); return 2; } } while (0)
typedef unsigned long long ull;

struct PrintOps { FILE *o; void operator()(uint32_t op, uint32_t len, uint64_t p, uint64_t q) const { fprintf(o, " %u %u %llu %llu", op, len, (ull)p, (ull)q); } };
struct PrintBlocks { FILE *o; void operator()(uint32_t, uint64_t s, uint64_t e) { fprintf(o, " %llu %llu", (ull)s, (ull)e); } };

static void head_and_walk(FILE *o, const unsigned char *rec, uint64_t avail)
{
    const BamHead h = bam_head(rec, avail);
    fprintf(o, "head %d %d %d %u %u %u %u %u %d %d %d %llu %llu %llu %llu %llu %llu\n", (int)h.ok, h.refid, h.pos, h.l_name, h.mapq, h.n_cigar, h.flag, h.l_seq, h.next_refid, h.next_pos, h.tlen,
            (ull)h.block, (ull)h.size, (ull)h.cigar_at, (ull)h.seq_at, (ull)h.qual_at, (ull)h.aux_at);
    uint64_t n_ops = h.cigar_at <= h.size ? (h.size - h.cigar_at) / 4 : 0;
    if (n_ops > h.n_cigar) n_ops = h.n_cigar;
    fprintf(o, "walk %llu", (ull)n_ops);
    const BamAt end = bam_cigar_walk(rec, h.cigar_at, n_ops, (uint64_t)h.pos, PrintOps{o});
    fprintf(o, " %llu %llu\n", (ull)end.p, (ull)end.q);
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: bamrec_checks <input> <output.txt>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<unsigned char> in;
    { unsigned char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k); fclose(f); }
    CHECK(in.size() >= 24);
    long long head[3]; memcpy(head, in.data(), 24);
    const int n_chr = (int)head[0];
    CHECK(n_chr >= 1 && head[1] >= 1 && head[2] >= 0);
    // a DIndex as far as the record functions look: the chromosomes' places (ChrLocMap's forward keys are their last bases)
    std::vector<int64_t> chr_off((size_t)n_chr), loc_key(2 * (size_t)n_chr, 0);
    for (int t = 0; t < n_chr; t++) { chr_off[(size_t)t] = (int64_t)t * head[1]; loc_key[(size_t)t] = chr_off[(size_t)t] + head[1] - 1; }
    DIndex ix; memset(&ix, 0, sizeof ix);
    ix.n_chr = n_chr; ix.chr_off = chr_off.data(); ix.loc_key = loc_key.data();
    FILE *o = fopen(argv[2], "w");
    CHECK(o);
    size_t at = 24;
    for (long long i = 0; i < head[2]; i++) {
        CHECK(at + 8 <= in.size());
        long long len; memcpy(&len, in.data() + at, 8); at += 8;
        CHECK(len >= 0 && at + (size_t)len <= in.size());
        std::vector<unsigned char> whole(in.begin() + (long)at, in.begin() + (long)at + (long)len);
        whole.insert(whole.end(), 4, (unsigned char)0xEE);
        at += ((size_t)len + 7) & ~(size_t)7;
        for (uint64_t avail = 0; avail <= whole.size(); avail++) {
            // (an exact-size copy on the heap: a read behind `avail` leaves its allocation, which the sanitizer build sees)
            std::vector<unsigned char> cut(whole.begin(), whole.begin() + (long)avail);
            const unsigned char *rec = cut.data();
            fprintf(o, "case %lld %llu\n", i, (ull)avail);
            head_and_walk(o, rec, avail);
            if (avail >= BAM_FIXED) fprintf(o, "key %llu\n", (ull)bs_key(rec, n_chr));
            size_t size = 0;
            const int code = bs_record_check(rec, (size_t)avail, n_chr, &size);
            fprintf(o, "chk %d %zu\n", code, code == BS_REC_OK ? size : (size_t)0);
            const BiRec b = bi_record(rec, avail, n_chr);
            fprintf(o, "bi %d %d %lld %lld %lld %u %d %d\n", b.refid, b.pos, b.beg, b.end, b.rlen, b.bin, (int)b.placed, (int)b.mapped);
            const CvFilter cf{0u, 0x704u, 0u};
            const CvRec c = cv_record(rec, avail, n_chr, cf);
            fprintf(o, "cv %d %d %d %llu %u", (int)c.counted, c.refid, c.pos, (ull)c.cigar_at, c.n_ops);
            if (c.counted) { PrintBlocks pb{o}; (void)cv_blocks(rec, c, pb); }
            fprintf(o, "\n");
            const MdRec m = md_record(rec, avail, n_chr, MD_HASH_BITS);
            fprintf(o, "md %d %d %d %llu %llu %u %u\n", (int)m.examined, (int)m.candidate, (int)m.bad, (ull)m.E, (ull)m.h, m.score, avail >= BAM_FIXED ? md_name_len(rec) : 0u);
            const PuFilter pf{0u, 0u};
            const PuRec p = pu_record(rec, avail, ix, pf);
            fprintf(o, "pu %d %d %d %u %u %u %llu %llu %llu\n", p.state, p.refid, p.pos, p.n_ops, p.l_seq, p.s, (ull)p.cigar_at, (ull)p.seq_at, (ull)p.rlen);
            const QcHead q = qc_head(rec, avail);
            fprintf(o, "qc %d %u %u %u %d %d %d %d %d\n", (int)q.whole, q.flag, q.mapq, q.l_seq, q.refid, q.pos, q.next_refid, q.next_pos, q.tlen);
            const TgPlan t = tg_plan(rec, avail, ix, TG_ALL);
            fprintf(o, "tg %d %llu %llu %llu %u\n", t.kind, (ull)t.size, (ull)t.aux_at, (ull)t.kept, t.removed);
        }
    }
    fclose(o);
    return 0;
}
