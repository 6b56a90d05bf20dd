// CPU suite: the __host__ __device__ functions of dart_amd/csrc/dg_bamfmt.h and dg_bgzf.h run on the host.
//   records <batch> <out>   the per-read record code, read by read, the way k_bam_len (lengths, counters) and k_bam_write (the bytes) use it; the batch is
//                           the file tests/sam_device_inputs.py::write_batch writes; out = u64 len[n], u64 counters[3], u64 records, u64 refused,
//                           u64 bytes, the records
//   tokens <out>            one raw deflate stream per (length, distance): `distance` literals, ONE match token, the end-of-block code; out = a list of
//                           u32 length, u32 distance, u32 stream bytes, the stream.  Literal i is bgzf_check_byte(i).
//   deflate <file> <out>    the file as BGZF blocks through the lane functions of k_bgzf_deflate, in the kernel's order: a strip's lanes one after the other
//                           through each phase (tokens; scan of the bit counts; bits into the zeroed slot; table inserts), a barrier being the end of a loop
//   crc <file> <cut>...     CRC32 of the file from the CRCs of its pieces [0, cut1), [cut1, cut2), ... combined with bgzf_crc_combine, and once more the way
//                           k_bgzf_deflate does it (256 pieces, pairwise); prints both in hex
#include "../../dart_amd/csrc/dg_bamfmt.h"
#include "../../dart_amd/csrc/dg_bgzf.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static std::vector<char> blob;
static size_t at = 0;
template <typename T> static const T *take(size_t n) { const T *p = (const T *)(blob.data() + at); at += (n * sizeof(T) + 7) & ~(size_t)7; if (at > blob.size()) { fprintf(stderr, "input too short\n"); exit(2); } return p; }
static bool slurp(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END); blob.resize((size_t)ftell(f) + 8); fseek(f, 0, SEEK_SET);
    const bool ok = fread(blob.data(), 1, blob.size() - 8, f) == blob.size() - 8;
    fclose(f);
    return ok;
}

static int records(const char *in, const char *out)
{
    if (!slurp(in)) return 2;
    const int32_t *h = take<int32_t>(8);
    const int n = h[0], n_rep = h[1], n_cig = h[2], n_chr = h[3], has_qual = h[7];
    SamBatch b;
    b.n_reads = n; b.n_pair_mode = h[4]; b.unique_only = h[5]; b.multi = h[6]; b.qlen = nullptr;
    b.ro = take<dg_read_out>(n); b.po = take<dg_report_out>(n_rep); b.cig = take<uint32_t>(n_cig);
    b.seq_off = take<uint32_t>(n + 1); b.rlen = take<uint16_t>(n); b.seq = take<unsigned char>(b.seq_off[n]);
    b.hdr_off = take<uint32_t>(n + 1); b.hdr = take<char>(b.hdr_off[n]);
    b.qual_off = take<uint32_t>(n + 1); b.qual = take<char>(b.qual_off[n]);
    if (!has_qual) b.qual = nullptr;
    b.chr_off = take<uint32_t>(n_chr + 1); b.chr = take<char>(b.chr_off[n_chr]);

    std::vector<uint64_t> len(n);
    std::vector<uint32_t> ql(n);
    uint64_t ct64[5] = {0, 0, 0, 0, 0}, total = 0;
    for (int k = 0; k < n; k++) {
        uint32_t ct[3] = {0, 0, 0}, rr[2] = {0, 0};
        len[k] = bam_read_len(b, k, ct, rr, &ql[k]); total += len[k];
        for (int i = 0; i < 3; i++) ct64[i] += ct[i];
        ct64[3] += rr[0]; ct64[4] += rr[1];
    }
    std::vector<unsigned char> rec(total + 1);
    uint64_t pos = 0; int bad = 0;
    SamBatch b2 = b; b2.qlen = ql.data();                  // the writer takes the quality lengths pass 1 left, as k_bam_write does
    for (int k = 0; k < n; k++) {
        const uint64_t w = bam_read_records(b2, k, rec.data() + pos);
        if (w != len[k]) { fprintf(stderr, "read %d: wrote %llu bytes, pass 1 said %llu\n", k, (unsigned long long)w, (unsigned long long)len[k]); bad++; }
        // every record once more from the pieces the kernel's lanes store: the staged fixed bytes and tags, a byte of bases, a byte of quality
        const SamRead e = sam_read_begin(b2, k);
        uint64_t lp = pos;
        for (int j = sam_line_first(b2, e); j != SAM_LINE_NONE; j = sam_line_after(b2, e, j)) {
            const uint32_t sz = bam_line_size(b2, e, j);
            if (!sz) continue;
            unsigned char fix[BAM_FIXED], tags[BAM_TAGS_MAX + 3];
            bam_line_fixed(b2, e, j, sz, fix);
            const uint32_t nt = bam_line_tags(e, j, tags);
            if (memcmp(fix, rec.data() + lp, BAM_FIXED)) { fprintf(stderr, "read %d line %d: staged fixed bytes differ\n", k, j); bad++; }
            if (nt > BAM_TAGS_MAX || memcmp(tags, rec.data() + lp + sz - nt, nt)) { fprintf(stderr, "read %d line %d: staged tags differ\n", k, j); bad++; }
            lp += sz;
        }
        if (lp != pos + w) { fprintf(stderr, "read %d: record sizes do not add up\n", k); bad++; }
        pos += w;
    }
    FILE *o = fopen(out, "wb");
    if (!o) return 2;
    fwrite(len.data(), 8, n, o); fwrite(ct64, 8, 5, o); fwrite(&pos, 8, 1, o); fwrite(rec.data(), 1, pos, o);
    fclose(o);
    printf("reads %d bytes %llu bad %d\n", n, (unsigned long long)pos, bad);
    return bad ? 1 : 0;
}

static unsigned char bgzf_check_byte(uint32_t i) { return (unsigned char)((i * 2654435761u) >> 23); }
struct Bits {
    std::vector<unsigned char> v; uint64_t acc = 0; uint32_t n = 0;
    void put(uint32_t bits, uint32_t nb) { acc |= (uint64_t)bits << n; n += nb; while (n >= 8) { v.push_back((unsigned char)acc); acc >>= 8; n -= 8; } }
    void end() { if (n) { v.push_back((unsigned char)acc); acc = 0; n = 0; } }
};
static int tokens(const char *out)
{
    FILE *o = fopen(out, "wb");
    if (!o) return 2;
    std::vector<uint32_t> dists = {1, 2, 3, 4, 32767, 32768};
    for (uint32_t k = 2; k <= 14; k++) for (uint32_t half = 0; half < 2; half++) { const uint32_t d = (1u << k) + half * (1u << (k - 1)) + 1u; dists.push_back(d); dists.push_back(d - 1); dists.push_back(d + 1 <= 32768 ? d + 1 : d); }
    int cases = 0;
    auto one = [&](uint32_t len, uint32_t dist) {
        Bits s;
        s.put(3, 3);                                       // BFINAL = 1, BTYPE = 01
        for (uint32_t i = 0; i < dist; i++) { uint32_t nb; const uint32_t b = bgzf_token_bits(bgzf_check_byte(i), nb); s.put(b, nb); }
        uint32_t nb; const uint32_t b = bgzf_token_bits(bgzf_tok_match(len, dist), nb);
        if (nb != bgzf_token_nbits(bgzf_tok_match(len, dist)) || nb > 31) exit(3);
        s.put(b, nb);
        s.put(0, 7);                                       // end of block
        s.end();
        const uint32_t head[3] = {len, dist, (uint32_t)s.v.size()};
        fwrite(head, 4, 3, o); fwrite(s.v.data(), 1, s.v.size(), o);
        cases++;
    };
    for (uint32_t len = 3; len <= 258; len++) { one(len, 1); one(len, 300); }
    for (uint32_t d : dists) { one(3, d); one(4, d); one(258, d); }
    fclose(o);
    printf("cases %d\n", cases);
    return 0;
}

static int crc(int argc, char **argv)
{
    if (!slurp(argv[2])) return 2;
    const size_t n = blob.size() - 8;
    const unsigned char *p = (const unsigned char *)blob.data();
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; i++) table[i] = bgzf_crc_entry(i);
    uint32_t c = 0; size_t lo = 0;
    for (int a = 3; a <= argc; a++) {
        const size_t hi = a < argc ? (size_t)strtoull(argv[a], nullptr, 10) : n;
        if (hi < lo || hi > n) return 2;
        c = bgzf_crc_combine(c, bgzf_crc_bytes(table, p + lo, (uint32_t)(hi - lo)), (uint32_t)(hi - lo));
        lo = hi;
    }
    // the kernel's scheme: BGZF_THREADS pieces of ceil(n / BGZF_THREADS) bytes, combined pairwise
    uint32_t pc[BGZF_THREADS], pl[BGZF_THREADS];
    const uint32_t per = (uint32_t)((n + BGZF_THREADS - 1) / BGZF_THREADS);
    for (uint32_t t = 0; t < BGZF_THREADS; t++) {
        const uint32_t a = t * per < n ? t * per : (uint32_t)n, b = a + per < n ? a + per : (uint32_t)n;
        pc[t] = bgzf_crc_bytes(table, p + a, b - a); pl[t] = b - a;
    }
    for (uint32_t st = 1; st < BGZF_THREADS; st <<= 1)
        for (uint32_t t = 0; t < BGZF_THREADS; t += 2 * st) { pc[t] = bgzf_crc_combine(pc[t], pc[t + st], pl[t + st]); pl[t] += pl[t + st]; }
    printf("%08x %08x\n", c, pc[0]);
    return 0;
}

static int deflate_file(const char *in, const char *out)
{
    if (!slurp(in)) return 2;
    const size_t n_total = blob.size() - 8;
    FILE *o = fopen(out, "wb");
    if (!o) return 2;
    BgzfLds *s = new BgzfLds;
    std::vector<uint32_t> slot_w(BGZF_SLOT / 4);
    unsigned char *slot = (unsigned char *)slot_w.data();
    for (size_t at = 0; at < n_total; at += BGZF_BLOCK) {
        const uint32_t n = (uint32_t)(n_total - at < BGZF_BLOCK ? n_total - at : BGZF_BLOCK);
        memset(s, 0, sizeof *s); memcpy(s->in, blob.data() + at, n);
        for (auto &w : slot_w) w = 0xdeadbeefu;                // what the kernel does not zero it must not need
        const uint32_t zero_words = (18u + n + 8u + 3u) / 4u + 1u;
        for (uint32_t w = 0; w < zero_words; w++) slot_w[w] = 0;
        for (uint32_t i = 0; i < 256; i++) s->crc_tab[i] = bgzf_crc_entry(i);
        const uint32_t crc = bgzf_crc_bytes(s->crc_tab, (const unsigned char *)s->in, n);
        uint32_t bit_base = 3; bool coded = true;
        for (uint32_t s0 = 0; s0 < n && coded; s0 += BGZF_STRIP) {
            uint32_t nt[BGZF_THREADS], nb[BGZF_THREADS], incl[BGZF_THREADS], sum = 0;
            auto seg = [&](uint32_t t, uint32_t &a, uint32_t &b) { a = s0 + t * BGZF_SEG; b = a + BGZF_SEG < n ? a + BGZF_SEG : n; };
            for (uint32_t t = 0; t < BGZF_THREADS; t++) { uint32_t a, b; seg(t, a, b); nt[t] = bgzf_lane_tokens(*s, t, a, b, nb[t]); if (nt[t] > BGZF_SEG) return 3; }
            for (uint32_t t = 0; t < BGZF_THREADS; t++) s->len[t] = bgzf_lane_meta(*s, t, nt[t]);
            for (uint32_t t = BGZF_THREADS; t-- > 0;) bgzf_lane_merge(*s, s->len, t, nt[t], nb[t]);
            for (uint32_t t = 0; t < BGZF_THREADS; t++) { sum += nb[t]; incl[t] = sum; }
            coded = bgzf_still_coded(bit_base, sum, n);
            for (uint32_t t = BGZF_THREADS; t-- > 0;)             // (any order: here the last lane first)
                if (coded && nt[t]) bgzf_lane_emit(*s, t, nt[t], 18u * 8u + bit_base + incl[t] - nb[t], s0 == 0 && t == 0, slot_w.data());
            bit_base += sum;
            for (uint32_t t = BGZF_THREADS; t-- > 0;) { uint32_t a, b; seg(t, a, b); bgzf_lane_insert(*s, a, b, n); }
        }
        const uint32_t clen = coded ? (bit_base + 7u + 7u) / 8u : n + 5u;
        if (!coded) { bgzf_put_stored_head(slot + 18, n); memcpy(slot + 23, s->in, n); }
        const uint32_t bsize = 18u + clen + 8u;
        if (bsize > BGZF_SLOT) return 3;
        bgzf_put_header(slot, bsize);
        bgzf_put_trailer(slot + 18u + clen, crc, n);
        fwrite(slot, 1, bsize, o);
    }
    fclose(o);
    delete s;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "deflate")) return deflate_file(argv[2], argv[3]);
    if (argc >= 4 && !strcmp(argv[1], "records")) return records(argv[2], argv[3]);
    if (argc >= 3 && !strcmp(argv[1], "tokens")) return tokens(argv[2]);
    if (argc >= 3 && !strcmp(argv[1], "crc")) return crc(argc, argv);
    return 2;
}
