// tests/native/qc_checks.hip -- the host-callable code of the device's QC tables (dart_amd/csrc/dg_qc.h) run on the CPU as the kernels apply it: k_qc_flag's lane
// per record (qc_head, qc_tables), k_qc_cycle's group of lanes per record -- the filter, the per-op terms handed to lane j & 15, the steps of 64 bases with the cursor carried
// along, and in every step QC_GROUP lanes with four bases each (qc_lane_step: qc_quad, qc_fetch4, qc_base) -- and the host formatter.  The reference is a forward-only
// pac in a zeroed DIndex; the array and the pac are exact-size heap copies, so a read that leaves them is the sanitizer build's.
// usage: qc_checks tables <input> <output.words> <output.txt>
//          input         i64 n_chr, exclude_flags, min_mapq, 0, n_raw, names_len, l_pac, pac_bytes; n_chr x i64 chr_off; n_chr x i64 chr_len; (n_chr + 1) x u32 name
//                        offsets (padded to 8 bytes); the names (padded to 8); pac (padded to 8); the records
//          output.words  the u64 words; output.txt: qc_format's text of them
//        qc_checks format <input> <output.txt>
//          input         i64 n_chr; n_chr x i64 lengths; per name i64 length and the bytes; the u64 words
#include "../../dart_amd/csrc/dg_qc.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "qc_checks: %s failed (line %d)\n", #x, __LINE__); return 2; } } while (0)

struct HostSink {                   // every term into the one array of words
    uint64_t *w; int n_chr;
    void sn(uint32_t word, unsigned long long v) { w[qc_off_sn(n_chr) + word] += v; }
    void fs(uint32_t fail, uint32_t row) { w[qc_off_fs() + fail * 16u + row]++; }
    void ch(uint32_t t, uint32_t col) { w[qc_off_ch() + 2u * t + col]++; }
    void mq(uint32_t q) { w[qc_off_mq(n_chr) + q]++; }
    void is(uint32_t row, uint32_t bin) { w[qc_off_is(n_chr) + (size_t)row * DG_QC_ISIZE + bin]++; }
    void rl(uint32_t k, uint32_t bin) { w[qc_off_rl(n_chr) + k * (uint32_t)DG_QC_CYCLES + bin]++; }
    void pc(uint32_t k, uint32_t col, uint32_t cycle, uint32_t v) { w[qc_off_pc(n_chr) + ((size_t)k * 12 + col) * DG_QC_CYCLES + cycle] += v; }
    void id(uint32_t row, uint32_t bin) { w[qc_off_id(n_chr) + row * (uint32_t)DG_QC_INDEL + bin]++; }
};

static bool slurp(const char *path, std::vector<unsigned char> &in)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return false; }
    unsigned char buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k);
    fclose(f);
    return true;
}

static int run_format(const char *src, const char *dst)
{
    std::vector<unsigned char> in;
    if (!slurp(src, in)) return 1;
    CHECK(in.size() >= 8);
    long long n_chr; memcpy(&n_chr, in.data(), 8);
    CHECK(n_chr >= 1 && in.size() >= 8 + 8 * (size_t)n_chr);
    std::vector<int64_t> lens((size_t)n_chr); memcpy(lens.data(), in.data() + 8, 8 * (size_t)n_chr);
    size_t at = 8 + 8 * (size_t)n_chr;
    std::vector<std::string> names;
    for (long long k = 0; k < n_chr; k++) { long long l; CHECK(in.size() >= at + 8); memcpy(&l, in.data() + at, 8); at += 8; CHECK(l >= 0 && in.size() >= at + (size_t)l); names.emplace_back((const char *)in.data() + at, (size_t)l); at += (size_t)l; }
    CHECK(in.size() == at + 8 * qc_words((int)n_chr));
    std::vector<uint64_t> w(qc_words((int)n_chr)); memcpy(w.data(), in.data() + at, 8 * w.size());
    std::vector<const char *> np; for (auto &s : names) np.push_back(s.c_str());
    std::string text;
    qc_format(w.data(), (int)n_chr, np.data(), lens.data(), text);
    FILE *o = fopen(dst, "wb");
    CHECK(o && fwrite(text.data(), 1, text.size(), o) == text.size());
    fclose(o);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "format")) return run_format(argv[2], argv[3]);
    if (argc != 5 || strcmp(argv[1], "tables")) { fprintf(stderr, "usage: qc_checks tables <input> <output.words> <output.txt> | qc_checks format <input> <output.txt>\n"); return 1; }
    std::vector<unsigned char> in;
    if (!slurp(argv[2], in)) return 1;
    CHECK(in.size() >= 64);
    long long head[8]; memcpy(head, in.data(), 64);
    const int n_chr = (int)head[0]; const PuFilter flt{(uint32_t)head[1], (uint32_t)head[2]};
    const uint64_t n_raw = (uint64_t)head[4], names_len = (uint64_t)head[5], pac_len = (uint64_t)head[7];
    CHECK(n_chr >= 1);
    const auto pad8 = [](uint64_t x) { return (size_t)((x + 7) & ~7ull); };
    size_t at0 = 64;
    std::vector<int64_t> chr_off((size_t)n_chr), chr_len((size_t)n_chr), loc_key(2 * (size_t)n_chr, 0); std::vector<int32_t> loc_chr(2 * (size_t)n_chr, 0);
    CHECK(in.size() >= at0 + 16 * (size_t)n_chr);
    memcpy(chr_off.data(), in.data() + at0, 8 * (size_t)n_chr); at0 += 8 * (size_t)n_chr;
    memcpy(chr_len.data(), in.data() + at0, 8 * (size_t)n_chr); at0 += 8 * (size_t)n_chr;
    for (int i = 0; i < n_chr; i++) { loc_key[(size_t)i] = chr_off[(size_t)i] + chr_len[(size_t)i] - 1; loc_chr[(size_t)i] = i; }
    CHECK(in.size() == at0 + pad8(((size_t)n_chr + 1) * 4) + pad8(names_len) + pad8(pac_len) + n_raw);
    std::vector<uint32_t> name_off((size_t)n_chr + 1); memcpy(name_off.data(), in.data() + at0, ((size_t)n_chr + 1) * 4); at0 += pad8(((size_t)n_chr + 1) * 4);
    std::vector<char> names(in.begin() + (long)at0, in.begin() + (long)(at0 + names_len)); at0 += pad8(names_len);
    std::vector<uint8_t> pac(in.begin() + (long)at0, in.begin() + (long)(at0 + pac_len)); at0 += pad8(pac_len);
    std::vector<unsigned char> raw(in.begin() + (long)at0, in.end());
    CHECK(name_off[(size_t)n_chr] == names_len && raw.size() == n_raw && pac_len == (uint64_t)head[6] / 4 + 1);
    DIndex ix; memset(&ix, 0, sizeof ix);
    ix.pac = pac.data(); ix.l_pac = head[6]; ix.n_chr = n_chr; ix.chr_off = chr_off.data(); ix.loc_key = loc_key.data(); ix.loc_chr = loc_chr.data();
    // the section offsets leave no gap and no overlap
    CHECK(qc_off_ch() == 32 && qc_off_mq(n_chr) == qc_off_ch() + 2 * ((size_t)n_chr + 1) && qc_off_is(n_chr) == qc_off_mq(n_chr) + 256 && qc_off_rl(n_chr) == qc_off_is(n_chr) + 3 * 8001 &&
          qc_off_pc(n_chr) == qc_off_rl(n_chr) + 1024 && qc_off_id(n_chr) == qc_off_pc(n_chr) + 12288 && qc_off_sn(n_chr) == qc_off_id(n_chr) + 130 && qc_words(n_chr) == qc_off_sn(n_chr) + 32);
    std::vector<uint64_t> at;
    for (uint64_t p = 0; p + 4 <= n_raw;) { at.push_back(p); p += 4ull + bs_le32(raw.data() + p); }      // (the last record may be cut short by the array's end)
    std::vector<uint64_t> words(qc_words(n_chr), 0);
    HostSink s{words.data(), n_chr};
    // k_qc_flag: lane = record
    for (size_t i = 0; i < at.size(); i++) qc_tables(qc_head(raw.data() + at[i], n_raw - at[i]), n_chr, s);
    // k_qc_cycle: a group of QC_GROUP lanes = record
    QcLaneSums sums{0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < at.size(); i++) {
        const unsigned char *rec = raw.data() + at[i];
        const QcHead h = qc_head(rec, n_raw - at[i]);
        if (!h.whole) continue;
        const PuRec r = pu_record(rec, n_raw - at[i], ix, flt);
        if (r.state == PU_LEFT_OUT || r.state == PU_RANGE) s.sn(QC_SN_LEFT_OUT, 1);
        if (r.state != PU_COUNTED) continue;
        const uint32_t k = h.flag >> 7 & 1u;
        s.sn(QC_SN_PROFILED, 1);
        uint64_t q = 0;
        for (uint32_t j = 0; j < r.n_ops; j++) {
            const uint32_t w = bs_le32(rec + r.cigar_at + 4ull * j), op = w & 15u, len = w >> 4;
            qc_op_event(op, len, q, r.l_seq, r.s, k, s);
            if (qc_op_takes_read(op)) q += len;
        }
        CHECK(q == r.l_seq);
        QcCursor c{0u, 0ull, (uint64_t)r.pos};
        const unsigned long long before = sums.bases;
        for (uint64_t b = 0; b < (uint64_t)r.l_seq; b += QC_STEP) {
            qc_seek(rec, r, c, b);
            CHECK(c.j < r.n_ops && c.q <= b);                            // the cursor's op holds the step's first base
            const uint64_t end = b + QC_STEP < (uint64_t)r.l_seq ? b + QC_STEP : (uint64_t)r.l_seq;
            for (uint32_t lane = 0; lane < (uint32_t)QC_GROUP; lane++) qc_lane_step(rec, r, ix, c, b + (uint64_t)lane * QC_LANE_BASES, end, k, s, sums);
        }
        CHECK(sums.bases - before == r.l_seq);                           // every stored base of a profiled record lies in exactly one op
    }
    s.sn(QC_SN_PROF_BASES, sums.bases); s.sn(QC_SN_ALIGNED, sums.aligned); s.sn(QC_SN_MISMATCH, sums.mism); s.sn(QC_SN_INSERTED, sums.inserted); s.sn(QC_SN_CLIPPED, sums.clipped);
    s.sn(QC_SN_NOQUAL, sums.noqual); s.sn(QC_SN_QUAL_SUM, sums.qsum);
    std::vector<std::string> nm; std::vector<const char *> np;
    for (int t = 0; t < n_chr; t++) nm.emplace_back(names.data() + name_off[(size_t)t], names.data() + name_off[(size_t)t + 1]);
    for (auto &x : nm) np.push_back(x.c_str());
    std::string text;
    qc_format(words.data(), n_chr, np.data(), chr_len.data(), text);
    FILE *fw = fopen(argv[3], "wb"), *ft = fopen(argv[4], "wb");
    CHECK(fw && ft);
    CHECK(fwrite(words.data(), 8, words.size(), fw) == words.size() && fwrite(text.data(), 1, text.size(), ft) == text.size());
    fclose(fw); fclose(ft);
    return 0;
}
