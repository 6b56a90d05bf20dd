// tests/native/tags_checks.hip -- the host-callable code of the device's MD / NM / ts stage (dart_amd/csrc/dg_tags.h) run on the CPU, step by step as the kernels
// apply it: per record the length pass (eligibility, the aux walk, the counting walk), the scan of the new sizes, then the write pass lane by lane -- all TG_LANES
// lanes of a record, one after the other -- into an array of exactly the scanned size.  The reference is a forward-only pac in a zeroed DIndex.
// usage: tags_checks <input> <output.txt> <output.bin>
//   input       i64 n_chr, flags, n_raw, l_pac, pac_bytes, 0, 0, 0; n_chr x i64 chr_off; n_chr x i64 chr_len; pac (padded to 8 bytes); the records
//   output.txt  per record "rec <i> <kind> <new size>", then "stats" and the eight
//   output.bin  the new array
#include "../../dart_amd/csrc/dg_tags.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "tags_checks: %s failed (line %d)\n", #x, __LINE__); return 2; } } while (0)

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: tags_checks <input> <output.txt> <output.bin>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<unsigned char> in;
    { unsigned char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k); fclose(f); }
    CHECK(in.size() >= 64);
    long long head[8]; memcpy(head, in.data(), 64);
    const int n_chr = (int)head[0]; const uint32_t flags = (uint32_t)head[1];
    const uint64_t n_raw = (uint64_t)head[2], pac_len = (uint64_t)head[4];
    CHECK(n_chr >= 1 && flags >= 1u && flags <= TG_ALL);
    const auto pad8 = [](uint64_t x) { return (size_t)((x + 7) & ~7ull); };
    size_t at0 = 64;
    // (exact-size copies on the heap: a read that leaves an array leaves its allocation, which the sanitizer build sees)
    std::vector<int64_t> chr_off((size_t)n_chr), loc_key(2 * (size_t)n_chr, 0); std::vector<int32_t> loc_chr(2 * (size_t)n_chr, 0);
    CHECK(in.size() >= at0 + 16 * (size_t)n_chr);
    memcpy(chr_off.data(), in.data() + at0, 8 * (size_t)n_chr); at0 += 8 * (size_t)n_chr;
    for (int i = 0; i < n_chr; i++) { int64_t len; memcpy(&len, in.data() + at0 + 8 * (size_t)i, 8); loc_key[(size_t)i] = chr_off[(size_t)i] + len - 1; loc_chr[(size_t)i] = i; }
    at0 += 8 * (size_t)n_chr;
    CHECK(in.size() == at0 + pad8(pac_len) + n_raw);
    std::vector<uint8_t> pac(in.begin() + (long)at0, in.begin() + (long)(at0 + pac_len)); at0 += pad8(pac_len);
    std::vector<unsigned char> raw(in.begin() + (long)at0, in.end());
    CHECK(raw.size() == n_raw && pac_len == (uint64_t)head[3] / 4 + 1);
    DIndex ix; memset(&ix, 0, sizeof ix);
    ix.pac = pac.data(); ix.l_pac = head[3]; ix.n_chr = n_chr; ix.chr_off = chr_off.data(); ix.loc_key = loc_key.data(); ix.loc_chr = loc_chr.data();
    FILE *txt = fopen(argv[2], "w"), *bin = fopen(argv[3], "wb");
    CHECK(txt && bin);
    // decimal runs: the digits change at 10, 100, ...
    for (uint32_t u : {0u, 9u, 10u, 99u, 100u, 999u, 1000u, 999999999u, 1000000000u, 4294967295u}) {
        unsigned char b[24]; TgPut o{b, 0, sizeof b, true}; tg_num(o, u);
        char want[24]; const int w = snprintf(want, sizeof want, "%llu", (unsigned long long)u);
        CHECK(o.n == (uint64_t)w && !memcmp(b, want, (size_t)w));
        TgPut cnt{nullptr, 0, 0, true}; tg_num(cnt, u); CHECK(cnt.n == (uint64_t)w);
        TgPut off{nullptr, 0, 0, false}; tg_num(off, u); CHECK(off.n == 0);
    }
    CHECK(tg_nm_width(255) == 1u && tg_nm_width(256) == 2u && tg_nm_width(65535) == 2u && tg_nm_width(65536) == 4u);
    // the motifs: exactly four of the 256 vote
    { int plus = 0, minus = 0;
      for (uint32_t m = 0; m < 256; m++) { const uint32_t v = tg_motif(m >> 6, m >> 4 & 3u, m >> 2 & 3u, m & 3u); plus += v == 1u; minus += v == 2u; CHECK(v <= 2u); }
      CHECK(plus == 2 && minus == 2 && tg_motif(2, 3, 0, 2) == 1u && tg_motif(2, 1, 0, 2) == 1u && tg_motif(1, 3, 0, 1) == 2u && tg_motif(1, 3, 2, 1) == 2u); }
    // the records' places (on the device: k_bs_len's scan)
    std::vector<uint64_t> at;
    for (uint64_t p = 0; p + 4 <= n_raw;) { at.push_back(p); p += 4ull + bs_le32(raw.data() + p); }      // (the last record may be cut short by the array's end)
    const size_t n = at.size();
    // k_tg_len
    std::vector<uint64_t> to(n + 1, 0);
    uint64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < n; i++) {
        const TgLen l = tg_len_record(raw.data() + at[i], n_raw - at[i], ix, flags);
        if (l.kind == TG_NOT_ELIGIBLE) st[1]++;
        else if (l.kind == TG_AUX_BAD) st[2]++;
        else { st[0]++; st[3] += l.removed; st[4] += l.t.mism; st[5] += l.t.indel; st[6] += l.t.ts ? 1 : 0; st[7] += (uint64_t)l.t.no_motif | (uint64_t)l.t.conflict << 32; CHECK(l.t.nm == l.t.mism + l.t.indel); }
        if (l.kind != TG_REWRITE) CHECK(l.size == (at[i] + 4ull + bs_le32(raw.data() + at[i]) <= n_raw ? 4ull + bs_le32(raw.data() + at[i]) : n_raw - at[i]));
        fprintf(txt, "rec %zu %d %llu\n", i, l.kind, (unsigned long long)l.size);
        to[i + 1] = to[i] + l.size;
    }
    // k_tg_tail and k_tg_copy (tg_write_record is both, as one lane of sixteen sees them): an array of exactly the scanned size, filled twice with different bytes: a byte nobody wrote shows, a byte behind the end is the sanitizer's
    const uint64_t bytes = to[n];
    std::vector<unsigned char> out((size_t)bytes, (unsigned char)0xA5), again((size_t)bytes, (unsigned char)0x5A);
    for (std::vector<unsigned char> *o : {&out, &again})
        for (size_t i = 0; i < n; i++)
            for (uint32_t lane = 0; lane < TG_LANES; lane++) {
                // (each record's own room as the cap: tighter than the kernel's, which is the rest of the array)
                const uint64_t size = tg_write_record(raw.data() + at[i], n_raw - at[i], ix, flags, o->data() + to[i], to[i + 1] - to[i], lane);
                if (lane == 0u) CHECK(size == to[i + 1] - to[i]);
            }
    CHECK(out == again);
    // a cap that is too small stores nothing behind it (the kernel's guard against a length pass that disagrees)
    for (size_t i = 0; i < n && i < 64; i++) {
        const uint64_t room = to[i + 1] - to[i];
        if (room < 8) continue;
        std::vector<unsigned char> small((size_t)room - 5, (unsigned char)0xA5);
        for (uint32_t lane = 0; lane < TG_LANES; lane++) (void)tg_write_record(raw.data() + at[i], n_raw - at[i], ix, flags, small.data(), small.size(), lane);
    }
    fprintf(txt, "stats %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[3],
            (unsigned long long)st[4], (unsigned long long)st[5], (unsigned long long)st[6], (unsigned long long)st[7]);
    CHECK(fwrite(out.data(), 1, out.size(), bin) == out.size());
    fclose(txt); fclose(bin);
    return 0;
}
