// tests/native/pileup_checks.hip -- the host-callable code of the device's allele counts (dart_amd/csrc/dg_pileup.h) run on the CPU, step by step as the kernels
// apply it: a record's filter and its walk (counting, then emitting into exact-size arrays), the events' sort (here std::stable_sort over the same keys), the two
// scanned planes, the tails with the previous tail carried along, the distinct allele keys and the sites, every entry, the filter and every line's bytes.  The
// reference is a forward-only pac in a zeroed DIndex.
// usage: pileup_checks <input> <output.txt> <output.tsv>
//   input       i64 n_chr, exclude_flags, min_mapq, min_alt, n_raw, names_len, l_pac, pac_bytes; n_chr x i64 chr_off; n_chr x i64 chr_len; (n_chr + 1) x u32 name
//               offsets (padded to 8 bytes); the names (padded to 8); pac (padded to 8); the records
//   output.txt  per record "rec <i> <state> <events>"; "bad <i>" for the first record out of range (then nothing else follows); per sorted event "ev <key> <value>",
//               per distinct allele key "key <key> <n | n_rev << 32> <depth | depth_rev << 32>", per site "site" and the entry's twenty numbers, per kept site "ent"
//               and the same, "stats" and the ten
//   output.tsv  the text
#include "../../dart_amd/csrc/dg_pileup.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "pileup_checks: %s failed (line %d)\n", #x, __LINE__); return 2; } } while (0)

static void print_entry(FILE *txt, const char *what, const dg_site_entry &e)
{
    fprintf(txt, "%s %u %u %u %u %u %u", what, e.chr, e.pos, e.depth, e.depth_rev, e.ref, e.top);
    for (int a = 0; a < 7; a++) fprintf(txt, " %u", e.n[a]);
    for (int a = 0; a < 7; a++) fprintf(txt, " %u", e.n_rev[a]);
    fprintf(txt, "\n");
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: pileup_checks <input> <output.txt> <output.tsv>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<unsigned char> in;
    { unsigned char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k); fclose(f); }
    CHECK(in.size() >= 64);
    long long head[8]; memcpy(head, in.data(), 64);
    const int n_chr = (int)head[0]; const PuFilter flt{(uint32_t)head[1], (uint32_t)head[2]}; const uint32_t min_alt = (uint32_t)head[3];
    const uint64_t n_raw = (uint64_t)head[4], names_len = (uint64_t)head[5], pac_len = (uint64_t)head[7];
    CHECK(n_chr >= 1 && min_alt >= 1);
    const auto pad8 = [](uint64_t x) { return (size_t)((x + 7) & ~7ull); };
    size_t at0 = 64;
    // (exact-size copies on the heap: a read that leaves an array leaves its allocation, which the sanitizer build sees)
    std::vector<int64_t> chr_off((size_t)n_chr), loc_key(2 * (size_t)n_chr, 0); std::vector<int32_t> loc_chr(2 * (size_t)n_chr, 0);
    CHECK(in.size() >= at0 + 16 * (size_t)n_chr);
    memcpy(chr_off.data(), in.data() + at0, 8 * (size_t)n_chr); at0 += 8 * (size_t)n_chr;
    for (int i = 0; i < n_chr; i++) { int64_t len; memcpy(&len, in.data() + at0 + 8 * (size_t)i, 8); loc_key[(size_t)i] = chr_off[(size_t)i] + len - 1; loc_chr[(size_t)i] = i; }
    at0 += 8 * (size_t)n_chr;
    CHECK(in.size() == at0 + pad8(((size_t)n_chr + 1) * 4) + pad8(names_len) + pad8(pac_len) + n_raw);
    std::vector<uint32_t> name_off((size_t)n_chr + 1); memcpy(name_off.data(), in.data() + at0, ((size_t)n_chr + 1) * 4); at0 += pad8(((size_t)n_chr + 1) * 4);
    std::vector<char> names(in.begin() + (long)at0, in.begin() + (long)(at0 + names_len)); at0 += pad8(names_len);
    std::vector<uint8_t> pac(in.begin() + (long)at0, in.begin() + (long)(at0 + pac_len)); at0 += pad8(pac_len);
    std::vector<unsigned char> raw(in.begin() + (long)at0, in.end());
    CHECK(name_off[(size_t)n_chr] == names_len && raw.size() == n_raw && pac_len == (uint64_t)head[6] / 4 + 1);
    DIndex ix; memset(&ix, 0, sizeof ix);
    ix.pac = pac.data(); ix.l_pac = head[6]; ix.n_chr = n_chr; ix.chr_off = chr_off.data(); ix.loc_key = loc_key.data(); ix.loc_chr = loc_chr.data();
    FILE *txt = fopen(argv[2], "w"), *tsv = fopen(argv[3], "wb");
    CHECK(txt && tsv);
    // the packed fetch against the text base by base, at every offset
    for (int64_t g = -3; g < ix.l_pac + 3 && g < 4000; g++) {
        const uint32_t w = pu_ref16(ix, g);
        for (int k = 0; k < PU_STEP; k++) if (g + k >= 0 && g + k < ix.l_pac) CHECK(((w >> (30 - 2 * k)) & 3u) == (uint32_t)d_nt4((unsigned char)d_refchar(ix, g + k)));
    }
    // the records' places (on the device: k_bs_len's scan)
    std::vector<uint64_t> at;
    for (uint64_t p = 0; p + 4 <= n_raw;) { at.push_back(p); p += 4ull + bs_le32(raw.data() + p); }      // (the last record may be cut short by the array's end)
    const size_t n = at.size();
    // k_pu_count
    std::vector<uint64_t> first(n + 1, 0);
    uint64_t counted = 0, left_out = 0, aligned = 0, blocks = 0, mism = 0, del = 0, ins = 0, bad = CV_NONE, kmin = CV_NONE, kmax = 0;
    for (size_t i = 0; i < n; i++) {
        const PuRec r = pu_record(raw.data() + at[i], n_raw - at[i], ix, flt);
        uint64_t ne = 0;
        if (r.state == PU_RANGE) { if (bad == CV_NONE) bad = i; }
        else if (r.state == PU_LEFT_OUT) left_out++;
        else if (r.state == PU_COUNTED) {
            PuNoSink none;
            const PuTally t = pu_walk(raw.data() + at[i], r, ix, none);
            counted++; ne = t.events; aligned += t.aligned; blocks += t.blocks; mism += t.mism; del += t.del; ins += t.ins;
            CHECK(t.events == 2ull * t.blocks + t.mism + t.del + t.ins);
            if (ne) { kmin = std::min(kmin, pu_key_lo(r)); kmax = std::max(kmax, pu_key_hi(r)); }
        }
        fprintf(txt, "rec %zu %d %llu\n", i, r.state, (unsigned long long)ne);
        first[i + 1] = first[i] + ne;
    }
    if (bad != CV_NONE) { fprintf(txt, "bad %llu\n", (unsigned long long)bad); fclose(txt); fclose(tsv); return 0; }
    const uint64_t n_ev = first[n];
    // k_pu_emit: exact-size arrays, every slot written exactly once
    std::vector<uint64_t> keys((size_t)n_ev, CV_NONE); std::vector<int64_t> vals((size_t)n_ev, 0);
    for (size_t i = 0; i < n; i++) {
        const PuRec r = pu_record(raw.data() + at[i], n_raw - at[i], ix, flt);
        if (r.state != PU_COUNTED) continue;
        PuEmit e{keys.data(), vals.data(), first[i], first[i + 1], (uint32_t)r.refid, r.s};        // (the limit: the record's own end, tighter than the kernel's)
        CHECK(pu_walk(raw.data() + at[i], r, ix, e).events == first[i + 1] - first[i]);
        for (uint64_t k = first[i]; k < first[i + 1]; k++) CHECK(keys[k] != CV_NONE && keys[k] >= pu_key_lo(r) && keys[k] <= pu_key_hi(r) && vals[k] != 0);
    }
    // the sort: no key differs from another in a bit the sorter does not look at
    const int bits = n_ev ? std::min(cv_key_bits(kmin, kmax), pu_key_bits_max(n_chr)) : 0;
    for (uint64_t k = 0; k < n_ev; k++) CHECK(bits >= 64 || (keys[k] >> bits) == (kmin >> bits));
    std::vector<uint32_t> order((size_t)n_ev);
    for (uint64_t k = 0; k < n_ev; k++) order[k] = (uint32_t)k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    std::vector<uint64_t> skey((size_t)n_ev); std::vector<int64_t> sval((size_t)n_ev);
    for (uint64_t k = 0; k < n_ev; k++) { skey[k] = keys[order[k]]; sval[k] = vals[order[k]]; fprintf(txt, "ev %llu %lld\n", (unsigned long long)skey[k], (long long)sval[k]); }
    // k_pu_scan, k_pu_tails / k_cv_tails_top / k_pu_flag, k_pu_compact: the planes, the previous tail, the marks of a workgroup's events
    std::vector<uint64_t> incl_d((size_t)n_ev), incl_a((size_t)n_ev), ak_key, ak_n, ak_depth; std::vector<uint32_t> site_key;
    uint64_t run_d = 0, run_a = 0, prev = 0;                                  // prev: the last tail in front, index + 1
    uint32_t in_wg_keys = 0, in_wg_sites = 0;
    for (uint64_t k = 0; k < n_ev; k++) {
        if (k % PU_WG == 0) { in_wg_keys = 0; in_wg_sites = 0; }
        run_d += pu_plane_depth(skey[k], sval[k]); run_a += pu_plane_allele(skey[k], sval[k]);
        incl_d[k] = run_d; incl_a[k] = run_a;
        CHECK((uint32_t)run_d < 0x80000000u && (run_d >> 32) < 0x80000000ull);       // every prefix a true pair of counts
        const bool tail = cv_is_tail(skey[k], k + 1 < n_ev ? skey[k + 1] : 0ull, k + 1 == n_ev);
        const bool ak = pu_is_allele_key(tail, skey[k]), site = pu_opens_site(ak, skey[k], prev != 0, prev ? skey[prev - 1] : 0ull);
        const uint32_t m = pu_mark(in_wg_keys | in_wg_sites << 16, ak, site);
        CHECK(pu_mark_keys(m) == in_wg_keys && pu_mark_sites(m) == in_wg_sites && (m >> 30 & 1u) == (ak ? 1u : 0u) && (m >> 31) == (site ? 1u : 0u));
        if (ak) {
            if (site) site_key.push_back((uint32_t)ak_key.size());
            ak_key.push_back(skey[k]); ak_n.push_back(incl_a[k] - (prev ? incl_a[prev - 1] : 0ull)); ak_depth.push_back(incl_d[k]);
            fprintf(txt, "key %llu %llu %llu\n", (unsigned long long)skey[k], (unsigned long long)ak_n.back(), (unsigned long long)ak_depth.back());
        }
        in_wg_keys += ak ? 1u : 0u; in_wg_sites += site ? 1u : 0u;
        if (tail) prev = cv_fill(prev, k + 1);
    }
    CHECK(run_d == 0 && (uint32_t)run_a == mism + del + ins);
    // k_pu_sites / k_pu_write: the text has exactly the scanned size; a byte nobody wrote shows, a byte behind the end is the sanitizer's
    const size_t n_keys = ak_key.size(), n_sites = site_key.size();
    std::vector<dg_site_entry> entries; std::vector<uint64_t> line_at(1, 0);
    uint64_t deepest = 0;
    for (size_t t = 0; t < n_sites; t++) {
        const PuSite s = pu_site(ak_key.data(), ak_n.data(), ak_depth.data(), site_key[t], n_keys, ix, min_alt);
        CHECK(s.e.chr < (uint32_t)n_chr && s.e.ref < 4u && s.e.top < 7u && s.e.top != s.e.ref);
        CHECK(s.e.n[0] + s.e.n[1] + s.e.n[2] + s.e.n[3] + s.e.n[4] == s.e.depth && s.e.n_rev[0] + s.e.n_rev[1] + s.e.n_rev[2] + s.e.n_rev[3] + s.e.n_rev[4] == s.e.depth_rev);
        CHECK(pu_site_mark(5u, s.kept) == (5u | (s.kept ? 0x80000000u : 0u)));
        print_entry(txt, "site", s.e);
        if (!s.kept) continue;
        const uint32_t len = pu_line_len(name_off.data(), s.e);
        entries.push_back(s.e); line_at.push_back(line_at.back() + len);
        if (s.e.depth > deepest) deepest = s.e.depth;
        print_entry(txt, "ent", s.e);
    }
    std::vector<char> text((size_t)line_at.back(), (char)0xA5);
    for (size_t j = 0; j < entries.size(); j++) CHECK(pu_line_write(text.data() + line_at[j], name_off.data(), names.data(), entries[j]) == line_at[j + 1] - line_at[j]);
    fprintf(txt, "stats %llu %llu %llu %llu %llu %llu %zu %zu %llu %llu\n", (unsigned long long)counted, (unsigned long long)blocks, (unsigned long long)aligned, (unsigned long long)mism,
            (unsigned long long)del, (unsigned long long)ins, n_sites, entries.size(), (unsigned long long)left_out, (unsigned long long)deepest);
    CHECK(fwrite(text.data(), 1, text.size(), tsv) == text.size());
    fclose(txt); fclose(tsv);
    return 0;
}
