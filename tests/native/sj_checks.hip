// tests/native/sj_checks.hip -- the host-callable code of the device's junction table (dart_amd/csrc/dg_sjtab.h) run on the CPU: the key words and their
// order, the hash and the probe sequence (a serial table with the kernel's two-word claim and the library's growth rule), the chromosome look-up, a line's
// length and bytes.  usage: sj_checks <input> <output>
//   input   i64 n_items, n_chr, l_pac, slots; i64 chr_off[n_chr], chr_len[n_chr]; u32 name_off[n_chr + 1]; names; dg_sj_entry items[n_items] (every
//           array padded to 8 bytes)
//   output  u64 n_entries, n_lines, n_bytes, growths; dg_sj_entry entries[n_entries]; the text
#include "../../dart_amd/csrc/dg_sjtab.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "sj_checks: %s failed (line %d)\n", #x, __LINE__); return 2; } } while (0)

struct HostTable {
    std::vector<SjSlot> t; size_t distinct = 0, growths = 0;
    explicit HostTable(size_t slots) : t(slots) { memset(t.data(), 0, slots * sizeof(SjSlot)); }
    // k_sj_insert's probe loop, one item at a time
    bool put(long long g1, long long g2, unsigned int cnt)
    {
        const unsigned long long w1 = sj_bias(g1), w2 = sj_bias(g2), mask = t.size() - 1;
        unsigned long long p = sj_hash(w1, w2) & mask;
        for (int k = 0; k < SJ_PROBES; k++, p = (p + 1) & mask) {
            SjSlot &s = t[p];
            if (s.k1 == 0) s.k1 = w1; else if (s.k1 != w1) continue;
            if (s.k2 == 0) { s.k2 = w2; distinct++; } else if (s.k2 != w2) continue;
            s.cnt += cnt;
            return true;
        }
        return false;
    }
    // the library's rule: the old slots and the overflow list into a table of twice the size, while an item found no slot or more than half the slots hold a key
    void add(std::vector<dg_sj_entry> items)
    {
        std::vector<dg_sj_entry> ovf;
        for (const dg_sj_entry &e : items) if (e.count && !put(e.g1, e.g2, e.count)) ovf.push_back(e);
        while (!ovf.empty() || distinct > t.size() / 2) {
            std::vector<SjSlot> old; old.swap(t);
            t.assign(old.size() * 2, SjSlot{0, 0, 0, 0}); distinct = 0; growths++;
            std::vector<dg_sj_entry> next;
            for (const SjSlot &s : old) if (s.k1 && s.k2 && !put(sj_unbias(s.k1), sj_unbias(s.k2), s.cnt)) next.push_back(dg_sj_entry{sj_unbias(s.k1), sj_unbias(s.k2), s.cnt, 0});
            for (const dg_sj_entry &e : ovf) if (!put(e.g1, e.g2, e.count)) next.push_back(e);
            ovf.swap(next);
        }
    }
};

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: sj_checks <input> <output>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<unsigned char> raw;
    { unsigned char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + k); fclose(f); }
    size_t at = 0;
    auto take = [&](size_t bytes) { const unsigned char *p = raw.data() + at; at += (bytes + 7) & ~(size_t)7; return p; };
    CHECK(raw.size() >= 32);
    long long head[4]; memcpy(head, take(32), 32);
    const size_t n = (size_t)head[0]; const int n_chr = (int)head[1]; const long long l_pac = head[2]; const size_t slots = (size_t)head[3];
    CHECK(n_chr > 0 && slots >= SJ_MIN_SLOTS && (slots & (slots - 1)) == 0);
    std::vector<int64_t> off(n_chr), len(n_chr); std::vector<uint32_t> noff(n_chr + 1);
    memcpy(off.data(), take(8 * n_chr), 8 * n_chr); memcpy(len.data(), take(8 * n_chr), 8 * n_chr); memcpy(noff.data(), take(4 * (n_chr + 1)), 4 * (n_chr + 1));
    std::vector<char> names(noff[n_chr] + 1); memcpy(names.data(), take(noff[n_chr]), noff[n_chr]);
    std::vector<dg_sj_entry> items(n);
    if (n) memcpy(items.data(), take(n * sizeof(dg_sj_entry)), n * sizeof(dg_sj_entry));
    CHECK(at <= raw.size());

    // the key words: unsigned order of the words = signed order of the coordinates; 0 stands for INT64_MIN alone
    for (size_t i = 0; i + 1 < n; i++) {
        const dg_sj_entry &a = items[i], &b = items[i + 1];
        CHECK(sj_unbias(sj_bias(a.g1)) == a.g1 && sj_key_ok(a.g1, a.g2));
        const bool less = sj_key_less(a.g1, a.g2, b.g1, b.g2);
        const bool wless = sj_bias(a.g1) != sj_bias(b.g1) ? sj_bias(a.g1) < sj_bias(b.g1) : sj_bias(a.g2) < sj_bias(b.g2);
        CHECK(less == wless);
    }
    CHECK(!sj_key_ok(INT64_MIN, 0) && !sj_key_ok(0, INT64_MIN) && sj_key_ok(-1, INT64_MAX));
    CHECK(sj_key_bits(5, 5) == 0 && sj_key_bits(4, 5) == 1 && sj_key_bits(0, ~0ull) == 64 && sj_key_bits(sj_bias(-1), sj_bias(0)) == 64);

    HostTable tab(slots);
    tab.add(items);
    std::vector<dg_sj_entry> ent;
    for (const SjSlot &s : tab.t) if (s.k1 && s.k2) ent.push_back(dg_sj_entry{sj_unbias(s.k1), sj_unbias(s.k2), s.cnt, 0});
    CHECK(ent.size() == tab.distinct);
    std::sort(ent.begin(), ent.end(), [](const dg_sj_entry &a, const dg_sj_entry &b) { return sj_key_less(a.g1, a.g2, b.g1, b.g2); });

    // the boundary keys as dg_init lays them out
    std::vector<int64_t> key(2 * n_chr); std::vector<int32_t> who(2 * n_chr);
    for (int i = 0; i < n_chr; i++) { key[i] = off[i] + len[i] - 1; who[i] = i; key[2 * n_chr - 1 - i] = 2 * l_pac - off[i] - 1; who[2 * n_chr - 1 - i] = i; }
    const LocTab lt{key.data(), who.data(), off.data(), 2 * n_chr};
    std::vector<char> text; size_t lines = 0;
    for (dg_sj_entry &e : ent) {
        e.chr = sj_chr_of(lt, e.g1);
        if (e.chr == SJ_NO_CHR) continue;
        const uint32_t want = sj_line_len(noff.data(), e.chr, off[e.chr], e.g1, e.g2, e.count);
        const size_t p = text.size();
        text.resize(p + want);
        CHECK(sj_line_write(text.data() + p, noff.data(), names.data(), e.chr, off[e.chr], e.g1, e.g2, e.count) == want);
        lines++;
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    const unsigned long long tail[4] = {ent.size(), lines, text.size(), tab.growths};
    fwrite(tail, 8, 4, f);
    if (!ent.empty()) fwrite(ent.data(), sizeof(dg_sj_entry), ent.size(), f);
    if (!text.empty()) fwrite(text.data(), 1, text.size(), f);
    fclose(f);
    return 0;
}
