// tests/native/bamsort_checks.hip -- the host-callable code of the device's coordinate sort (dart_amd/csrc/dg_bamsort.h) run on the CPU: the key of a
// record, the checked walk over records from outside, the walk over a read's byte range, the segment order, and the final order the library's stable sort
// leaves (here std::stable_sort over the same keys in the same arrangement).  usage: bamsort_checks <input> <output.txt> <output.bin>
//   input       i64 n_chr, n_segments; per segment: i64 ordinal, n_bytes, then the bytes (every item padded to 8 bytes)
//   output.txt  per segment "seg <i> why <code> bad <index> n <records> range <records the range walk finds>", per record "rec <key> <offset>";
//               "order <segment indices>", "bits <key bits>", "sorted <records> <bytes>"
//   output.bin  the records of all accepted segments in sorted order
#include "../../dart_amd/csrc/dg_bamsort.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "bamsort_checks: %s failed (line %d)\n", #x, __LINE__); return 2; } } while (0)

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: bamsort_checks <input> <output.txt> <output.bin>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<unsigned char> raw;
    { unsigned char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + k); fclose(f); }
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += (bytes + 7) & ~(size_t)7; return here; };
    CHECK(raw.size() >= 16);
    long long head[2]; memcpy(head, raw.data() + take(16), 16);
    const int n_chr = (int)head[0]; const size_t n_seg = (size_t)head[1];
    FILE *txt = fopen(argv[2], "w"), *bin = fopen(argv[3], "wb");
    CHECK(txt && bin);
    // the store as the library keeps it: the bytes of the accepted segments one behind the other, a key and an offset per record, the segment list
    std::vector<unsigned char> store; std::vector<uint64_t> keys; std::vector<int64_t> offs; std::vector<BsSeg> segs; std::vector<size_t> seg_of;
    for (size_t s = 0; s < n_seg; s++) {
        CHECK(at + 16 <= raw.size());
        long long sh[2]; memcpy(sh, raw.data() + take(16), 16);
        const size_t n = (size_t)sh[1];
        CHECK(at + n <= raw.size());
        // (an exact-size copy on the heap: a walk that leaves the segment leaves the allocation, which the sanitizer build sees)
        std::vector<unsigned char> seg(raw.begin() + (long)at, raw.begin() + (long)(at + n));
        (void)take(n);
        std::vector<uint64_t> k2; std::vector<int64_t> o2;
        size_t bad = 0; int why = 0;
        const unsigned char *p = seg.data();
        const uint64_t base = store.size();
        const size_t cnt = bs_walk_checked(p, n, n_chr, &bad, &why, [&](size_t, size_t a) { k2.push_back(bs_key(p + a, n_chr)); o2.push_back((int64_t)(base + a)); });
        const uint32_t in_range = bs_range_walk(p, 0, n, BsNoop());
        fprintf(txt, "seg %zu why %d bad %zu n %zu range %u\n", s, why, why ? bad : (size_t)0, cnt, in_range);
        if (why) continue;                                     // refused: nothing is added
        // the emit functor of k_bs_emit over the same range must leave the same keys and offsets
        std::vector<uint64_t> k3(cnt, 0); std::vector<int64_t> o3(cnt, 0);
        const BsEmit e{p, k3.data(), o3.data(), 0, cnt, base, n_chr};
        CHECK(bs_range_walk(p, 0, n, e) == cnt && k3 == k2 && o3 == o2);
        for (size_t i = 0; i < cnt; i++) fprintf(txt, "rec %llu %lld\n", (unsigned long long)k2[i], (long long)o2[i]);
        segs.push_back(BsSeg{(uint32_t)sh[0], (uint64_t)keys.size(), (uint64_t)cnt});
        seg_of.push_back(s);
        keys.insert(keys.end(), k2.begin(), k2.end()); offs.insert(offs.end(), o2.begin(), o2.end());
        store.insert(store.end(), seg.begin(), seg.end());
    }
    std::vector<uint32_t> order(segs.size());
    bs_order_segments(segs.data(), segs.size(), order.data());
    fprintf(txt, "order");
    for (uint32_t o : order) fprintf(txt, " %zu", seg_of[o]);
    fprintf(txt, "\nbits %d\n", bs_key_bits(n_chr));
    // dg_bam_sort_finish: keys and offsets in segment order, one stable sort by the low bs_key_bits bits, the gather
    std::vector<std::pair<uint64_t, int64_t>> kv;
    for (uint32_t o : order) for (uint64_t i = 0; i < segs[o].count; i++) kv.emplace_back(keys[segs[o].start + i], offs[segs[o].start + i]);
    const int bits = bs_key_bits(n_chr);
    const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1ull;
    for (auto &x : kv) CHECK((x.first & mask) == x.first);     // no key has a bit the sorter does not look at
    std::stable_sort(kv.begin(), kv.end(), [](const std::pair<uint64_t, int64_t> &a, const std::pair<uint64_t, int64_t> &b) { return a.first < b.first; });
    size_t out_bytes = 0;
    for (auto &x : kv) {
        const size_t len = 4 + (size_t)bs_le32(store.data() + x.second);
        CHECK((size_t)x.second + len <= store.size());
        CHECK(fwrite(store.data() + x.second, 1, len, bin) == len);
        out_bytes += len;
    }
    CHECK(out_bytes == store.size());
    fprintf(txt, "sorted %zu %zu\n", kv.size(), out_bytes);
    fclose(txt); fclose(bin);
    return 0;
}
