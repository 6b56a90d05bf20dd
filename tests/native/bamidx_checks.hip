// tests/native/bamidx_checks.hip -- the host-callable code of the device's BAM index (dart_amd/csrc/dg_bamidx.h) run on the CPU, step by step as the kernels
// apply it: a record's beg / end / bin / rlen and its virtual offset, the head test, the chunks sorted by (refID, bin) (here std::stable_sort over the same
// keys), the merge test, the fill rule and the byte offset of every element.  usage: bamidx_checks <input> <output.txt> <output.bai>
//   input       i64 n_chr, u64 first_block_offset, i64 n_raw, i64 n_blocks; n_blocks x u32 compressed sizes (padded to 8 bytes); the sorted records
//   output.txt  per record "rec <i> <beg> <end> <bin> <voff> <placed> <mapped>"; "bad <i>" for the first placed record that ends behind 2^29 (then nothing
//               else follows); per sorted chunk "chunk <key> <beg> <end>", after the merge "merged <key> <beg> <end>"; per window "lin <ref> <window> <voff>"
//   output.bai  the index
#include "../../dart_amd/csrc/dg_bamidx.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "bamidx_checks: %s failed (line %d)\n", #x, __LINE__); return 2; } } while (0)

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: bamidx_checks <input> <output.txt> <output.bai>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<unsigned char> in;
    { unsigned char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k); fclose(f); }
    CHECK(in.size() >= 32);
    long long head[4]; memcpy(head, in.data(), 32);
    const int n_chr = (int)head[0]; const uint64_t first = (uint64_t)head[1], n_raw = (uint64_t)head[2], n_blocks = (uint64_t)head[3];
    CHECK(n_chr >= 1 && n_blocks == (n_raw + BI_BLOCK - 1) / BI_BLOCK);
    const size_t sizes_bytes = (size_t)((n_blocks * 4 + 7) & ~7ull);
    CHECK(in.size() == 32 + sizes_bytes + n_raw);
    std::vector<uint32_t> sizes((size_t)n_blocks);
    if (n_blocks) memcpy(sizes.data(), in.data() + 32, (size_t)n_blocks * 4);
    // (an exact-size copy on the heap: a walk that leaves the array leaves the allocation, which the sanitizer build sees)
    std::vector<unsigned char> raw(in.begin() + 32 + (long)sizes_bytes, in.end());
    FILE *txt = fopen(argv[2], "w"), *bai = fopen(argv[3], "wb");
    CHECK(txt && bai);
    // k_bi_coff
    std::vector<uint64_t> coff((size_t)n_blocks + 1);
    coff[0] = first;
    for (uint64_t k = 0; k < n_blocks; k++) coff[k + 1] = coff[k] + sizes[k];
    CHECK(!(coff[n_blocks] >> 48));
    // the records' places (on the device: k_bs_len's scan)
    std::vector<uint64_t> at;
    for (uint64_t p = 0; p < n_raw;) { CHECK(p + 4 <= n_raw); at.push_back(p); p += 4ull + bs_le32(raw.data() + p); CHECK(p <= n_raw); }
    const size_t n = at.size();
    // k_bi_rec
    std::vector<uint64_t> key(n), voff(n + 1); std::vector<uint32_t> span(n);
    std::vector<uint64_t> ref((size_t)BI_REF_PLANES * n_chr, 0);
    for (int t = 0; t < n_chr; t++) ref[3 * (size_t)n_chr + t] = BI_NONE;
    uint64_t bad = BI_NONE;
    for (size_t i = 0; i < n; i++) {
        const BiRec r = bi_record(raw.data() + at[i], n_raw - at[i], n_chr);
        key[i] = bi_key(r); voff[i] = bi_voff(at[i], n_raw, coff.data(), n_blocks); span[i] = bi_span(r);
        fprintf(txt, "rec %zu %lld %lld %u %llu %d %d\n", i, r.beg, r.end, r.bin, (unsigned long long)voff[i], (int)r.placed, (int)r.mapped);
        if (!r.placed) continue;
        if (r.end > BI_MAX_END) { if (bad == BI_NONE) bad = i; continue; }
        uint64_t *p = ref.data() + r.refid;
        if (r.mapped) { p[n_chr]++; p[0] = std::max<uint64_t>(p[0], (uint64_t)((r.end - 1) >> 14) + 1); } else p[2 * (size_t)n_chr]++;
        p[3 * (size_t)n_chr] = std::min<uint64_t>(p[3 * (size_t)n_chr], i); p[4 * (size_t)n_chr] = std::max<uint64_t>(p[4 * (size_t)n_chr], i);
    }
    voff[n] = bi_voff(n_raw, n_raw, coff.data(), n_blocks);
    if (bad != BI_NONE) { fprintf(txt, "bad %llu\n", (unsigned long long)bad); fclose(txt); fclose(bai); return 0; }
    size_t n_placed = 0, n_lin = 0;
    std::vector<uint64_t> lin_at((size_t)n_chr + 1);
    for (int t = 0; t < n_chr; t++) { lin_at[(size_t)t] = n_lin; n_lin += (size_t)ref[(size_t)t]; n_placed += (size_t)(ref[(size_t)n_chr + t] + ref[2 * (size_t)n_chr + t]); }
    lin_at[(size_t)n_chr] = n_lin;
    // k_bi_lin
    std::vector<uint64_t> lin(n_lin, BI_NONE);
    for (size_t i = 0; i < n; i++) {
        if (!bi_span_mapped(span[i])) continue;
        const uint64_t t = key[i] >> 16;
        uint32_t skip_first = 1u, skip_last = 0u;                // (as k_bi_lin: the windows of the mapped record in front, same reference, are not stored again)
        if (i && bi_span_mapped(span[i - 1]) && key[i - 1] >> 16 == t) { skip_first = bi_span_first(span[i - 1]); skip_last = bi_span_last(span[i - 1]); }
        for (uint32_t w = bi_span_first(span[i]); w <= bi_span_last(span[i]); w++) {
            CHECK(lin_at[t] + w < lin_at[t + 1]);
            if (!bi_lin_covered(w, skip_first, skip_last)) lin[lin_at[t] + w] = std::min(lin[lin_at[t] + w], voff[i]);
        }
    }
    // k_bi_heads / k_bi_chunks
    std::vector<std::pair<uint64_t, int64_t>> ch; std::vector<uint32_t> chead;
    for (size_t i = 0; i < n; i++) if (bi_is_head(i ? key[i - 1] : BI_NONE, key[i], i == 0)) { ch.emplace_back(key[i], (int64_t)ch.size()); chead.push_back((uint32_t)i); }
    const size_t n_chunks = ch.size();
    chead.push_back((uint32_t)n_placed);
    const int bits = bi_key_bits(n_chr);
    for (auto &x : ch) CHECK(x.first >> bits == 0);                  // no key has a bit the sorter does not look at
    std::stable_sort(ch.begin(), ch.end(), [](const std::pair<uint64_t, int64_t> &a, const std::pair<uint64_t, int64_t> &b) { return a.first < b.first; });
    auto c_beg = [&](size_t j) { return voff[chead[(size_t)ch[j].second]]; };
    auto c_end = [&](size_t j) { return voff[chead[(size_t)ch[j].second + 1]]; };
    // k_bi_merge_scan / k_bi_merge_emit
    std::vector<uint32_t> mhead(n_chunks + 1), mbin(n_chunks + 1), binq(n_chunks + 1), ref_q((size_t)n_chr + 1, 0), ref_b((size_t)n_chr + 1, 0);
    uint32_t q = 0, b = 0;
    for (size_t j = 0; j < n_chunks; j++) {
        fprintf(txt, "chunk %llu %llu %llu\n", (unsigned long long)ch[j].first, (unsigned long long)c_beg(j), (unsigned long long)c_end(j));
        const bool bin_head = j == 0 || ch[j].first != ch[j - 1].first;
        const bool merged = !bin_head && bi_merges(c_end(j - 1), c_beg(j));
        const int64_t t = (int64_t)(ch[j].first >> 16), before = j ? (int64_t)(ch[j - 1].first >> 16) : -1;
        CHECK(t < n_chr);
        for (int64_t x = before + 1; x <= t; x++) { ref_q[(size_t)x] = q; ref_b[(size_t)x] = b; }
        if (!merged) { mhead[q] = (uint32_t)j; mbin[q] = b + (bin_head ? 1u : 0u) - 1u; }
        if (bin_head) binq[b] = q;
        q += merged ? 0u : 1u; b += bin_head ? 1u : 0u;
    }
    const uint32_t all_q = q, all_b = b;
    for (int64_t x = (n_chunks ? (int64_t)(ch[n_chunks - 1].first >> 16) : -1) + 1; x <= n_chr; x++) { ref_q[(size_t)x] = all_q; ref_b[(size_t)x] = all_b; }
    binq[all_b] = all_q; mhead[all_q] = (uint32_t)n_chunks;
    // k_bi_refs
    std::vector<uint64_t> ref_at((size_t)n_chr + 1);
    uint64_t total = 8;
    for (int t = 0; t < n_chr; t++) {
        ref_at[(size_t)t] = total;
        total += bi_ref_bytes(ref_b[(size_t)t + 1] - ref_b[(size_t)t], ref_q[(size_t)t + 1] - ref_q[(size_t)t], ref[(size_t)n_chr + t] + ref[2 * (size_t)n_chr + t] > 0, ref[(size_t)t]);
    }
    ref_at[(size_t)n_chr] = total; total += 8;
    CHECK(total <= bi_bytes_bound((uint64_t)n_chr, n_chunks, n_lin));
    // (exact size, and filled with a byte no field ends up as: a byte nobody wrote shows, a byte behind the end is the sanitizer's)
    std::vector<uint32_t> out_words((size_t)(total / 4), 0xA5A5A5A5u);
    unsigned char *out = (unsigned char *)out_words.data();
    bi_put_head(out, total, n_chr, total, n - n_placed);
    // k_bi_write_chunks
    for (uint32_t m = 0; m < all_q; m++) {
        const uint32_t j = mhead[m], j_next = mhead[m + 1], bb = mbin[m];
        const uint64_t t = ch[j].first >> 16;
        const uint64_t bin_in_ref = bb - ref_b[t], chunk_in_ref = m - ref_q[t], c = bi_chunk_at(ref_at[t], bin_in_ref, chunk_in_ref);
        bi_put64(out, total, c, c_beg(j)); bi_put64(out, total, c + 8, c_end(j_next - 1));
        fprintf(txt, "merged %llu %llu %llu\n", (unsigned long long)ch[j].first, (unsigned long long)c_beg(j), (unsigned long long)c_end(j_next - 1));
        if (binq[bb] == m) {
            const uint64_t h = bi_bin_at(ref_at[t], bin_in_ref, chunk_in_ref);
            bi_put32(out, total, h, (uint32_t)(ch[j].first & 0xffffu)); bi_put32(out, total, h + 4, binq[bb + 1] - m);
        }
    }
    // k_bi_write_refs
    for (int t = 0; t < n_chr; t++) {
        uint64_t r[BI_REF_PLANES];
        for (int p = 0; p < BI_REF_PLANES; p++) r[p] = ref[(size_t)p * n_chr + t];
        const bool has = r[1] + r[2] > 0;
        const uint64_t n_bins = ref_b[(size_t)t + 1] - ref_b[(size_t)t], n_ch = ref_q[(size_t)t + 1] - ref_q[(size_t)t];
        const uint64_t v_first = has ? voff[r[3]] : 0, v_last = has ? voff[r[4] + 1] : 0;
        bi_put_ref(out, total, ref_at[(size_t)t], n_bins, n_ch, r, v_first, v_last);
        const uint64_t dst = bi_intv_at(ref_at[(size_t)t], n_bins, n_ch, has) + 4;
        uint64_t carry = v_first;
        for (uint64_t w = 0; w < r[0]; w++) {
            carry = bi_fill(carry, lin[lin_at[(size_t)t] + w]);
            bi_put64(out, total, dst + 8 * w, carry);
            fprintf(txt, "lin %d %llu %llu\n", t, (unsigned long long)w, (unsigned long long)carry);
        }
    }
    CHECK(fwrite(out, 1, (size_t)total, bai) == (size_t)total);
    fclose(txt); fclose(bai);
    return 0;
}
