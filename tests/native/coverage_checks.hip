// tests/native/coverage_checks.hip -- the host-callable code of the device's coverage track (dart_amd/csrc/dg_coverage.h) run on the CPU, step by step as the
// kernels apply it: a record's filter and blocks, the two events per block, their sort (here std::stable_sort over the same keys), the 32-bit scan of the deltas,
// the tail and breakpoint tests with the last-valid fill, the marks, the entries and every line's length and bytes.
// usage: coverage_checks <input> <output.txt> <output.bedgraph>
//   input       i64 n_chr, flags, exclude_flags, min_mapq, n_raw, names_len; (n_chr + 1) x u32 name offsets (padded to 8 bytes); the names (padded to 8); the records
//   output.txt  per record "rec <i> <counted> <blocks>", per block "blk <record> <start> <end>"; "bad <i>" for the first record out of range (then nothing else
//               follows); per sorted event "ev <key> <delta>", per breakpoint "bp <key> <depth>", per entry "ent <chr> <start> <end> <depth>", "stats" and the seven
//   output.bedgraph  the text
#include "../../dart_amd/csrc/dg_coverage.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "coverage_checks: %s failed (line %d)\n", #x, __LINE__); return 2; } } while (0)

struct Print { FILE *txt; size_t rec; void operator()(uint32_t, uint64_t s, uint64_t e) { fprintf(txt, "blk %zu %llu %llu\n", rec, (unsigned long long)s, (unsigned long long)e); } };

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: coverage_checks <input> <output.txt> <output.bedgraph>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<unsigned char> in;
    { unsigned char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k); fclose(f); }
    CHECK(in.size() >= 48);
    long long head[6]; memcpy(head, in.data(), 48);
    const int n_chr = (int)head[0]; const CvFilter flt{(uint32_t)head[1], (uint32_t)head[2], (uint32_t)head[3]};
    const uint64_t n_raw = (uint64_t)head[4], names_len = (uint64_t)head[5];
    CHECK(n_chr >= 1);
    const size_t off_bytes = (size_t)((((size_t)n_chr + 1) * 4 + 7) & ~7ull), names_bytes = (size_t)((names_len + 7) & ~7ull);
    CHECK(in.size() == 48 + off_bytes + names_bytes + n_raw);
    // (exact-size copies on the heap: a read that leaves an array leaves its allocation, which the sanitizer build sees)
    std::vector<uint32_t> name_off((size_t)n_chr + 1); memcpy(name_off.data(), in.data() + 48, ((size_t)n_chr + 1) * 4);
    std::vector<char> names(in.begin() + 48 + (long)off_bytes, in.begin() + 48 + (long)off_bytes + (long)names_len);
    std::vector<unsigned char> raw(in.begin() + 48 + (long)(off_bytes + names_bytes), in.end());
    CHECK(name_off[(size_t)n_chr] == names_len);
    FILE *txt = fopen(argv[2], "w"), *bed = fopen(argv[3], "wb");
    CHECK(txt && bed);
    // the records' places (on the device: k_bs_len's scan)
    std::vector<uint64_t> at;
    for (uint64_t p = 0; p < n_raw;) { CHECK(p + 4 <= n_raw); at.push_back(p); p += 4ull + bs_le32(raw.data() + p); CHECK(p <= n_raw); }
    const size_t n = at.size();
    // k_cv_count
    std::vector<uint64_t> first(n + 1, 0);
    uint64_t counted = 0, aligned = 0, bad = CV_NONE, kmin = CV_NONE, kmax = 0;
    for (size_t i = 0; i < n; i++) {
        const CvRec r = cv_record(raw.data() + at[i], n_raw - at[i], n_chr, flt);
        uint32_t nb = 0;
        if (r.counted) {
            CvTally t; t.aligned = 0; t.lo = CV_NONE; t.hi = 0; t.bad = false;
            nb = cv_blocks(raw.data() + at[i], r, t);
            counted++;
            if (t.bad) { if (bad == CV_NONE) bad = i; }
            else if (nb) { aligned += t.aligned; kmin = std::min(kmin, cv_key(r.refid, t.lo)); kmax = std::max(kmax, cv_key(r.refid, t.hi)); }
            Print pr{txt, i};
            (void)cv_blocks(raw.data() + at[i], r, pr);
        }
        fprintf(txt, "rec %zu %d %u\n", i, (int)r.counted, nb);
        first[i + 1] = first[i] + nb;
    }
    if (bad != CV_NONE) { fprintf(txt, "bad %llu\n", (unsigned long long)bad); fclose(txt); fclose(bed); return 0; }
    const uint64_t n_blocks = first[n], n_ev = 2 * n_blocks;
    // k_cv_emit: exact-size arrays, every slot written exactly once
    std::vector<uint64_t> keys((size_t)n_ev, CV_NONE); std::vector<int64_t> vals((size_t)n_ev, 0);
    for (size_t i = 0; i < n; i++) {
        const CvRec r = cv_record(raw.data() + at[i], n_raw - at[i], n_chr, flt);
        if (!r.counted) continue;
        CvEmit e{keys.data(), vals.data(), first[i], n_blocks, r.refid};
        CHECK(cv_blocks(raw.data() + at[i], r, e) == first[i + 1] - first[i]);
    }
    for (uint64_t k = 0; k < n_ev; k++) CHECK(vals[k] == (k & 1 ? -1 : 1) && keys[k] != CV_NONE);
    // the sort: no key differs from another in a bit the sorter does not look at
    const int bits = n_ev ? std::min(cv_key_bits(kmin, kmax), cv_key_bits_max(n_chr)) : 0;
    for (uint64_t k = 0; k < n_ev; k++) CHECK(bits >= 64 || (keys[k] >> bits) == (kmin >> bits));
    std::vector<uint32_t> order((size_t)n_ev);
    for (uint64_t k = 0; k < n_ev; k++) order[k] = (uint32_t)k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    std::vector<uint64_t> skey((size_t)n_ev); std::vector<int64_t> sval((size_t)n_ev);
    for (uint64_t k = 0; k < n_ev; k++) { skey[k] = keys[order[k]]; sval[k] = vals[order[k]]; fprintf(txt, "ev %llu %lld\n", (unsigned long long)skey[k], (long long)sval[k]); }
    // k_cv_depth (32 bit), k_cv_tails / k_cv_tails_top / k_cv_flag: the last-valid fill, the breakpoint test, the marks of a workgroup's events
    std::vector<uint64_t> bp_key; std::vector<uint32_t> bp_depth, ent_bp;
    uint32_t depth = 0; uint64_t prev_tail = 0, deepest = 0;
    uint32_t in_wg_bp = 0, in_wg_ent = 0;
    for (uint64_t k = 0; k < n_ev; k++) {
        if (k % CV_THREADS == 0) { in_wg_bp = 0; in_wg_ent = 0; }
        depth += (uint32_t)sval[k];
        const bool tail = cv_is_tail(skey[k], k + 1 < n_ev ? skey[k + 1] : 0ull, k + 1 == n_ev);
        const uint64_t own = tail ? (uint64_t)depth : CV_NONE;
        const bool bp = cv_is_breakpoint(tail, depth, (uint32_t)prev_tail), ent = bp && depth > 0u;
        const uint32_t m = cv_mark(in_wg_bp | in_wg_ent << 16, bp, ent);
        CHECK(cv_mark_bps(m) == in_wg_bp && cv_mark_ents(m) == in_wg_ent && (m >> 30 & 1u) == (bp ? 1u : 0u) && (m >> 31) == (ent ? 1u : 0u));
        if (bp) { if (ent) ent_bp.push_back((uint32_t)bp_key.size()); bp_key.push_back(skey[k]); bp_depth.push_back(depth); fprintf(txt, "bp %llu %u\n", (unsigned long long)skey[k], depth); }
        in_wg_bp += bp ? 1u : 0u; in_wg_ent += ent ? 1u : 0u;
        prev_tail = cv_fill(prev_tail, own);
        if (tail && depth > deepest) deepest = depth;
    }
    CHECK(depth == 0u);
    // k_cv_entries / k_cv_write: the text has exactly the scanned size; a byte nobody wrote shows, a byte behind the end is the sanitizer's
    const size_t n_ent = ent_bp.size();
    std::vector<dg_cov_entry> entries(n_ent); std::vector<uint64_t> line_at(n_ent + 1, 0);
    uint64_t covered = 0, area = 0;
    for (size_t j = 0; j < n_ent; j++) {
        const uint32_t q = ent_bp[j];
        CHECK((size_t)q + 1 < bp_key.size());
        entries[j] = cv_entry(bp_key[q], bp_key[q + 1], bp_depth[q]);
        CHECK(entries[j].chr < (uint32_t)n_chr && entries[j].chr == (uint32_t)(bp_key[q + 1] >> 32) && entries[j].end > entries[j].start);
        covered += entries[j].end - entries[j].start; area += (uint64_t)(entries[j].end - entries[j].start) * entries[j].depth;
        const uint32_t len = cv_line_len(name_off.data(), entries[j]);
        CHECK(len <= cv_line_bound((uint32_t)names_len));
        line_at[j + 1] = line_at[j] + len;
        fprintf(txt, "ent %u %u %u %u\n", entries[j].chr, entries[j].start, entries[j].end, entries[j].depth);
    }
    CHECK(area == aligned);
    std::vector<char> text((size_t)line_at[n_ent], (char)0xA5);
    for (size_t j = 0; j < n_ent; j++) CHECK(cv_line_write(text.data() + line_at[j], name_off.data(), names.data(), entries[j]) == line_at[j + 1] - line_at[j]);
    fprintf(txt, "stats %llu %llu %zu %zu %llu %llu %llu\n", (unsigned long long)counted, (unsigned long long)n_blocks, bp_key.size(), n_ent, (unsigned long long)covered,
            (unsigned long long)aligned, (unsigned long long)deepest);
    CHECK(fwrite(text.data(), 1, text.size(), bed) == text.size());
    fclose(txt); fclose(bed);
    return 0;
}
