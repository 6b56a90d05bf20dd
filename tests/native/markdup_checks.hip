// tests/native/markdup_checks.hip -- the host-callable code of the device's duplicate marking (dart_amd/csrc/dg_markdup.h) run on the CPU, step by step as the
// kernels apply it: a record's filter, end key, score and hash, the candidates' sort (here std::stable_sort over the same keys), the mate search, the pairs and
// ends in index order, their stable sorts key by key, the head tests and the byte that is written.
// usage: markdup_checks <input> <output.txt> <output.bin>
//   input       i64 n_chr, hash_bits, n_raw; the records
//   output.txt  per record "rec <i> <examined> <candidate> <E> <score> <h>"; "bad <i>" for the first record out of range (then nothing else follows, and
//               output.bin holds the input's bytes); per examined record "mate <i> <partner or -1>" and "dup <i> <0|1>"; "stats" and the eight
//   output.bin  the marked array
#include "../../dart_amd/csrc/dg_markdup.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "markdup_checks: %s failed (line %d)\n", #x, __LINE__); return 2; } } while (0)

// one stable sort by the low `bits` bits of the key, as rs_sort_passes leaves it
static void sort_by(std::vector<uint64_t> &keys, std::vector<int64_t> &vals, int bits)
{
    const size_t n = keys.size();
    std::vector<uint32_t> order(n);
    for (size_t k = 0; k < n; k++) { order[k] = (uint32_t)k; if (bits < 64 && (keys[k] >> bits) != 0) { fprintf(stderr, "markdup_checks: a key has a bit above %d\n", bits); exit(2); } }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    std::vector<uint64_t> k2(n); std::vector<int64_t> v2(n);
    for (size_t k = 0; k < n; k++) { k2[k] = keys[order[k]]; v2[k] = vals[order[k]]; }
    keys.swap(k2); vals.swap(v2);
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: markdup_checks <input> <output.txt> <output.bin>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<unsigned char> in;
    { unsigned char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k); fclose(f); }
    CHECK(in.size() >= 24);
    long long head[3]; memcpy(head, in.data(), 24);
    const int n_chr = (int)head[0], hash_bits = (int)head[1];
    const uint64_t n_raw = (uint64_t)head[2];
    CHECK(n_chr >= 1 && hash_bits >= 1 && hash_bits <= MD_HASH_BITS && in.size() == 24 + n_raw);
    // (an exact-size copy on the heap: a read that leaves the array leaves its allocation, which the sanitizer build sees)
    std::vector<unsigned char> raw(in.begin() + 24, in.end());
    FILE *txt = fopen(argv[2], "w"), *bin = fopen(argv[3], "wb");
    CHECK(txt && bin);
    // the records' places as k_bs_len's scan leaves them: an offset inside the workgroup's tile, and the tiles' bases
    std::vector<uint64_t> dst_off, tile_base;
    for (uint64_t p = 0; p < n_raw;) {
        CHECK(p + 4 <= n_raw);
        if (dst_off.size() % BS_THREADS == 0) tile_base.push_back(p);
        dst_off.push_back(p - tile_base.back());
        p += 4ull + bs_le32(raw.data() + p); CHECK(p <= n_raw);
    }
    const size_t n = dst_off.size();
    // k_md_rec
    std::vector<uint64_t> E(n), h(n); std::vector<uint32_t> score(n), mate(n);
    std::vector<uint64_t> ck; std::vector<int64_t> cvl;
    uint64_t examined = 0, bad = ~0ull;
    for (size_t i = 0; i < n; i++) {
        const uint64_t at = md_rec_start(dst_off.data(), tile_base.data(), (uint32_t)i);
        const MdRec r = md_record(raw.data() + at, n_raw - at, n_chr, hash_bits);
        if (r.bad && bad == ~0ull) bad = i;
        E[i] = r.E; h[i] = r.h; score[i] = r.score; mate[i] = r.examined ? MD_FRAGMENT : MD_NOT_EXAMINED;
        examined += r.examined ? 1 : 0;
        if (r.candidate) { CHECK(r.examined); ck.push_back(r.h); cvl.push_back((int64_t)i); }
        fprintf(txt, "rec %zu %d %d %llu %u %llu\n", i, (int)r.examined, (int)r.candidate, (unsigned long long)r.E, r.score, (unsigned long long)r.h);
    }
    if (bad != ~0ull) {
        fprintf(txt, "bad %llu\n", (unsigned long long)bad);
        CHECK(fwrite(raw.data(), 1, raw.size(), bin) == raw.size());
        fclose(txt); fclose(bin);
        return 0;
    }
    // the candidates' sort and k_md_mate
    sort_by(ck, cvl, hash_bits);
    const uint32_t n_cand = (uint32_t)ck.size();
    uint64_t crowded = 0;
    for (uint32_t j = 0; j < n_cand; j++) {
        bool cr = false;
        const uint32_t m = md_mate(ck.data(), cvl.data(), n_cand, j, raw.data(), dst_off.data(), tile_base.data(), &cr);
        mate[(size_t)cvl[j]] = m;
        crowded += cr ? 1 : 0;
    }
    for (size_t i = 0; i < n; i++) if (mate[i] < MD_FRAGMENT) CHECK(mate[i] < n && mate[mate[i]] == (uint32_t)i && mate[i] != (uint32_t)i);
    // k_md_count / k_md_emit: exact-size lists in index order
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) total += md_counts((uint32_t)i, mate[i]);
    const size_t n_pairs = (size_t)(total >> 32), n_ends = (size_t)(uint32_t)total;
    CHECK(n_ends == examined && 2 * n_pairs <= n_cand);
    std::vector<uint64_t> pk, ek; std::vector<int64_t> pv, ev;
    for (size_t i = 0; i < n; i++) {
        const uint32_t m = mate[i];
        if (m == MD_NOT_EXAMINED) continue;
        if (m == MD_FRAGMENT) { ek.push_back(md_end_score_key(false, score[i])); ev.push_back((int64_t)i); continue; }
        if (!md_is_rep((uint32_t)i, m)) continue;
        pk.push_back(md_pair_score_key(score[i], score[m])); pv.push_back((int64_t)i);
        ek.push_back(md_end_score_key(true, 0)); ev.push_back(~(int64_t)i); ek.push_back(md_end_score_key(true, 0)); ev.push_back(~(int64_t)m);
    }
    CHECK(pk.size() == n_pairs && ek.size() == n_ends);
    // the pair sorts and the end sorts, key by key (k_md_rekey)
    const int e_bits = md_e_bits(n_chr);
    sort_by(pk, pv, MD_SCORE_BITS);
    for (size_t q = 0; q < n_pairs; q++) pk[q] = md_hi(E[(size_t)pv[q]], E[mate[(size_t)pv[q]]]);
    sort_by(pk, pv, e_bits);
    for (size_t q = 0; q < n_pairs; q++) pk[q] = md_lo(E[(size_t)pv[q]], E[mate[(size_t)pv[q]]]);
    sort_by(pk, pv, e_bits);
    sort_by(ek, ev, MD_SCORE_BITS);
    for (size_t q = 0; q < n_ends; q++) ek[q] = E[md_end_record(ev[q])];
    sort_by(ek, ev, e_bits);
    // k_md_heads / k_md_flag_pairs / k_md_flag_ends: every examined record gets exactly one write
    std::vector<unsigned char> out(raw);
    std::vector<int> verdict(n, -1);
    uint64_t dup_pairs = 0, dup_frags = 0, family = 0, first = 0;
    auto write = [&](uint32_t i, bool dup) {
        const uint64_t at = md_rec_start(dst_off.data(), tile_base.data(), i) + 19;
        out[at] = md_verdict(out[at], dup);
        const int seen = verdict[i]; verdict[i] = dup ? 1 : 0;
        return seen == -1;
    };
    for (size_t q = 0; q < n_pairs; q++) {
        const bool head = md_pair_is_head(pk.data(), pv.data(), (uint32_t)q, E.data(), mate.data());
        if (head) first = q;
        family = std::max<uint64_t>(family, q - first + 1);
        dup_pairs += head ? 0 : 1;
        const uint32_t i = (uint32_t)pv[q];
        CHECK(write(i, !head) && write(mate[i], !head));
    }
    for (size_t q = 0; q < n_ends; q++) {
        if (ev[q] < 0) continue;
        const bool dup = md_end_is_dup(ek.data(), ev.data(), (uint32_t)q);
        dup_frags += dup ? 1 : 0;
        CHECK(write((uint32_t)ev[q], dup));
    }
    for (size_t i = 0; i < n; i++) {
        CHECK((verdict[i] >= 0) == (mate[i] != MD_NOT_EXAMINED));
        if (verdict[i] >= 0) fprintf(txt, "mate %zu %lld\ndup %zu %d\n", i, mate[i] == MD_FRAGMENT ? -1ll : (long long)mate[i], i, verdict[i]);
    }
    fprintf(txt, "stats %llu %zu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)examined, n_pairs, (unsigned long long)(examined - 2 * n_pairs), (unsigned long long)dup_pairs,
            (unsigned long long)dup_frags, (unsigned long long)crowded, (unsigned long long)(2 * dup_pairs + dup_frags), (unsigned long long)family);
    CHECK(fwrite(out.data(), 1, out.size(), bin) == out.size());
    fclose(txt); fclose(bin);
    return 0;
}
