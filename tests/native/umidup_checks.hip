// tests/native/umidup_checks.hip -- the host-callable code of the device's UMI-aware duplicate marking (dart_amd/csrc/dg_umidup.h over dg_markdup.h) run on the
// CPU, step by step as the kernels apply it: a record's filter, end key, score, hash and U from one pass over its name, the candidates' sort and the mate search,
// the pairs and ends in index order, their stable sorts key by key with U among the keys, the head tests, the marks, groups and families, the walk of a
// family's groups (one by one here, where the kernel lets 64 lanes test at once), and the byte that is written.
// usage: umidup_checks <input> <output.txt> <output.bin>
//   input       i64 n_chr, hash_bits, n_raw, max_edit, sep; the records
//   output.txt  per record "rec <i> <examined> <candidate> <E> <score> <h> <U>"; "bad <i>" for the first record out of range (then nothing else follows, and
//               output.bin holds the input's bytes); per examined record "dup <i> <0|1>"; "stats" and the twelve
//   output.bin  the marked array
#include "../../dart_amd/csrc/dg_umidup.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "umidup_checks: %s failed (line %d)\n", #x, __LINE__); exit(2); } } while (0)

// one stable sort by the low `bits` bits of the key, as rs_sort_passes leaves it
static void sort_by(std::vector<uint64_t> &keys, std::vector<int64_t> &vals, int bits)
{
    const size_t n = keys.size();
    std::vector<uint32_t> order(n);
    for (size_t k = 0; k < n; k++) { order[k] = (uint32_t)k; CHECK(bits >= 64 || (keys[k] >> bits) == 0); }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    std::vector<uint64_t> k2(n); std::vector<int64_t> v2(n);
    for (size_t k = 0; k < n; k++) { k2[k] = keys[order[k]]; v2[k] = vals[order[k]]; }
    keys.swap(k2); vals.swap(v2);
}

struct Lists { std::vector<uint64_t> E, U; std::vector<uint32_t> score, mate; };
struct ListStats { uint64_t multi = 0, crowded = 0, absorbed = 0, largest = 0, dups = 0; };

// k_ud_heads .. k_ud_flag over one sorted list; write(i, dup) takes the verdicts
template <class W>
static ListStats verdicts(const std::vector<uint64_t> &keys, const std::vector<int64_t> &vals, int ends, uint32_t max_edit, const Lists &L, W write)
{
    ListStats st;
    const uint32_t n_items = (uint32_t)keys.size();
    if (!n_items) return st;
    // k_ud_heads: the marks, with the scan per workgroup of MD_THREADS; k_ud_groups
    std::vector<uint32_t> mark(n_items), grp_of(n_items), gpos(n_items + 1), ffirst(n_items + 1);
    std::vector<uint64_t> head_base;
    std::vector<unsigned char> win(n_items, 0);
    uint64_t total = 0, in_tile = 0;
    for (uint32_t q = 0; q < n_items; q++) {
        if (q % MD_THREADS == 0) { head_base.push_back(total); in_tile = 0; }
        const bool fh = ud_family_head(keys.data(), vals.data(), q, ends, L.E.data(), L.mate.data());
        const bool gh = fh || ud_group_head(keys.data(), vals.data(), q, ends, L.E.data(), L.mate.data(), L.U.data());
        mark[q] = ud_mark(in_tile, fh, gh);
        const uint64_t add = (fh ? 1ull << 32 : 0ull) | (gh ? 1ull : 0ull);
        in_tile += add; total += add;
    }
    const uint32_t n_fam = (uint32_t)(total >> 32), n_grp = (uint32_t)total;
    for (uint32_t q = 0; q < n_items; q++) {
        const uint32_t m = mark[q], gh = m >> 30 & 1u, fh = m >> 31;
        const uint64_t base = head_base[q / MD_THREADS];
        const uint32_t g_incl = (uint32_t)base + ud_mark_groups(m) + gh, f_incl = (uint32_t)(base >> 32) + ud_mark_fams(m) + fh;
        CHECK(g_incl >= 1 && f_incl >= 1 && g_incl <= q + 1 && f_incl <= g_incl);
        grp_of[q] = g_incl - 1;
        if (gh) { gpos[g_incl - 1] = q; win[g_incl - 1] = 1; }
        if (fh) ffirst[f_incl - 1] = g_incl - 1;
        if (q + 1 == n_items) { CHECK(g_incl == n_grp && f_incl == n_fam); gpos[g_incl] = n_items; ffirst[f_incl] = g_incl; }
    }
    // k_ud_fams / k_ud_worklist / k_ud_cluster
    for (uint32_t f = 0; f < n_fam; f++) {
        const uint32_t g0 = ffirst[f], ng = ffirst[f + 1] - g0;
        CHECK(ng >= 1);
        st.multi += ng > 1 ? 1 : 0; st.crowded += ng > UD_FAMILY ? 1 : 0;
        if (!ud_family_is_work(ng, max_edit)) continue;
        std::vector<uint64_t> U(ng), cnt(ng), rank(ng);
        std::vector<uint32_t> place(ng, 0), at(ng), root(ng);
        for (uint32_t l = 0; l < ng; l++) {
            const uint32_t q = gpos[g0 + l];
            const int64_t v = vals[q];
            cnt[l] = gpos[g0 + l + 1] - q; U[l] = L.U[md_end_record(v)];
            rank[l] = ends ? ud_end_rank(v, L.score.data()) : ud_pair_rank((uint32_t)v, L.score.data(), L.mate.data());
            root[l] = l;
        }
        for (uint32_t l = 0; l < ng; l++) for (uint32_t m = 0; m < ng; m++) if (m != l && ud_before(cnt[m], U[m], cnt[l], U[l])) place[l]++;
        for (uint32_t l = 0; l < ng; l++) at[place[l]] = l;
        for (uint32_t r = 0; r < ng; r++) {
            const uint32_t src = at[r];
            if (root[src] != src) continue;
            for (uint32_t l = 0; l < ng; l++) if (root[l] == l && place[l] > r && ud_joins(U[src], cnt[src], U[l], cnt[l])) root[l] = src;
        }
        for (uint32_t l = 0; l < ng; l++) {
            uint32_t best = l; uint64_t sum = 0;
            for (uint32_t m = 0; m < ng; m++) if (root[m] == root[l]) { sum += cnt[m]; if (rank[m] < rank[best] || (rank[m] == rank[best] && m < best)) best = m; }
            win[g0 + l] = best == l ? 1 : 0;
            st.absorbed += root[l] != l ? 1 : 0;
            st.largest = std::max<uint64_t>(st.largest, sum);
        }
    }
    // k_ud_flag
    for (uint32_t q = 0; q < n_items; q++) {
        const uint32_t g = grp_of[q];
        const bool dup = ud_is_dup(gpos[g] == q, win[g] != 0);
        st.largest = std::max<uint64_t>(st.largest, q - gpos[g] + 1);
        if (!ends) { st.dups += dup ? 1 : 0; CHECK(write((uint32_t)vals[q], dup) && write(L.mate[(uint32_t)vals[q]], dup)); }
        else if (vals[q] >= 0) { st.dups += dup ? 1 : 0; CHECK(write((uint32_t)vals[q], dup)); }
    }
    return st;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: umidup_checks <input> <output.txt> <output.bin>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<unsigned char> in;
    { unsigned char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k); fclose(f); }
    CHECK(in.size() >= 40);
    long long head[5]; memcpy(head, in.data(), 40);
    const int n_chr = (int)head[0], hash_bits = (int)head[1];
    const uint64_t n_raw = (uint64_t)head[2];
    const uint32_t max_edit = (uint32_t)head[3];
    const unsigned char sep = (unsigned char)head[4];
    CHECK(n_chr >= 1 && hash_bits >= 1 && hash_bits <= MD_HASH_BITS && max_edit <= 1 && sep != 0 && in.size() == 40 + n_raw);
    // (an exact-size copy on the heap: a read that leaves the array leaves its allocation, which the sanitizer build sees)
    std::vector<unsigned char> raw(in.begin() + 40, in.end());
    FILE *txt = fopen(argv[2], "w"), *bin = fopen(argv[3], "wb");
    CHECK(txt && bin);
    std::vector<uint64_t> dst_off, tile_base;
    for (uint64_t p = 0; p < n_raw;) {
        CHECK(p + 4 <= n_raw);
        if (dst_off.size() % BS_THREADS == 0) tile_base.push_back(p);
        dst_off.push_back(p - tile_base.back());
        p += 4ull + bs_le32(raw.data() + p); CHECK(p <= n_raw);
    }
    const size_t n = dst_off.size();
    // k_ud_rec
    Lists L; L.E.resize(n); L.U.resize(n); L.score.resize(n); L.mate.resize(n);
    std::vector<uint64_t> ck; std::vector<int64_t> cvl;
    uint64_t examined = 0, bad = ~0ull, with_umi = 0, u_max = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t at = md_rec_start(dst_off.data(), tile_base.data(), (uint32_t)i);
        const UdRec u = ud_record(raw.data() + at, n_raw - at, n_chr, hash_bits, sep);
        if (u.r.bad && bad == ~0ull) bad = i;
        L.E[i] = u.r.E; L.U[i] = u.U; L.score[i] = u.r.score; L.mate[i] = u.r.examined ? MD_FRAGMENT : MD_NOT_EXAMINED;
        examined += u.r.examined ? 1 : 0; with_umi += u.U ? 1 : 0; u_max = std::max(u_max, u.U);
        if (u.r.candidate) { CHECK(u.r.examined); ck.push_back(u.r.h); cvl.push_back((int64_t)i); }
        // the one pass over the name gives what md_record's own hash gives
        if (!u.r.bad) { const MdRec r = md_record(raw.data() + at, n_raw - at, n_chr, hash_bits); CHECK(r.h == u.r.h && r.E == u.r.E && r.score == u.r.score && r.examined == u.r.examined && r.candidate == u.r.candidate); }
        fprintf(txt, "rec %zu %d %d %llu %u %llu %llu\n", i, (int)u.r.examined, (int)u.r.candidate, (unsigned long long)u.r.E, u.r.score, (unsigned long long)u.r.h, (unsigned long long)u.U);
    }
    if (bad != ~0ull) {
        fprintf(txt, "bad %llu\n", (unsigned long long)bad);
        CHECK(fwrite(raw.data(), 1, raw.size(), bin) == raw.size());
        fclose(txt); fclose(bin);
        return 0;
    }
    const int umi_bits = ud_umi_bits(u_max);
    CHECK(umi_bits <= 63);
    // the candidates' sort and k_md_mate
    sort_by(ck, cvl, hash_bits);
    const uint32_t n_cand = (uint32_t)ck.size();
    uint64_t crowded = 0;
    for (uint32_t j = 0; j < n_cand; j++) {
        bool cr = false;
        L.mate[(size_t)cvl[j]] = md_mate(ck.data(), cvl.data(), n_cand, j, raw.data(), dst_off.data(), tile_base.data(), &cr);
        crowded += cr ? 1 : 0;
    }
    // k_md_count / k_md_emit
    std::vector<uint64_t> pk, ek; std::vector<int64_t> pv, ev;
    for (size_t i = 0; i < n; i++) {
        const uint32_t m = L.mate[i];
        if (m == MD_NOT_EXAMINED) continue;
        if (m == MD_FRAGMENT) { ek.push_back(md_end_score_key(false, L.score[i])); ev.push_back((int64_t)i); continue; }
        CHECK(m < n && L.mate[m] == (uint32_t)i && L.U[m] == L.U[i]);
        if (!md_is_rep((uint32_t)i, m)) continue;
        pk.push_back(md_pair_score_key(L.score[i], L.score[m])); pv.push_back((int64_t)i);
        ek.push_back(md_end_score_key(true, 0)); ev.push_back(~(int64_t)i); ek.push_back(md_end_score_key(true, 0)); ev.push_back(~(int64_t)m);
    }
    const size_t n_pairs = pk.size(), n_ends = ek.size();
    CHECK(n_ends == examined);
    // the sorts, key by key
    const int e_bits = md_e_bits(n_chr);
    sort_by(pk, pv, MD_SCORE_BITS);
    if (umi_bits) { for (size_t q = 0; q < n_pairs; q++) pk[q] = L.U[(size_t)pv[q]]; sort_by(pk, pv, umi_bits); }
    for (size_t q = 0; q < n_pairs; q++) pk[q] = md_hi(L.E[(size_t)pv[q]], L.E[L.mate[(size_t)pv[q]]]);
    sort_by(pk, pv, e_bits);
    for (size_t q = 0; q < n_pairs; q++) pk[q] = md_lo(L.E[(size_t)pv[q]], L.E[L.mate[(size_t)pv[q]]]);
    sort_by(pk, pv, e_bits);
    sort_by(ek, ev, MD_SCORE_BITS);
    if (umi_bits) { for (size_t q = 0; q < n_ends; q++) ek[q] = L.U[md_end_record(ev[q])]; sort_by(ek, ev, umi_bits); }
    for (size_t q = 0; q < n_ends; q++) ek[q] = L.E[md_end_record(ev[q])];
    sort_by(ek, ev, e_bits);
    // the verdicts: every examined record gets exactly one write
    std::vector<unsigned char> out(raw);
    std::vector<int> verdict(n, -1);
    auto write = [&](uint32_t i, bool dup) {
        const uint64_t at = md_rec_start(dst_off.data(), tile_base.data(), i) + 19;
        out[at] = md_verdict(out[at], dup);
        const int seen = verdict[i]; verdict[i] = dup ? 1 : 0;
        return seen == -1;
    };
    const ListStats P = verdicts(pk, pv, 0, max_edit, L, write), Q = verdicts(ek, ev, 1, max_edit, L, write);
    for (size_t i = 0; i < n; i++) {
        CHECK((verdict[i] >= 0) == (L.mate[i] != MD_NOT_EXAMINED));
        if (verdict[i] >= 0) fprintf(txt, "dup %zu %d\n", i, verdict[i]);
    }
    fprintf(txt, "stats %llu %zu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)examined, n_pairs, (unsigned long long)(examined - 2 * n_pairs), (unsigned long long)P.dups,
            (unsigned long long)Q.dups, (unsigned long long)crowded, (unsigned long long)(2 * P.dups + Q.dups), (unsigned long long)P.largest, (unsigned long long)with_umi,
            (unsigned long long)P.multi, (unsigned long long)(P.absorbed + Q.absorbed), (unsigned long long)(P.crowded + Q.crowded));
    CHECK(fwrite(out.data(), 1, out.size(), bin) == out.size());
    fclose(txt); fclose(bin);
    return 0;
}
