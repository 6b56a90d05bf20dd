// tests/native/txquant_checks.hip -- the host-callable code of the device's expression stage (dart_amd/csrc/dg_txquant.h) run on the CPU as the library and the
// kernels apply it: the flattening of the annotation, the check of host records, every unit's lane code in both passes (count, then write into a pool of
// exactly the counted size), the class building (hash, stable sort, heads against the predecessor's full list, the exact host build when hashes collide), a
// table folded into itself, the EM's rounds and the text.
// usage: txquant_checks <input> <output.txt> <table.txt>
//   input       16 x i64: n_chr, n_tx, n_exons, n_reads, n_pair_mode, min_mapq, n_reports, n_ops, strand_mode, hash_bits, frag_mean, max_rounds, scale (every
//               class count is multiplied by it in front of the EM), n_start (0, or n_tx: the EM begins from the S given at the end of the input instead of the
//               definition's start values -- a test's way into states those do not reach), 0, 0; then dg_rna_tx (32 bytes each), dg_rna_exon (8), dg_read_out,
//               dg_report_out, CIGAR words, each array padded to 8 bytes; then n_start u64
//   output.txt  "err <text>" when the annotation is refused (nothing else follows); "tx <t> <L> <merged exons>"; "seg <chr> <start> <ids ...>"; "bad <read>" for
//               the first read whose ranges leave the arrays (then nothing else follows); "unit <u> <outcome> <has_fl> <fl> <ids ...>"; "collision <0|1>";
//               "class <count> <ids ...>"; "words <8>"; "range" when N >= 2^33, else "res <n_tx + 16 words>"
//   table.txt   tx_format's text with the names T<t>
#include "../../dart_amd/csrc/dg_txquant.h"
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "txquant_checks: %s failed (line %d)\n", #x, __LINE__); return 2; } } while (0)

template <typename T> static std::vector<T> take(const std::vector<unsigned char> &in, size_t &at, size_t n)
{
    std::vector<T> v(n);                                  // (exact-size copies on the heap: a read that leaves an array leaves its allocation, which the sanitizer build sees)
    if (n) memcpy(v.data(), in.data() + at, n * sizeof(T));
    at += (n * sizeof(T) + 7) & ~(size_t)7;
    return v;
}
template <typename T> static std::vector<T> exact(const std::vector<T> &v) { return std::vector<T>(v.begin(), v.end()); }

// the device's class building over two item sources, on the CPU: -> the new table; collided: the exact host build finished it
static int build(const TxTwo &s, int hash_bits, TxHostTab &o, bool &collided)
{
    const uint64_t n = s.a.n + s.b.n, mask = tx_hash_mask(hash_bits);
    std::vector<uint64_t> keys(n); std::vector<int64_t> vals(n);
    for (uint64_t i = 0; i < n; i++) { keys[i] = tx_item_hash(s, i) & mask; vals[i] = (int64_t)i; }
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return keys[x] < keys[y]; });
    std::vector<uint64_t> sk(n); std::vector<int64_t> sv(n);
    for (size_t i = 0; i < n; i++) { sk[i] = keys[order[i]]; sv[i] = vals[order[i]]; }
    collided = false;
    std::vector<uint32_t> sz(n);
    for (uint64_t j = 0; j < n; j++) sz[j] = tx_head(s, sk.data(), sv.data(), j, collided);
    if (collided) { tx_build_host(s, o); return 0; }
    o.off.assign(1, 0ull); o.cnt.clear(); o.ids.clear();
    for (uint64_t j = 0; j < n; j++) {
        uint64_t len, cnt;
        const uint32_t *p = tx_item(s, (uint64_t)sv[j], len, cnt);
        if (sz[j]) { CHECK(sz[j] == len); o.ids.insert(o.ids.end(), p, p + len); o.off.push_back(o.ids.size()); o.cnt.push_back(0ull); }
        CHECK(!o.cnt.empty());
        o.cnt.back() += cnt;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: txquant_checks <input> <output.txt> <table.txt>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<unsigned char> in;
    { unsigned char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k); fclose(f); }
    CHECK(in.size() >= 128);
    long long head[16]; memcpy(head, in.data(), 128);
    const int n_chr = (int)head[0], n_reads = (int)head[3], n_pair_mode = (int)head[4], hash_bits = (int)head[9];
    const uint32_t n_tx = (uint32_t)head[1], min_mapq = (uint32_t)head[5], strand_mode = (uint32_t)head[8], max_rounds = (uint32_t)head[11];
    const size_t n_exons = (size_t)head[2], n_reports = (size_t)head[6], n_ops = (size_t)head[7];
    const unsigned long long frag_mean = (unsigned long long)head[10], scale = (unsigned long long)head[12];
    const size_t n_start = (size_t)head[13];
    static_assert(sizeof(dg_rna_tx) == 32 && sizeof(dg_rna_exon) == 8 && sizeof(dg_read_out) == 36 && sizeof(dg_report_out) == 40, "record sizes");
    const auto pad = [](size_t b) { return (b + 7) & ~(size_t)7; };
    CHECK(in.size() == 128 + pad((size_t)n_tx * 32) + pad(n_exons * 8) + pad((size_t)n_reads * 36) + pad(n_reports * 40) + pad(n_ops * 4) + n_start * 8);
    CHECK(n_start == 0 || n_start == n_tx);
    CHECK(hash_bits >= 1 && hash_bits <= 64 && strand_mode <= 2u);
    size_t at = 128;
    const std::vector<dg_rna_tx> txs = take<dg_rna_tx>(in, at, n_tx);
    const std::vector<dg_rna_exon> exons = take<dg_rna_exon>(in, at, n_exons);
    const std::vector<dg_read_out> reads = take<dg_read_out>(in, at, (size_t)n_reads);
    const std::vector<dg_report_out> reports = take<dg_report_out>(in, at, n_reports);
    const std::vector<uint32_t> cigar = take<uint32_t>(in, at, n_ops);
    const std::vector<uint64_t> start = take<uint64_t>(in, at, n_start);
    FILE *txt = fopen(argv[2], "w");
    CHECK(txt);
    // dg_tx_set_annotation
    const dg_rna_annot annot{n_tx, 0u, n_exons, txs.data(), exons.data()};
    TxFlat fl;
    char why[400];
    if (!tx_flatten(n_chr, &annot, fl, why, sizeof why)) { fprintf(txt, "err %s\n", why); fclose(txt); return 0; }
    CHECK(fl.chr_first.size() == (size_t)n_chr + 1 && fl.seg_off.size() == fl.seg_start.size() + 1 && fl.tx.size() == n_tx && fl.seg_off.back() == fl.seg_ids.size());
    const std::vector<uint32_t> t_first = exact(fl.chr_first), t_start = exact(fl.seg_start), t_ids = exact(fl.seg_ids);
    const std::vector<uint64_t> t_off = exact(fl.seg_off);
    const std::vector<TxTx> t_tx = exact(fl.tx);
    const std::vector<TxExon> t_ex = exact(fl.ex);
    std::vector<uint32_t> len(n_tx);
    for (uint32_t t = 0; t < n_tx; t++) { len[t] = t_tx[t].len; fprintf(txt, "tx %u %u %u\n", t, t_tx[t].len, t_tx[t].n_ex); }
    for (int c = 0; c < n_chr; c++)
        for (uint32_t i = t_first[(size_t)c]; i < t_first[(size_t)c + 1]; i++) {
            fprintf(txt, "seg %d %u", c, t_start[i]);
            for (uint64_t k = t_off[i]; k < t_off[i + 1]; k++) fprintf(txt, " %u", t_ids[k]);
            fprintf(txt, "\n");
        }
    // dg_tx_count_records
    CHECK(n_pair_mode >= 0 && !(n_pair_mode & 1) && n_pair_mode <= n_reads);
    const long long bad = gc_first_bad_read(reads.data(), n_reads, reports.data(), n_reports, n_ops);
    if (bad >= 0) { fprintf(txt, "bad %lld\n", bad); fclose(txt); return 0; }
    const TxTable T{t_first.data(), t_start.data(), t_off.data(), t_ids.data(), t_tx.data(), t_ex.data(), n_chr, n_tx};
    const GcBatch b{reads.data(), reports.data(), cigar.data(), (unsigned long long)n_reports, (unsigned long long)n_ops, n_reads, n_pair_mode, min_mapq};
    const unsigned long long n_units = gc_units(n_reads, n_pair_mode);
    // k_tx_count: sizes, hashes, the words
    unsigned long long words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> size((size_t)n_units);
    std::vector<uint64_t> hash((size_t)n_units);
    unsigned long long n_ids = 0, n_items = 0;
    for (unsigned long long u = 0; u < n_units; u++) {
        const TxUnit r = tx_unit(b, T, u, strand_mode, nullptr, 0u);
        CHECK(r.outcome <= (uint32_t)TX_COUNTED && (r.outcome == (uint32_t)TX_COUNTED) == (r.size > 0));
        size[(size_t)u] = r.size; hash[(size_t)u] = r.hash;
        words[TXW_UNITS]++; words[1 + r.outcome]++;
        if (r.has_fl) { words[TXW_FL_SUM] += r.fl; words[TXW_FL_N]++; }
        n_ids += r.size; n_items += r.size ? 1 : 0;
    }
    // k_tx_write: a pool of exactly that size
    std::vector<uint32_t> pool((size_t)n_ids);
    std::vector<uint64_t> pool_off((size_t)n_items + 1);
    {
        unsigned long long at_id = 0, item = 0;
        for (unsigned long long u = 0; u < n_units; u++) {
            if (size[(size_t)u]) {
                pool_off[(size_t)item++] = at_id;
                const TxUnit r = tx_unit(b, T, u, strand_mode, pool.data() + at_id, size[(size_t)u]);
                CHECK(r.size == size[(size_t)u] && r.hash == hash[(size_t)u]);
                uint64_t h = 0;
                for (uint32_t k = 0; k < r.size; k++) h = tx_hash_step(h, pool[(size_t)at_id + k]);
                CHECK(tx_hash_end(h, r.size) == r.hash);
                at_id += r.size;
            }
            const TxUnit r = tx_unit(b, T, u, strand_mode, nullptr, 0u);
            fprintf(txt, "unit %llu %u %u %llu", u, r.outcome, r.has_fl, r.fl);
            for (uint32_t k = 0; k < r.size; k++) fprintf(txt, " %u", pool[(size_t)(at_id - r.size) + k]);
            fprintf(txt, "\n");
        }
        pool_off[(size_t)n_items] = at_id;
        CHECK(at_id == n_ids && item == n_items);
    }
    // the class building: the pool into an empty table, then the table folded into itself (every count doubles, the classes stay)
    TxHostTab tab, twice;
    bool collided = false, collided2 = false;
    { const int rc = build(TxTwo{TxItems{nullptr, nullptr, nullptr, 0ull}, TxItems{pool_off.data(), pool.data(), nullptr, n_items}}, hash_bits, tab, collided); if (rc) return rc; }
    {
        const std::vector<uint64_t> off = exact(tab.off), cnt = exact(tab.cnt); const std::vector<uint32_t> ids = exact(tab.ids);
        const TxItems me{off.data(), ids.data(), cnt.data(), (uint64_t)cnt.size()};
        const int rc = build(TxTwo{me, me}, hash_bits, twice, collided2); if (rc) return rc;
        CHECK(twice.cnt.size() == tab.cnt.size() && twice.ids.size() == tab.ids.size());
        std::map<std::vector<uint32_t>, uint64_t> m;
        for (size_t i = 0; i < tab.cnt.size(); i++) m[std::vector<uint32_t>(tab.ids.begin() + tab.off[i], tab.ids.begin() + tab.off[i + 1])] = tab.cnt[i];
        for (size_t i = 0; i < twice.cnt.size(); i++) CHECK(m[std::vector<uint32_t>(twice.ids.begin() + twice.off[i], twice.ids.begin() + twice.off[i + 1])] * 2 == twice.cnt[i]);
        size_t where;
        CHECK(tx_bad_table(off.data(), ids.data(), cnt.data(), cnt.size(), n_tx, where) == nullptr);
    }
    fprintf(txt, "collision %d\n", collided ? 1 : 0);
    const std::vector<uint64_t> c_off = exact(tab.off); const std::vector<uint32_t> c_ids = exact(tab.ids);
    std::vector<uint64_t> c_cnt = exact(tab.cnt);
    const size_t nc = c_cnt.size(), nm = c_ids.size();
    for (size_t i = 0; i < nc; i++) {
        fprintf(txt, "class %llu", (unsigned long long)c_cnt[i]);
        for (uint64_t k = c_off[i]; k < c_off[i + 1]; k++) fprintf(txt, " %u", c_ids[k]);
        fprintf(txt, "\n");
    }
    fprintf(txt, "words");
    for (int i = 0; i < 8; i++) fprintf(txt, " %llu", words[i]);
    fprintf(txt, "\n");
    // dg_tx_finish
    { const uint32_t two[2] = {0u, 1u}; const double zero[2] = {0.0, 0.0}; CHECK(tx_class_D(two, 2, zero) == 0.0 && tx_theta(0ull, 7ull) == 0.0); }      // a class whose members hold nothing gives nothing
    for (uint64_t &v : c_cnt) v *= scale;
    std::vector<uint32_t> active(n_tx, 0u);
    for (uint32_t id : c_ids) active[id] = 1u;
    unsigned long long M = 0, N = 0;
    for (uint32_t t = 0; t < n_tx; t++) M += active[t];
    for (uint64_t v : c_cnt) N += v;
    if (N >= TX_MAX_N) { fprintf(txt, "range\n"); fclose(txt); return 0; }
    const unsigned long long mean = words[TXW_FL_N] ? words[TXW_FL_SUM] / words[TXW_FL_N] : frag_mean;
    std::vector<unsigned long long> S(n_tx), S2(n_tx, 0ull), eff(n_tx);
    std::vector<double> theta(n_tx);
    for (uint32_t t = 0; t < n_tx; t++) { eff[t] = tx_eff(len[t], mean); S[t] = n_start ? start[t] : active[t] ? N * TX_F / M : 0ull; theta[t] = tx_theta(S[t], eff[t]); }
    unsigned long long rounds = 0, converged = M ? 0ull : 1ull;
    while (M && rounds < max_rounds) {
        for (size_t c = 0; c < nc; c++) {
            const uint32_t *p = c_ids.data() + c_off[c];
            const uint64_t n = c_off[c + 1] - c_off[c];
            const double D = tx_class_D(p, n, theta.data());
            if (D == 0.0) continue;
            for (uint64_t k = 0; k < n; k++) S2[p[k]] += tx_share(theta[p[k]], D, c_cnt[c]);
        }
        bool moved = false;
        for (uint32_t t = 0; t < n_tx; t++) { moved = moved || tx_moved(S2[t], S[t]); S[t] = S2[t]; S2[t] = 0ull; theta[t] = tx_theta(S[t], eff[t]); }
        rounds++;
        converged = moved ? 0ull : 1ull;
        if (converged && rounds % TX_CHECK_EVERY == 0) break;
    }
    std::vector<uint64_t> res(n_tx + 16);
    for (uint32_t t = 0; t < n_tx; t++) res[t] = S[t];
    const unsigned long long tail[16] = {words[0], words[1], words[2], words[3], words[4], nc, nm, M, rounds, converged, words[TXW_FL_SUM], words[TXW_FL_N], mean, strand_mode, 0ull, 0ull};
    for (int i = 0; i < 16; i++) res[n_tx + i] = tail[i];
    fprintf(txt, "res");
    for (uint64_t v : res) fprintf(txt, " %llu", (unsigned long long)v);
    fprintf(txt, "\n");
    fclose(txt);
    // dg_tx_format
    std::vector<std::string> names(n_tx);
    std::vector<const char *> name_p(n_tx);
    for (uint32_t t = 0; t < n_tx; t++) { names[t] = "T" + std::to_string(t); name_p[t] = names[t].c_str(); }
    const std::string text = tx_format(res.data(), n_tx, len.data(), name_p.data());
    FILE *tf = fopen(argv[3], "w");
    CHECK(tf);
    fwrite(text.data(), 1, text.size(), tf);
    fclose(tf);
    return 0;
}
