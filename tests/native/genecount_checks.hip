// tests/native/genecount_checks.hip -- the host-callable code of the device's gene counts (dart_amd/csrc/dg_genecount.h) run on the CPU as the library and the
// kernel apply it: the flattening of the annotation, the check of host records, every unit's rows (k_gc_count's lane code) and the table they add up to.
// usage: genecount_checks <input> <output.txt>
//   input       i64 n_chr, n_genes, n_exons, n_reads, n_pair_mode, min_mapq, n_reports, n_ops, 0; the exons (20 bytes each), dg_read_out, dg_report_out, CIGAR
//               words, each array padded to 8 bytes
//   output.txt  "err <text>" when the annotation is refused (nothing else follows); per segment "seg <chr> <start> <any> <plus> <minus>"; "bad <read>" for
//               the first read whose ranges leave the arrays (then nothing else follows); per unit "unit <u> <r0> <r1> <r2>"; per row "row <i> <c0> <c1> <c2>"
#include "../../dart_amd/csrc/dg_genecount.h"
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "genecount_checks: %s failed (line %d)\n", #x, __LINE__); return 2; } } while (0)

template <typename T> static std::vector<T> take(const std::vector<unsigned char> &in, size_t &at, size_t n)
{
    std::vector<T> v(n);                                  // (exact-size copies on the heap: a read that leaves an array leaves its allocation, which the sanitizer build sees)
    if (n) memcpy(v.data(), in.data() + at, n * sizeof(T));
    at += (n * sizeof(T) + 7) & ~(size_t)7;
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: genecount_checks <input> <output.txt>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<unsigned char> in;
    { unsigned char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k); fclose(f); }
    CHECK(in.size() >= 72);
    long long head[9]; memcpy(head, in.data(), 72);
    const int n_chr = (int)head[0], n_reads = (int)head[3], n_pair_mode = (int)head[4];
    const uint32_t n_genes = (uint32_t)head[1], min_mapq = (uint32_t)head[5];
    const size_t n_exons = (size_t)head[2], n_reports = (size_t)head[6], n_ops = (size_t)head[7];
    static_assert(sizeof(dg_gene_exon) == 20 && sizeof(dg_read_out) == 36 && sizeof(dg_report_out) == 40, "record sizes");
    const auto pad = [](size_t b) { return (b + 7) & ~(size_t)7; };
    CHECK(in.size() == 72 + pad(n_exons * 20) + pad((size_t)n_reads * 36) + pad(n_reports * 40) + pad(n_ops * 4));
    size_t at = 72;
    const std::vector<dg_gene_exon> exons = take<dg_gene_exon>(in, at, n_exons);
    const std::vector<dg_read_out> reads = take<dg_read_out>(in, at, (size_t)n_reads);
    const std::vector<dg_report_out> reports = take<dg_report_out>(in, at, n_reports);
    const std::vector<uint32_t> cigar = take<uint32_t>(in, at, n_ops);
    FILE *txt = fopen(argv[2], "w");
    CHECK(txt);
    // dg_gene_set_annotation
    std::vector<uint32_t> first, start, lab;
    char why[400];
    if (!gc_flatten(n_chr, n_genes, n_exons, exons.data(), first, start, lab, why, sizeof why)) { fprintf(txt, "err %s\n", why); fclose(txt); return 0; }
    CHECK(first.size() == (size_t)n_chr + 1 && lab.size() == 3 * start.size() && first[(size_t)n_chr] == start.size());
    // (exact sizes again: gc_flatten's vectors may hold spare capacity)
    const std::vector<uint32_t> t_first(first.begin(), first.end()), t_start(start.begin(), start.end()), t_lab(lab.begin(), lab.end());
    for (int c = 0; c < n_chr; c++)
        for (uint32_t i = t_first[(size_t)c]; i < t_first[(size_t)c + 1]; i++) fprintf(txt, "seg %d %u %u %u %u\n", c, t_start[i], t_lab[3 * (size_t)i], t_lab[3 * (size_t)i + 1], t_lab[3 * (size_t)i + 2]);
    // dg_gene_count_records
    CHECK(n_pair_mode >= 0 && !(n_pair_mode & 1) && n_pair_mode <= n_reads);
    const long long bad = gc_first_bad_read(reads.data(), n_reads, reports.data(), n_reports, n_ops);
    if (bad >= 0) { fprintf(txt, "bad %lld\n", bad); fclose(txt); return 0; }
    const GcTable t{t_first.data(), t_start.data(), t_lab.data(), n_chr};
    const GcBatch b{reads.data(), reports.data(), cigar.data(), (unsigned long long)n_reports, (unsigned long long)n_ops, n_reads, n_pair_mode, min_mapq};
    const size_t n_rows = 4 + (size_t)n_genes;
    std::vector<unsigned long long> counts(n_rows * 3, 0ull);
    const unsigned long long n_units = gc_units(n_reads, n_pair_mode);
    for (unsigned long long u = 0; u < n_units; u++) {
        uint32_t r0 = 0, r1 = 0, r2 = 0;
        gc_unit_rows(b, t, u, r0, r1, r2);
        CHECK(r0 < n_rows && r1 < n_rows && r2 < n_rows);
        counts[3 * (size_t)r0]++; counts[3 * (size_t)r1 + 1]++; counts[3 * (size_t)r2 + 2]++;
        fprintf(txt, "unit %llu %u %u %u\n", u, r0, r1, r2);
    }
    for (size_t i = 0; i < n_rows; i++) fprintf(txt, "row %zu %llu %llu %llu\n", i, counts[3 * i], counts[3 * i + 1], counts[3 * i + 2]);
    fclose(txt);
    return 0;
}
