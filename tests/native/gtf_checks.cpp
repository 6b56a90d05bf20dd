// tests/native/gtf_checks.cpp -- the GTF reader of `dart` (dart_amd/csrc/host/gtf.h) on a file: what DART_GENE_COUNTS would hand to dg_gene_set_annotation.
// usage: gtf_checks <file.gtf> <feature> <chromosome name>...
//   stdout  per gene "gene <index> <name>", per exon "exon <chr> <start> <end> <strand> <gene>", "skipped <sequences> <strands>"; a refusal: "error <text>", exit 1
#include "../../dart_amd/csrc/host/gtf.h"

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: gtf_checks <file.gtf> <feature> <chromosome name>...\n"); return 2; }
    std::vector<std::string> names(argv + 3, argv + argc);
    GtfAnnotation a;
    const std::string err = gtf_parse(argv[1], names, argv[2], a);
    if (!err.empty()) { printf("error %s\n", err.c_str()); return 1; }
    for (size_t g = 0; g < a.genes.size(); g++) printf("gene %zu %s\n", g, a.genes[g].c_str());
    for (const dg_gene_exon &x : a.exons) printf("exon %d %u %u %u %u\n", x.chr, x.start, x.end, x.strand, x.gene);
    printf("skipped %zu %zu\n", a.skipped_seq, a.skipped_strand);
    return 0;
}
