// tests/native/gtf_rna_checks.cpp -- the transcript reader of `dart` (dart_amd/csrc/host/gtf.h, gtf_parse_transcripts) on a file: what DART_RNA_METRICS would
// hand to dg_rna_set_annotation.
// usage: gtf_rna_checks <file.gtf> <chromosome name>...
//   stdout  per transcript "tx <index> <chr> <strand> <flags> <cds_start> <cds_end> <n_exons> <first_exon> <name>", per exon "exon <start> <end>",
//           "skipped <sequences> <strands>"; a refusal: "error <text>", exit 1
#include "../../dart_amd/csrc/host/gtf.h"

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: gtf_rna_checks <file.gtf> <chromosome name>...\n"); return 2; }
    std::vector<std::string> names(argv + 2, argv + argc);
    GtfTranscripts a;
    const std::string err = gtf_parse_transcripts(argv[1], names, a);
    if (!err.empty()) { printf("error %s\n", err.c_str()); return 1; }
    for (size_t t = 0; t < a.tx.size(); t++)
        printf("tx %zu %d %u %u %u %u %u %llu %s\n", t, a.tx[t].chr, a.tx[t].strand, a.tx[t].flags, a.tx[t].cds_start, a.tx[t].cds_end, a.tx[t].n_exons, (unsigned long long)a.tx[t].first_exon, a.names[t].c_str());
    for (const dg_rna_exon &x : a.exons) printf("exon %u %u\n", x.start, x.end);
    printf("skipped %zu %zu\n", a.skipped_seq, a.skipped_strand);
    return 0;
}
