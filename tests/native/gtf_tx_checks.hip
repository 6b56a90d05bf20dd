// tests/native/gtf_tx_checks.hip -- the path from a GTF file to the expression stage's tables as `dart` walks it under DART_TX_QUANT: gtf_parse_transcripts
// (dart_amd/csrc/host/gtf.h), the dg_rna_annot it is handed on as, tx_flatten (dart_amd/csrc/dg_txquant.h).  Stand-alone, host code only.
// usage: gtf_tx_checks <annotation.gtf> <chromosome names ...>
//   stdout  "error <text>" (exit 1) when the reader or the flattening refuses; else "skipped <seq> <strand>", per transcript "tx <t> <chr> <strand> <L> <merged
//           exons> <name>", per merged exon "mex <t> <start> <end> <before>", per segment "seg <chr> <start> <ids ...>"
#include "../../dart_amd/csrc/host/gtf.h"
#include "../../dart_amd/csrc/dg_txquant.h"

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: gtf_tx_checks <annotation.gtf> <chromosome names ...>\n"); return 2; }
    const std::vector<std::string> names(argv + 2, argv + argc);
    GtfTranscripts g;
    const std::string err = gtf_parse_transcripts(argv[1], names, g);
    if (!err.empty()) { printf("error %s\n", err.c_str()); return 1; }
    dg_rna_annot ann; ann.n_tx = (uint32_t)g.tx.size(); ann.pad = 0; ann.n_exons = g.exons.size(); ann.tx = g.tx.data(); ann.exons = g.exons.data();
    TxFlat fl;
    char why[400];
    if (!tx_flatten((int)names.size(), &ann, fl, why, sizeof why)) { printf("error %s\n", why); return 1; }
    printf("skipped %zu %zu\n", g.skipped_seq, g.skipped_strand);
    for (size_t t = 0; t < fl.tx.size(); t++) {
        printf("tx %zu %d %u %u %u %s\n", t, fl.tx[t].chr, fl.tx[t].strand, fl.tx[t].len, fl.tx[t].n_ex, g.names[t].c_str());
        for (uint32_t k = 0; k < fl.tx[t].n_ex; k++) { const TxExon &e = fl.ex[fl.tx[t].first_ex + k]; printf("mex %zu %u %u %u\n", t, e.start, e.end, e.before); }
    }
    for (size_t c = 0; c < names.size(); c++)
        for (uint32_t i = fl.chr_first[c]; i < fl.chr_first[c + 1]; i++) {
            printf("seg %zu %u", c, fl.seg_start[i]);
            for (uint64_t k = fl.seg_off[i]; k < fl.seg_off[i + 1]; k++) printf(" %u", fl.seg_ids[k]);
            printf("\n");
        }
    return 0;
}
