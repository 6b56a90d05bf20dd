// gtf.h -- the annotation of DART_GENE_COUNTS: a GTF file read on the host into the genes and exons dg_gene_set_annotation takes.
//   * lines that do not start with '#' hold nine tab-separated fields: seqname, source, feature, start, end, score, strand, frame, attributes
//   * a line counts when its feature equals `feature` (DART_GENE_FEATURE, default "exon")
//   * its gene is the value of gene_id "..."; among its attributes; genes are numbered by first appearance
//   * the 1-based closed start, end become the 0-based half-open start - 1, end
//   * a counting line on a sequence the index lacks, or with a strand other than '+' / '-', is skipped and counted (skipped_seq, skipped_strand)
//   * fatal, with the line's number: fewer than nine fields, start or end that is no number, start < 1, end < start, end above 2^32 - 1, no gene_id on a
//     counting line; and a file that leaves no gene at all
// A second reader, gtf_parse_transcripts, makes the transcripts and exons dg_rna_set_annotation takes (DART_RNA_METRICS):
//   * `exon` lines are grouped by transcript_id "..."; transcripts are numbered by first appearance (one id on two sequences or strands gives two transcripts)
//   * `CDS`, `start_codon` and `stop_codon` lines give the transcript's cds_start / cds_end: their smallest start and largest end; none: no CDS
//   * the ribosomal flag is set when gene_biotype, gene_type or transcript_biotype on one of the transcript's lines equals rRNA, Mt_rRNA or rRNA_pseudogene
//   * the skipping and fatal rules above hold for all four features, with transcript_id in gene_id's place: an `exon` line without one is fatal, a CDS or
//     codon line without one counts for nothing; a transcript without an `exon` line is dropped; a file that leaves no transcript at all is fatal
#ifndef DART_GTF_H
#define DART_GTF_H
#include "../../../include/dartgpu.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <unordered_map>

struct GtfAnnotation {
    std::vector<std::string> genes;              // names, in the order of their first appearance
    std::vector<dg_gene_exon> exons;
    size_t lines = 0, skipped_seq = 0, skipped_strand = 0;
};

// the value of gene_id in a GTF attribute field: false when there is none
static inline bool gtf_gene_id(const char *a, const char *end, std::string &out)
{
    while (a < end) {
        while (a < end && (*a == ' ' || *a == '\t')) a++;
        const char *stop = a;                      // the attribute ends at the next ';' outside quotes
        bool quoted = false;
        while (stop < end && (quoted || *stop != ';')) { if (*stop == '"') quoted = !quoted; stop++; }
        if (stop - a > 7 && memcmp(a, "gene_id", 7) == 0 && (a[7] == ' ' || a[7] == '\t')) {
            const char *v = a + 7;
            while (v < stop && (*v == ' ' || *v == '\t')) v++;
            const char *w = stop;
            while (w > v && (w[-1] == ' ' || w[-1] == '\t')) w--;
            if (w - v >= 2 && *v == '"' && w[-1] == '"') { v++; w--; }
            if (w > v) { out.assign(v, w); return true; }
            return false;
        }
        a = stop < end ? stop + 1 : end;
    }
    return false;
}

static inline bool gtf_number(const char *s, const char *e, long long &v)
{
    if (s == e || e - s > 18) return false;
    v = 0;
    for (const char *p = s; p < e; p++) { if (*p < '0' || *p > '9') { if (p == s && *p == '-' && e - s > 1) continue; return false; } v = v * 10 + (*p - '0'); }
    if (*s == '-') v = -v;
    return true;
}

// "" on success, else the failure's text
static inline std::string gtf_parse(const char *path, const std::vector<std::string> &chr_names, const char *feature, GtfAnnotation &out)
{
    FILE *f = fopen(path, "rb");
    if (!f) return std::string("cannot read ") + path;
    std::unordered_map<std::string, int> chr_of, gene_of;
    for (size_t i = 0; i < chr_names.size(); i++) chr_of.emplace(chr_names[i], (int)i);
    const size_t flen = strlen(feature);
    std::string line, gene;
    char *buf = nullptr; size_t cap = 0; ssize_t got;
    std::string err;
    while (err.empty() && (got = getline(&buf, &cap, f)) >= 0) {
        out.lines++;
        size_t n = (size_t)got;
        while (n && (buf[n - 1] == '\n' || buf[n - 1] == '\r')) n--;
        if (!n || buf[0] == '#') continue;
        const char *fld[10]; int nf = 0;
        fld[nf++] = buf;
        for (size_t i = 0; i < n && nf < 9; i++) if (buf[i] == '\t') fld[nf++] = buf + i + 1;
        const std::string at = "line " + std::to_string(out.lines) + ": ";
        if (nf < 9) { err = at + "fewer than nine tab-separated fields"; break; }
        fld[9] = buf + n + 1;                                      // (field k ends one in front of field k + 1)
        auto len = [&](int k) { return (size_t)(fld[k + 1] - 1 - fld[k]); };
        if (len(2) != flen || memcmp(fld[2], feature, flen) != 0) continue;
        const auto c = chr_of.find(std::string(fld[0], len(0)));
        if (c == chr_of.end()) { out.skipped_seq++; continue; }
        if (len(6) != 1 || (fld[6][0] != '+' && fld[6][0] != '-')) { out.skipped_strand++; continue; }
        long long s = 0, e = 0;
        if (!gtf_number(fld[3], fld[3] + len(3), s) || !gtf_number(fld[4], fld[4] + len(4), e)) { err = at + "start or end is not a number"; break; }
        if (s < 1) { err = at + "start " + std::to_string(s) + " is below 1"; break; }
        if (e < s) { err = at + "end " + std::to_string(e) + " is below start " + std::to_string(s); break; }
        if (e > 0xFFFFFFFFll) { err = at + "end " + std::to_string(e) + " is above 2^32 - 1"; break; }
        if (!gtf_gene_id(fld[8], buf + n, gene)) { err = at + "no gene_id among the attributes"; break; }
        auto g = gene_of.find(gene);
        if (g == gene_of.end()) { g = gene_of.emplace(gene, (int)out.genes.size()).first; out.genes.push_back(gene); }
        dg_gene_exon x; x.chr = c->second; x.start = (uint32_t)(s - 1); x.end = (uint32_t)e; x.strand = fld[6][0] == '-' ? 1u : 0u; x.gene = (uint32_t)g->second;
        out.exons.push_back(x);
    }
    free(buf);
    fclose(f);
    if (err.empty() && out.genes.empty()) err = "no gene: none of the " + std::to_string(out.lines) + " lines is a '" + feature + "' line on a sequence of the index";
    return err;
}

struct GtfTranscripts {
    std::vector<std::string> names;              // transcript_id, in the order of first appearance
    std::vector<dg_rna_tx> tx;
    std::vector<dg_rna_exon> exons;
    size_t lines = 0, skipped_seq = 0, skipped_strand = 0, ribosomal = 0, with_cds = 0;
};

// the value of attribute `key` in a GTF attribute field: false when there is none
static inline bool gtf_attr(const char *a, const char *end, const char *key, std::string &out)
{
    const size_t kl = strlen(key);
    while (a < end) {
        while (a < end && (*a == ' ' || *a == '\t')) a++;
        const char *stop = a;                      // the attribute ends at the next ';' outside quotes
        bool quoted = false;
        while (stop < end && (quoted || *stop != ';')) { if (*stop == '"') quoted = !quoted; stop++; }
        if ((size_t)(stop - a) > kl && memcmp(a, key, kl) == 0 && (a[kl] == ' ' || a[kl] == '\t')) {
            const char *v = a + kl;
            while (v < stop && (*v == ' ' || *v == '\t')) v++;
            const char *w = stop;
            while (w > v && (w[-1] == ' ' || w[-1] == '\t')) w--;
            if (w - v >= 2 && *v == '"' && w[-1] == '"') { v++; w--; }
            if (w > v) { out.assign(v, w); return true; }
            return false;
        }
        a = stop < end ? stop + 1 : end;
    }
    return false;
}

// "" on success, else the failure's text
static inline std::string gtf_parse_transcripts(const char *path, const std::vector<std::string> &chr_names, GtfTranscripts &out)
{
    FILE *f = fopen(path, "rb");
    if (!f) return std::string("cannot read ") + path;
    struct Tx { int chr; uint32_t strand; bool ribosomal = false, cds = false; uint32_t cds_start = 0, cds_end = 0; std::vector<dg_rna_exon> exons; };
    std::unordered_map<std::string, int> chr_of, tx_of;
    std::vector<Tx> txs; std::vector<std::string> ids;
    for (size_t i = 0; i < chr_names.size(); i++) chr_of.emplace(chr_names[i], (int)i);
    std::string id, val;
    char *buf = nullptr; size_t cap = 0; ssize_t got;
    std::string err;
    while (err.empty() && (got = getline(&buf, &cap, f)) >= 0) {
        out.lines++;
        size_t n = (size_t)got;
        while (n && (buf[n - 1] == '\n' || buf[n - 1] == '\r')) n--;
        if (!n || buf[0] == '#') continue;
        const char *fld[10]; int nf = 0;
        fld[nf++] = buf;
        for (size_t i = 0; i < n && nf < 9; i++) if (buf[i] == '\t') fld[nf++] = buf + i + 1;
        const std::string at = "line " + std::to_string(out.lines) + ": ";
        if (nf < 9) { err = at + "fewer than nine tab-separated fields"; break; }
        fld[9] = buf + n + 1;                                      // (field k ends one in front of field k + 1)
        auto len = [&](int k) { return (size_t)(fld[k + 1] - 1 - fld[k]); };
        auto is = [&](const char *w) { return len(2) == strlen(w) && memcmp(fld[2], w, len(2)) == 0; };
        const bool exon = is("exon");
        if (!exon && !is("CDS") && !is("start_codon") && !is("stop_codon")) continue;
        const auto c = chr_of.find(std::string(fld[0], len(0)));
        if (c == chr_of.end()) { out.skipped_seq++; continue; }
        if (len(6) != 1 || (fld[6][0] != '+' && fld[6][0] != '-')) { out.skipped_strand++; continue; }
        long long s = 0, e = 0;
        if (!gtf_number(fld[3], fld[3] + len(3), s) || !gtf_number(fld[4], fld[4] + len(4), e)) { err = at + "start or end is not a number"; break; }
        if (s < 1) { err = at + "start " + std::to_string(s) + " is below 1"; break; }
        if (e < s) { err = at + "end " + std::to_string(e) + " is below start " + std::to_string(s); break; }
        if (e > 0xFFFFFFFFll) { err = at + "end " + std::to_string(e) + " is above 2^32 - 1"; break; }
        if (!gtf_attr(fld[8], buf + n, "transcript_id", id)) { if (exon) { err = at + "no transcript_id among the attributes"; break; } continue; }
        const std::string key = id + '\t' + std::to_string(c->second) + fld[6][0];
        auto t = tx_of.find(key);
        if (t == tx_of.end()) { t = tx_of.emplace(key, (int)txs.size()).first; Tx x; x.chr = c->second; x.strand = fld[6][0] == '-' ? 1u : 0u; txs.push_back(x); ids.push_back(id); }
        Tx &x = txs[(size_t)t->second];
        if (exon) x.exons.push_back(dg_rna_exon{(uint32_t)(s - 1), (uint32_t)e});
        else {
            if (!x.cds || (uint32_t)(s - 1) < x.cds_start) x.cds_start = (uint32_t)(s - 1);
            if (!x.cds || (uint32_t)e > x.cds_end) x.cds_end = (uint32_t)e;
            x.cds = true;
        }
        for (const char *k : {"gene_biotype", "gene_type", "transcript_biotype"})
            if (gtf_attr(fld[8], buf + n, k, val) && (val == "rRNA" || val == "Mt_rRNA" || val == "rRNA_pseudogene")) x.ribosomal = true;
    }
    free(buf);
    fclose(f);
    if (!err.empty()) return err;
    for (size_t i = 0; i < txs.size(); i++) {
        const Tx &x = txs[i];
        if (x.exons.empty()) continue;
        dg_rna_tx t; t.chr = x.chr; t.strand = x.strand; t.flags = x.ribosomal ? DG_RNA_TX_RIBOSOMAL : 0u; t.cds_start = x.cds ? x.cds_start : 0u; t.cds_end = x.cds ? x.cds_end : 0u;
        t.n_exons = (uint32_t)x.exons.size(); t.first_exon = (uint64_t)out.exons.size();
        out.exons.insert(out.exons.end(), x.exons.begin(), x.exons.end());
        out.tx.push_back(t); out.names.push_back(ids[i]);
        out.ribosomal += x.ribosomal ? 1 : 0; out.with_cds += x.cds ? 1 : 0;
    }
    if (out.tx.empty()) return "no transcript: none of the " + std::to_string(out.lines) + " lines is an 'exon' line on a sequence of the index";
    return "";
}
#endif
