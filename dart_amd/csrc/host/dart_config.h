// dart_amd/csrc/host/dart_config.h -- what `dart` was asked to do, decided once: the command line (main.cpp:96-239 of the reference), every DART_*
// variable of the environment, and what follows from them.  Config::parse fills it before the first HIP call and nothing reads the environment after it;
// choose_pipelines states, in one place, which of the four host pipelines a library's files may take.  No GPU and no libdartgpu here (dartgpu.h for its
// types only): tests/native/dart_config_checks.cpp includes this header without `main` and checks both against tables.
#pragma once
#include "dartgpu.h"
#include <zlib.h>
#include <sys/stat.h>
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

static const char *VersionStr = "1.4.6";

static const int RUN = -1;      // what Config::parse and the stages of main return to go on; anything else is the exit code

struct Config {
    // ---- the command line (main.cpp:136-205) ----
    const char *index = nullptr, *out = "output.sam";
    char sj[256] = "junctions.tab";
    std::vector<std::string> f1, f2;
    int threads = 4;
    bool pair_end = false, multi = false, unique = false, silent = false, all_sj = false, bam = false;
    dg_params p;                            // the caller's defaults with -mis, -max_dup, -max_intron, -min_intron, -m, -all_sj and `paired` applied
    bool two_files() const { return f1.size() == f2.size(); }      // separate mate files: library k is f1[k] + f2[k]

    // ---- the environment ----
    size_t batch_reads = 500000;            // DART_BATCH: at least 4000, even
    int inflight = 2;                       // DART_INFLIGHT: contexts per device, at least 1
    bool has_gpus = false; int gpus = 0;    // DART_GPUS (raw: the clamp needs the device count)
    int same_device_times = 0;              // DART_SAME_DEVICE_TIMES: 0 = unset, else 1..8
    bool streaming = false;                 // DART_STREAMING is set (to anything): every library takes the streaming pipeline
    bool gz_stream = false;                 // DART_GZ_STREAM is set (to anything): no .gz file is inflated whole
    size_t gz_whole_max = 0;                // DART_GZ_WHOLE_MAX_GB (default 8) in bytes, per library
    bool timing = false;                    // DART_TIMING is set (to anything)
    bool sync_aids = false;                 // DART_SYNC_AIDS
    bool has_expected_reads = false; uint64_t expected_reads = 0;      // DART_EXPECTED_READS
    bool device_fastq = false;              // DART_DEVICE_FASTQ, unless -bo streams
    bool device_sj = false;                 // DART_DEVICE_SJ
    bool sort_bam = false, bam_index = false, mark_dups = false;       // DART_SORT_BAM, DART_BAM_INDEX, DART_MARK_DUPLICATES
    int md_umi = 0; char md_umi_sep = '_';  // DART_MARKDUP_UMI: 0 = unset, 1 = exact, 2 = edit1; DART_MARKDUP_UMI_SEP (default: DART_UMI_SEP)
    int coverage = 0;                       // DART_COVERAGE: 0, 1 or 2
    uint32_t cov_exclude = 0x704u, cov_min_mapq = 0u;                  // DART_COVERAGE_EXCLUDE, DART_COVERAGE_MIN_MAPQ
    bool pileup = false;                    // DART_PILEUP
    uint32_t pu_min_alt = 2u, pu_exclude = 0x704u, pu_min_mapq = 0u;   // DART_PILEUP_MIN_ALT, DART_PILEUP_EXCLUDE, DART_PILEUP_MIN_MAPQ
    bool qc = false;                        // DART_QC
    uint32_t qc_exclude = 0x904u, qc_min_mapq = 0u;                    // DART_QC_EXCLUDE, DART_QC_MIN_MAPQ
    const char *rna_gtf = nullptr;          // DART_RNA_METRICS (empty = unset)
    uint32_t rna_exclude = 0x904u, rna_min_mapq = 0u;                  // DART_RNA_EXCLUDE, DART_RNA_MIN_MAPQ
    uint64_t rna_min_cov = 100u;            // DART_RNA_MIN_COV
    uint32_t bam_tags = 0u;                 // DART_BAM_TAGS: DG_TAG_* bits, 0 = not asked for
    double sort_piece_mb = 256.0;           // DART_SORT_PIECE_MB, raw: the piece arithmetic is where the pieces are cut
    const char *gene_gtf = nullptr;         // DART_GENE_COUNTS (empty = unset)
    const char *gene_feature = "exon";      // DART_GENE_FEATURE (empty = unset)
    uint32_t gene_min_mapq = 4u;            // DART_GENE_MIN_MAPQ
    const char *tx_gtf = nullptr;           // DART_TX_QUANT (empty = unset)
    uint32_t tx_strand = 0u, tx_max_rounds = 1000u;                    // DART_TX_STRAND (0, 1, 2), DART_TX_MAX_ROUNDS
    uint64_t tx_frag_mean = 200u;           // DART_TX_FRAG_MEAN
    static constexpr uint32_t tx_min_mapq = 4u;                        // the units that count as unique: the -unique rule, mapq > 3 (no switch)
    std::string tx_path;                    // <out>.transcripts.tab; empty = not asked for
    bool trim = false;                      // any of DART_TRIM_ADAPTER, DART_TRIM_QUAL, DART_TRIM_QUAL5, DART_TRIM_POLY
    dg_trim trim_par;                       // the DART_TRIM_* switches as dg_set_trim takes them (flags: the library's pairing decides DG_TRIM_PAIRS)
    std::string trim_path;                  // <out>.trim.txt; empty = not asked for
    bool umi = false;                       // DART_UMI
    dg_umi umi_par;                         // DART_UMI, DART_UMI_SKIP, DART_UMI_SEP as dg_set_umi takes them (flags: the library's pairing decides DG_UMI_PAIRS)
    bool cuts() const { return trim || umi; }      // the upload takes the trimmed path: what holds for DART_TRIM_* holds for DART_UMI
    int write_threads = 1;                  // DART_WRITE_THREADS, at least 1
    int fmt_threads = 0;                    // DART_FMT_THREADS, at least 1; 0 = unset (what -t leaves)
    bool write_mmap = false;                // DART_WRITE=mmap
    bool pinned = false;                    // DART_PINNED

    // ---- what follows from both ----
    bool device_bam = false;                // -bo and DART_DEVICE_BAM: records and BGZF blocks from the device
    bool bam_streams = false;               // -bo without it: the streaming pipeline, BAM from host text
    bool bgzf_dynamic = false;              // DART_BGZF_DYNAMIC beside device_bam (alone it does nothing)
    bool device_sam = false;                // DART_DEVICE_SAM, which -bo switches off (BAM is built from host text, or on the device)
    bool device_gz = false;                 // DART_DEVICE_GZ with DART_DEVICE_FASTQ, a device formatter, no -bo streaming and no DART_STREAMING
    std::vector<std::pair<std::string, uint32_t>> cov_tracks;      // the coverage tracks: path, strand flags
    std::string bai_path, md_path, genes_path, sites_path;         // <out>.bai, <out>.markdup.txt, <out>.genes.tab, <out>.sites.tsv; empty = not asked for
    std::string qc_path;                                           // <out>.qc.txt; empty = not asked for
    std::string rna_path;                                          // <out>.rna_metrics.txt; empty = not asked for
    const char *bam_dev_note = "";          // the `bam=` field of the DART_TIMING lines: the parallel pipeline's ...
    const char *bam_host_note = "";         // ... and the streaming pipeline's

    void usage(FILE *f, const char *prog) const      // ShowProgramUsage, main.cpp:20-40
    {
        fprintf(f, "\nDART v%s (Hsin-Nan Lin & Wen-Lian Hsu)\n\n", VersionStr);
        fprintf(f, "Usage: %s -i Index_Prefix -f <ReadFile_A1 ReadFile_B1 ...> [-f2 <ReadFile_A2 ReadFile_B2 ...>] -o|-bo Alignment_Output\n\n", prog);
        fprintf(f, "Options: -t INT        number of threads [4]\n");
        fprintf(f, "         -f            files with #1 mates reads\n");
        fprintf(f, "         -f2           files with #2 mates reads\n");
        fprintf(f, "         -mis INT      maximal number of mismatches in an alignment\n");
        fprintf(f, "         -max_dup INT  maximal number of repetitive fragments (between 100-10000) [%d]\n", p.max_dup);
        fprintf(f, "         -o            alignment filename in SAM format\n");
        fprintf(f, "         -bo           alignment filename in BAM format\n");
        fprintf(f, "                       (DART_DEVICE_BAM=1 DART_SORT_BAM=1: coordinate-sorted on the device; DART_BAM_INDEX=1 beside them: its .bai too; DART_COVERAGE=1 or 2: its bedGraph, or one per strand; DART_MARK_DUPLICATES=1: flag 0x400 set on the device)\n");
        fprintf(f, "         -j            splice junction output filename [junctions.tab]\n");
        fprintf(f, "         -m            output multiple alignments [false]\n");
        fprintf(f, "         -all_sj       detect all splice junction regardless of mapq score [false]\n");
        fprintf(f, "         -p            paired-end reads are interlaced in the same file\n");
        fprintf(f, "         -unique       output unique alignments\n");
        fprintf(f, "         -max_intron   the maximal intron size [500000]\n");
        fprintf(f, "         -min_intron   the minimal intron size [10]\n");
        fprintf(f, "         -v            version\n");
        fprintf(f, "\n");
    }

    // DART_BAM_TAGS' value -> DG_TAG_* bits; 0: `bad` holds the first word that is none of MD, NM, ts (the whole value for 1 / all misspelt; "" for an empty word)
    static uint32_t parse_bam_tags(const char *v, std::string &bad)
    {
        const std::string s = v;
        if (s == "1" || s == "all") return DG_TAG_MD | DG_TAG_NM | DG_TAG_TS;
        uint32_t bits = 0;
        for (size_t at = 0;;) {
            const size_t e = s.find(',', at);
            const std::string w = s.substr(at, e == std::string::npos ? std::string::npos : e - at);
            if (w == "MD") bits |= DG_TAG_MD; else if (w == "NM") bits |= DG_TAG_NM; else if (w == "ts") bits |= DG_TAG_TS;
            else { bad = w; return 0; }
            if (e == std::string::npos) break;
            at = e + 1;
        }
        return bits;
    }

    // the DART_TRIM_* switches into trim / trim_par; RUN, or 1 behind a value that cannot be used (said on err_f)
    int parse_trim(const char *(*lookup)(const char *), FILE *err_f)
    {
        memset(&trim_par, 0, sizeof trim_par);
        trim_par.qual_base = 33; trim_par.min_overlap = 3; trim_par.max_err_permille = 100; trim_par.poly_min = 10; trim_par.min_len = 20;
        auto adapter = [&](const char *key, int which) -> bool {      // false: said why
            const char *v = lookup(key);
            if (!v || !v[0]) return true;
            std::string a = v;
            if (a == "illumina") a = "AGATCGGAAGAGC"; else if (a == "nextera") a = "CTGTCTCTTATA"; else if (a == "smallrna") a = "TGGAATTCTCGG";
            if (a.size() > 64 || a.find_first_not_of("ACGT") != std::string::npos) {
                fprintf(err_f, "Error! %s=%s: an adapter is at most 64 letters of ACGT, or one of illumina, nextera, smallrna\n", key, v);
                return false;
            }
            trim_par.n_adapter[which] = (uint32_t)a.size(); memcpy(trim_par.adapter[which], a.data(), a.size());
            return true;
        };
        if (!adapter("DART_TRIM_ADAPTER", 0)) return 1;
        trim_par.n_adapter[1] = trim_par.n_adapter[0]; memcpy(trim_par.adapter[1], trim_par.adapter[0], 64);
        if (!adapter("DART_TRIM_ADAPTER2", 1)) return 1;
        const struct { const char *name; uint32_t *to; unsigned long long lo, hi; } num[7] = {
            {"DART_TRIM_QUAL", &trim_par.qual3, 0ull, 93ull}, {"DART_TRIM_QUAL5", &trim_par.qual5, 0ull, 93ull}, {"DART_TRIM_POLY_MIN", &trim_par.poly_min, 1ull, 1000ull},
            {"DART_TRIM_MIN_OVERLAP", &trim_par.min_overlap, 1ull, 64ull}, {"DART_TRIM_ERR", &trim_par.max_err_permille, 0ull, 1000ull}, {"DART_TRIM_MIN_LEN", &trim_par.min_len, 1ull, 1000ull},
            {nullptr, nullptr, 0ull, 0ull}};
        for (int k = 0; num[k].name; k++) if (const char *v = lookup(num[k].name)) {
            char *end = nullptr;
            errno = 0;
            const unsigned long long x = strtoull(v, &end, 10);
            if (!(v[0] >= '0' && v[0] <= '9') || *end || errno || x < num[k].lo || x > num[k].hi) {
                fprintf(err_f, "Error! %s=%s: a whole number from %llu to %llu is expected\n", num[k].name, v, num[k].lo, num[k].hi);
                return 1;
            }
            *num[k].to = (uint32_t)x;
        }
        if (const char *v = lookup("DART_TRIM_POLY")) for (const char *q = v; *q; q++) {
            const char *at = strchr("ACGT", *q >= 'a' && *q <= 'z' ? *q - 32 : *q);
            if (!at) { fprintf(err_f, "Error! DART_TRIM_POLY=%s: letters of ACGT are expected\n", v); return 1; }
            trim_par.poly_mask |= 1u << (at - "ACGT");
        }
        trim = trim_par.n_adapter[0] || trim_par.n_adapter[1] || trim_par.qual3 || trim_par.qual5 || trim_par.poly_mask;
        return RUN;
    }

    // DART_UMI=<n1>[,<n2>] (the UMI's letters at the start of mate 1 / mate 2), DART_UMI_SKIP=<n1>[,<n2>] (linker bases behind them), DART_UMI_SEP (one byte, default _)
    // into umi / umi_par; RUN, or 1 behind a value that cannot be used (said on err_f)
    int parse_umi(const char *(*lookup)(const char *), FILE *err_f)
    {
        memset(&umi_par, 0, sizeof umi_par);
        umi_par.sep = '_';
        auto two = [&](const char *key, uint32_t to[2]) -> bool {
            const char *v = lookup(key);
            if (!v) return true;
            const char *q = v;
            for (int m = 0; m < 2; m++) {
                char *end = nullptr;
                errno = 0;
                const unsigned long long x = strtoull(q, &end, 10);
                if (!(q[0] >= '0' && q[0] <= '9') || errno || x > 1000ull || (*end && !(*end == ',' && m == 0))) { fprintf(err_f, "Error! %s=%s: one or two whole numbers from 0 to 1000, <n1>[,<n2>], are expected\n", key, v); return false; }
                to[m] = (uint32_t)x;
                if (!*end) break;
                q = end + 1;
            }
            return true;
        };
        if (!two("DART_UMI", umi_par.len) || !two("DART_UMI_SKIP", umi_par.skip)) return 1;
        if (const char *v = lookup("DART_UMI_SEP")) {
            if (strlen(v) != 1 || strchr(" \t/ACGTN+-", v[0])) { fprintf(err_f, "Error! DART_UMI_SEP=%s: one byte that is no blank, tab, / or one of ACGTN+-\n", v); return 1; }
            umi_par.sep = v[0];
        }
        umi = lookup("DART_UMI") != nullptr;
        if (umi && (umi_par.len[0] + umi_par.len[1] == 0 || umi_par.len[0] + umi_par.len[1] > 21u)) { fprintf(err_f, "Error! DART_UMI=%s: the two lengths together are 1 to 21 letters\n", lookup("DART_UMI")); return 1; }
        if (!umi && lookup("DART_UMI_SKIP")) { fprintf(err_f, "Error! DART_UMI_SKIP=%s needs DART_UMI: DART_UMI is missing\n", lookup("DART_UMI_SKIP")); return 1; }
        return RUN;
    }

    // argv and the environment into *this.  lookup: getenv, or a test's table.  defaults: dg_params_default's, handed in so that this header links without the library.
    // The sequence of the checks is the program's: a run that fails two of them reports the first.
    // Returns RUN, or the exit code of a run that ends here: 0 behind -h, -v and an unreadable input (main.cpp returns 0 there), 1 behind an error.  What it
    // has to say goes to `out` (the program's stdout) and `err` (its stderr).
    int parse(int argc, char *argv[], const char *(*lookup)(const char *), const dg_params &defaults, FILE *out_f, FILE *err_f)
    {
        auto env_on = [lookup](const char *k) { const char *v = lookup(k); return v && atoi(v) != 0; };
        p = defaults;
        if (argc == 1 || strcmp(argv[1], "-h") == 0) { usage(out_f, argv[0]); return 0; }
        for (int i = 1; i < argc; i++) {   // main.cpp:136-205
            std::string a = argv[i];
            if (a == "-i") index = argv[++i];
            else if (a == "-f") { while (++i < argc && argv[i][0] != '-') f1.push_back(argv[i]); i--; }
            else if (a == "-f2") { while (++i < argc && argv[i][0] != '-') f2.push_back(argv[i]); i--; }
            else if (a == "-t") { if ((threads = atoi(argv[++i])) <= 0) { fprintf(out_f, "Warning! Thread number should be a positive number!\n"); threads = 4; } }
            else if (a == "-o") { out = argv[++i]; bam = false; }                      // main.cpp:158-168
            else if (a == "-bo") { out = argv[++i]; bam = true; }
            else if (a == "-mis" && i + 1 < argc) p.max_mismatch = atoi(argv[++i]);
            else if (a == "-max_dup" && i + 1 < argc) { p.max_dup = atoi(argv[++i]); if (p.max_dup < 100) p.max_dup = 100; else if (p.max_dup >= 10000) p.max_dup = 10000; }
            else if (a == "-silent") silent = true;
            else if (a == "-j") { strncpy(sj, argv[++i], 255); sj[255] = 0; }
            else if (a == "-p") pair_end = true;
            else if (a == "-m") multi = true;
            else if (a == "-unique") unique = true;
            else if (a == "-all_sj") all_sj = true;
            else if (a == "-max_intron") { if ((p.max_intron = atoi(argv[++i])) < 100000) p.max_intron = 100000; }
            else if (a == "-min_intron") p.min_intron = atoi(argv[++i]);
            else if (a == "-d" || a == "-debug") {}   // debug prints are not reproduced
            else if (a == "-v" || a == "--version") { fprintf(out_f, "DART v%s\n\n", VersionStr); return 0; }
            else { fprintf(err_f, "Error! Unknow parameter: %s\n", argv[i]); usage(out_f, argv[0]); return 1; }
        }
        p.multi_hit = multi; p.all_sj = all_sj;
        if (f1.empty()) { fprintf(err_f, "Error! Please specify a valid read input!\n"); usage(out_f, argv[0]); return 1; }
        if (!f2.empty() && f1.size() != f2.size()) {
            fprintf(err_f, "Error! Paired-end reads input numbers do not match!\n");
            fprintf(err_f, "Read1:\n"); for (auto &s : f1) fprintf(err_f, "\t%s\n", s.c_str());
            fprintf(err_f, "Read2:\n"); for (auto &s : f2) fprintf(err_f, "\t%s\n", s.c_str());
            return 1;
        }
        p.paired = (pair_end || two_files()) ? 1 : 0;
        {   // CheckInputFiles / CheckOutputFileName, main.cpp:42-94,220
            struct stat st; bool ok = true;
            for (auto &s : f1) if (stat(s.c_str(), &st) == -1) { ok = false; fprintf(err_f, "Cannot access file:[%s]\n", s.c_str()); }
            for (auto &s : f2) if (stat(s.c_str(), &st) == -1) { ok = false; fprintf(err_f, "Cannot access file:[%s]\n", s.c_str()); }
            if (strcmp(out, "output.sam") != 0 && stat(out, &st) == 0) {
                if (st.st_mode & S_IFDIR) { ok = false; fprintf(out_f, "Warning: %s is a directory!\n", out); }
                else if (!(st.st_mode & S_IFREG)) { ok = false; fprintf(out_f, "Warning: %s is not a regular file!\n", out); }
            }
            if (!ok) return 0;
        }
        if (const char *v = lookup("DART_BATCH")) batch_reads = (size_t)atoll(v);
        batch_reads = std::max<size_t>(4000, batch_reads & ~(size_t)1);
        if (const char *v = lookup("DART_INFLIGHT")) inflight = atoi(v);
        inflight = std::max(1, inflight);
        // DART_DEVICE_BAM=1 with -bo: plain-FASTQ libraries (and .gz ones inflated whole) take the parallel pipeline, and the BAM records and their BGZF blocks come
        // from the device (dg_batch_format_bam); FASTA and streamed .gz keep the host writer whatever the switch says.  Without the switch -bo is what it always was.
        device_bam = bam && env_on("DART_DEVICE_BAM");
        bgzf_dynamic = device_bam && env_on("DART_BGZF_DYNAMIC");      // (alone it does nothing)
        bam_streams = bam && !device_bam;         // -bo forces the streaming pipeline
        // DART_SORT_BAM=1 beside -bo and DART_DEVICE_BAM=1: the records of every batch stay in HBM (dg_batch_accumulate_bam) and the file is written once, at the end,
        // in coordinate order (dg_bam_sort_finish / dg_bam_sort_compress).  A user who asked for a sorted file never silently gets an unsorted one: whatever is
        // missing ends the run before any output exists.
        sort_bam = env_on("DART_SORT_BAM");
        if (sort_bam && !device_bam) {
            fprintf(err_f, "Error! DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1: %s missing\n", !bam ? (env_on("DART_DEVICE_BAM") ? "-bo is" : "both are") : "DART_DEVICE_BAM=1 is");
            return 1;
        }
        // DART_BAM_INDEX=1 beside DART_SORT_BAM=1: the sorted file's index <out>.bai, built on the device from the sorted records and the blocks' sizes
        // (dg_bam_index_finish) in place of the `samtools index` behind the sort.  Without the sort there is nothing to index: no output is begun.
        bam_index = env_on("DART_BAM_INDEX");
        if (bam_index && !sort_bam) {
            fprintf(err_f, "Error! DART_BAM_INDEX=1 needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing\n");
            return 1;
        }
        if (bam_index) bai_path = std::string(out) + ".bai";
        // DART_COVERAGE=1 beside DART_SORT_BAM=1: the sorted file's coverage track <out>.bedgraph, built on the device from the sorted records (dg_bam_coverage_finish)
        // in place of a `bedtools genomecov -bg -split` over the file; DART_COVERAGE=2: <out>.plus.bedgraph and <out>.minus.bedgraph.  DART_COVERAGE_EXCLUDE (default
        // 0x704) and DART_COVERAGE_MIN_MAPQ (default 0) are the filter.  Without the sort there is nothing to cover: no output is begun.
        if (const char *v = lookup("DART_COVERAGE")) coverage = atoi(v);
        if (coverage != 0 && coverage != 1 && coverage != 2) {
            fprintf(err_f, "Error! DART_COVERAGE=%d is neither 1 (one track) nor 2 (one track per strand)\n", coverage);
            return 1;
        }
        if (coverage && !sort_bam) {
            fprintf(err_f, "Error! DART_COVERAGE=%d needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing\n", coverage);
            return 1;
        }
        if (const char *v = lookup("DART_COVERAGE_EXCLUDE")) cov_exclude = (uint32_t)strtoul(v, nullptr, 0);
        if (const char *v = lookup("DART_COVERAGE_MIN_MAPQ")) cov_min_mapq = (uint32_t)strtoul(v, nullptr, 0);
        if (coverage == 1) cov_tracks.emplace_back(std::string(out) + ".bedgraph", 0u);
        if (coverage == 2) { cov_tracks.emplace_back(std::string(out) + ".plus.bedgraph", DG_COV_STRAND_PLUS); cov_tracks.emplace_back(std::string(out) + ".minus.bedgraph", DG_COV_STRAND_MINUS); }
        // DART_MARK_DUPLICATES=1 beside DART_SORT_BAM=1: flag 0x400 is written into the sorted records on the device (dg_bam_markdup_finish) before the first piece
        // is compressed, in place of a `samtools markdup` over the file; the index and the tracks see the marked records; <out>.markdup.txt holds the counts.
        // Without the sort there is nothing to mark: no output is begun.
        mark_dups = env_on("DART_MARK_DUPLICATES");
        if (mark_dups && !sort_bam) {
            fprintf(err_f, "Error! DART_MARK_DUPLICATES=1 needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing\n");
            return 1;
        }
        if (mark_dups) md_path = std::string(out) + ".markdup.txt";
        // DART_MARKDUP_UMI=exact|edit1 beside DART_MARK_DUPLICATES=1: the UMI behind the last DART_MARKDUP_UMI_SEP (default _; ':' for names that carry the UMI as their
        // last field) of a read's name is part of a duplicate's signature (dg_bam_markdup_umi_finish); edit1 also joins UMIs one letter apart.  <out>.markdup.txt
        // gains four counts.  Alone it would mark nothing: no output is begun.
        if (const char *v = lookup("DART_MARKDUP_UMI")) {
            md_umi = strcmp(v, "exact") == 0 ? 1 : strcmp(v, "edit1") == 0 ? 2 : 0;
            if (!md_umi) { fprintf(err_f, "Error! DART_MARKDUP_UMI=%s: exact or edit1\n", v); return 1; }
            if (!mark_dups) { fprintf(err_f, "Error! DART_MARKDUP_UMI=%s needs DART_MARK_DUPLICATES=1 (and with it DART_SORT_BAM=1): DART_MARK_DUPLICATES=1 is missing\n", v); return 1; }
        }
        if (const char *v = lookup("DART_UMI_SEP")) if (strlen(v) == 1) md_umi_sep = v[0];      // (the default: what DART_UMI appends; a value that cannot be used is refused further down)
        if (const char *v = lookup("DART_MARKDUP_UMI_SEP")) {
            if (strlen(v) != 1) { fprintf(err_f, "Error! DART_MARKDUP_UMI_SEP=%s: one byte\n", v); return 1; }
            md_umi_sep = v[0];
        }
        // DART_PILEUP=1 beside DART_SORT_BAM=1: the sorted file's variant-site table <out>.sites.tsv, allele counts built on the device from the sorted records and
        // the index's text (dg_bam_pileup_finish) in place of a `samtools mpileup` over the file; behind the duplicate marking when that is on.  DART_PILEUP_MIN_ALT
        // (default 2), DART_PILEUP_EXCLUDE (default 0x704) and DART_PILEUP_MIN_MAPQ (default 0) are the filter.  Without the sort there is nothing to pile up: no
        // output is begun.
        pileup = env_on("DART_PILEUP");
        if (pileup && !sort_bam) {
            fprintf(err_f, "Error! DART_PILEUP=1 needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing\n");
            return 1;
        }
        if (const char *v = lookup("DART_PILEUP_MIN_ALT")) pu_min_alt = (uint32_t)strtoul(v, nullptr, 0);
        if (const char *v = lookup("DART_PILEUP_EXCLUDE")) pu_exclude = (uint32_t)strtoul(v, nullptr, 0);
        if (const char *v = lookup("DART_PILEUP_MIN_MAPQ")) pu_min_mapq = (uint32_t)strtoul(v, nullptr, 0);
        if (pileup && pu_min_alt == 0u) {
            fprintf(err_f, "Error! DART_PILEUP_MIN_ALT=0: a site has at least one observation of its top allele\n");
            return 1;
        }
        if (pileup) sites_path = std::string(out) + ".sites.tsv";
        // DART_QC=1 beside DART_SORT_BAM=1: the sorted file's QC tables <out>.qc.txt -- flag summary, per-chromosome counts, MAPQ, insert-size and read-length
        // histograms, per-cycle base / quality / error tables -- built on the device from the sorted records and the index's text (dg_bam_qc_finish) in place of
        // `samtools flagstat`, `idxstats` and `stats` over the file; behind the duplicate marking when that is on.  DART_QC_EXCLUDE (default 0x904) and
        // DART_QC_MIN_MAPQ (default 0) pick the records the per-cycle tables profile.  Without the sort there is nothing to look at: no output is begun.
        qc = env_on("DART_QC");
        if (qc && !sort_bam) {
            fprintf(err_f, "Error! DART_QC=1 needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing\n");
            return 1;
        }
        if (const char *v = lookup("DART_QC_EXCLUDE")) qc_exclude = (uint32_t)strtoul(v, nullptr, 0);
        if (const char *v = lookup("DART_QC_MIN_MAPQ")) qc_min_mapq = (uint32_t)strtoul(v, nullptr, 0);
        if (qc) qc_path = std::string(out) + ".qc.txt";
        // DART_RNA_METRICS=<annotation.gtf> beside DART_SORT_BAM=1: the sorted file's RNA-seq metrics <out>.rna_metrics.txt -- aligned bases by class (coding, UTR,
        // intronic, intergenic, ribosomal), records by class and by strand against the annotation, the gene-body coverage profile -- built on the device from the
        // sorted records and the annotation's transcripts (dg_bam_rna_finish) in place of Picard CollectRnaSeqMetrics over the file; behind the duplicate marking
        // and the tagging when they are on.  DART_RNA_EXCLUDE (default 0x904) and DART_RNA_MIN_MAPQ (default 0) pick the records, DART_RNA_MIN_COV (default 100)
        // the transcripts whose profile counts.  Without the sort there is nothing to look at: no output is begun.
        { const char *v = lookup("DART_RNA_METRICS"); rna_gtf = v && v[0] ? v : nullptr; }
        if (rna_gtf && !sort_bam) {
            fprintf(err_f, "Error! DART_RNA_METRICS=%s needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing\n", rna_gtf);
            return 1;
        }
        if (const char *v = lookup("DART_RNA_EXCLUDE")) rna_exclude = (uint32_t)strtoul(v, nullptr, 0);
        if (const char *v = lookup("DART_RNA_MIN_MAPQ")) rna_min_mapq = (uint32_t)strtoul(v, nullptr, 0);
        if (const char *v = lookup("DART_RNA_MIN_COV")) rna_min_cov = (uint64_t)strtoull(v, nullptr, 0);
        if (rna_gtf) rna_path = std::string(out) + ".rna_metrics.txt";
        // DART_BAM_TAGS beside DART_SORT_BAM=1: a comma list of MD, NM, ts (1 or all: all three): the sorted records get MD:Z, NM as edit distance and ts:A on the
        // device (dg_bam_tags_finish) behind the duplicate marking and before the first piece is compressed, in place of a `samtools calmd` over the file.  A word
        // that is none of them ends the run before any output exists; so does a missing sort: there is nothing to tag.
        if (const char *v = lookup("DART_BAM_TAGS")) {
            std::string bad;
            bam_tags = parse_bam_tags(v, bad);
            if (!bam_tags) {
                fprintf(err_f, "Error! DART_BAM_TAGS=%s: \"%s\" is none of MD, NM, ts (a comma list of them; 1 or all: all three)\n", v, bad.c_str());
                return 1;
            }
            if (!sort_bam) {
                fprintf(err_f, "Error! DART_BAM_TAGS=%s needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing\n", v);
                return 1;
            }
        }
        bam_dev_note = sort_bam ? (bgzf_dynamic ? ", bam=device+sorted+dyn" : ", bam=device+sorted") : bgzf_dynamic ? ", bam=device+dyn" : device_bam ? ", bam=device" : "";
        bam_host_note = !bam ? "" : ", bam=host";
        // A library of .gz FASTQ files small enough to be inflated whole (libdeflate, ~3x zlib; DART_GZ_WHOLE_MAX_GB per file, default 8) goes through the
        // parallel pipeline too -- if the inflated text is one the reference's gz reader and its plain reader see alike (FastqIndex::run); else, and for
        // everything libdeflate cannot take, the streaming reader.
        { const char *v = lookup("DART_GZ_WHOLE_MAX_GB"); gz_whole_max = (size_t)((v ? atof(v) : 8.0) * (double)(1ull << 30)); }
        streaming = lookup("DART_STREAMING") != nullptr;
        gz_stream = lookup("DART_GZ_STREAM") != nullptr;
        // DART_DEVICE_SAM=1: SAM text from the device's formatter (dg_batch_format_sam) instead of the host's; -bo keeps the host's (BAM is built from host text)
        device_sam = !bam && env_on("DART_DEVICE_SAM");
        // DART_DEVICE_FASTQ=1: the parallel pipeline hands its batches to the GPU as FASTQ text (dg_batch_upload_fastq); the streaming pipeline and -bo ignore it
        device_fastq = !bam_streams && env_on("DART_DEVICE_FASTQ");
        // DART_DEVICE_GZ=1 beside DART_DEVICE_FASTQ=1 and a device formatter (DART_DEVICE_SAM=1, or DART_DEVICE_BAM=1 with -bo: the host never holds the names and
        // qualities): a library whose files are all FASTQ .gz with a BGZF block in front is inflated on the device too (GzDevPlan, fast_fastq.h).  Anything else
        // -- also a library its check pass turns down -- runs as without the switch.
        device_gz = env_on("DART_DEVICE_GZ") && env_on("DART_DEVICE_FASTQ") && !bam_streams && !streaming && (device_bam || device_sam);
        // DART_TRIM_*: adapters, poly tails and low-quality ends are cut on the device inside the FASTQ upload (dg_set_trim), in place of a cutadapt / fastp pass over
        // the files in front of the mapper; pairs that became too short are dropped; <out>.trim.txt holds the sums.  Any of DART_TRIM_ADAPTER (ACGT letters, or
        // illumina / nextera / smallrna), DART_TRIM_QUAL (3' end), DART_TRIM_QUAL5 or DART_TRIM_POLY (letters of ACGT) turns the stage on; DART_TRIM_ADAPTER2 (mate
        // 2's, default the first), DART_TRIM_POLY_MIN (10), DART_TRIM_MIN_OVERLAP (3), DART_TRIM_ERR (permille, 100) and DART_TRIM_MIN_LEN (20) tune it.  The host no
        // longer knows names, qualities or even the read count of a batch, so the stage needs the device parser and a device formatter: without them the job is
        // refused -- untrimmed reads are never mapped silently.
        {
            int trc = parse_trim(lookup, err_f);
            if (trc != RUN) return trc;
            if (trim && !(device_fastq && (device_sam || device_bam) && !streaming)) {
                fprintf(err_f, "Error! DART_TRIM_* needs the device parser and a device formatter (DART_DEVICE_FASTQ=1 with DART_DEVICE_SAM=1, or with DART_DEVICE_BAM=1 and -bo): %s\n",
                        streaming ? "DART_STREAMING is set" : bam && !device_bam ? "DART_DEVICE_BAM=1 is missing" : !device_fastq ? "DART_DEVICE_FASTQ=1 is missing" : "DART_DEVICE_SAM=1 is missing");
                return 1;
            }
            // DART_UMI: the inline UMI is cut inside the same upload and goes to the end of the read's name, where DART_MARKDUP_UMI reads it; the same needs, the same refusal
            trc = parse_umi(lookup, err_f);
            if (trc != RUN) return trc;
            if (umi && !(device_fastq && (device_sam || device_bam) && !streaming)) {
                fprintf(err_f, "Error! DART_UMI needs the device parser and a device formatter (DART_DEVICE_FASTQ=1 with DART_DEVICE_SAM=1, or with DART_DEVICE_BAM=1 and -bo): %s\n",
                        streaming ? "DART_STREAMING is set" : bam && !device_bam ? "DART_DEVICE_BAM=1 is missing" : !device_fastq ? "DART_DEVICE_FASTQ=1 is missing" : "DART_DEVICE_SAM=1 is missing");
                return 1;
            }
            if (cuts()) trim_path = std::string(out) + ".trim.txt";
        }
        // DART_DEVICE_SJ=1: the junction table is counted, sorted and printed on the device (dg_batch_accumulate_sj per batch, dg_sj_merge / dg_sj_finish at the end);
        // works in both pipelines, with -o and -bo alike.  Without the switch the ordered writer fills a std::map, as always.
        device_sj = env_on("DART_DEVICE_SJ");
        if (const char *v = lookup("DART_GPUS")) { has_gpus = true; gpus = atoi(v); }
        // DART_SAME_DEVICE_TIMES=k (a test hook for one-GPU boxes): k "devices" that are all device 0 -- each with its own index replica, root context and clones --, so
        // that the multi-device pool (several roots, one ordered writer: Mapping.cpp:644-664) runs where only one GPU exists
        if (const char *v = lookup("DART_SAME_DEVICE_TIMES")) same_device_times = std::max(1, std::min(8, atoi(v)));
        // DART_GENE_COUNTS=<annotation.gtf>: reads per gene, counted on the device batch by batch (dg_batch_accumulate_genes) from the records in HBM, written as
        // <out>.genes.tab (STAR's ReadsPerGene.out.tab layout) after the alignments are complete.  Both pipelines, -o and -bo, beside every other switch.
        // DART_GENE_FEATURE (default exon) picks the GTF lines, DART_GENE_MIN_MAPQ (default 4, the -unique rule mapq > 3) the units that count as unique.
        { const char *v = lookup("DART_GENE_COUNTS"); gene_gtf = v && v[0] ? v : nullptr; }
        if (gene_gtf) genes_path = std::string(out) + ".genes.tab";
        { const char *v = lookup("DART_GENE_FEATURE"); if (v && v[0]) gene_feature = v; }
        if (const char *v = lookup("DART_GENE_MIN_MAPQ")) gene_min_mapq = (uint32_t)strtoul(v, nullptr, 0);
        // DART_TX_QUANT=<annotation.gtf>: abundance per transcript: every batch's units are folded into equivalence classes on the device (dg_batch_accumulate_tx)
        // where the gene counts count, an EM over the merged classes runs there at the end of the job (dg_tx_finish), and <out>.transcripts.tab is written after the
        // alignments are complete.  Both pipelines, -o and -bo, beside every other switch; it does not need the sort.  DART_TX_STRAND (0 unstranded, 1 forward,
        // 2 reverse; default 0), DART_TX_FRAG_MEAN (the mean fragment length of a library without pairs, default 200) and DART_TX_MAX_ROUNDS (default 1000): a
        // value that is no such number ends the run before any output exists.
        { const char *v = lookup("DART_TX_QUANT"); tx_gtf = v && v[0] ? v : nullptr; }
        if (tx_gtf) tx_path = std::string(out) + ".transcripts.tab";
        {
            const struct { const char *name; unsigned long long lo, hi; } num[3] = {{"DART_TX_STRAND", 0ull, 2ull}, {"DART_TX_FRAG_MEAN", 1ull, 0xFFFFFFFFull}, {"DART_TX_MAX_ROUNDS", 0ull, 0xFFFFFFFFull}};
            unsigned long long val[3] = {tx_strand, tx_frag_mean, tx_max_rounds};
            for (int k = 0; k < 3; k++) if (const char *v = lookup(num[k].name)) {
                char *end = nullptr;
                errno = 0;
                const unsigned long long x = strtoull(v, &end, 0);
                if (!(v[0] >= '0' && v[0] <= '9') || *end || errno || x < num[k].lo || x > num[k].hi) {
                    fprintf(err_f, "Error! %s=%s: a whole number from %llu to %llu is expected\n", num[k].name, v, num[k].lo, num[k].hi);
                    return 1;
                }
                val[k] = x;
            }
            tx_strand = (uint32_t)val[0]; tx_frag_mean = val[1]; tx_max_rounds = (uint32_t)val[2];
        }
        if (const char *v = lookup("DART_EXPECTED_READS")) { has_expected_reads = true; expected_reads = (uint64_t)atoll(v); }
        sync_aids = env_on("DART_SYNC_AIDS");
        timing = lookup("DART_TIMING") != nullptr;
        if (const char *v = lookup("DART_SORT_PIECE_MB")) sort_piece_mb = atof(v);
        // the parallel pipeline's threads (fast_fastq.h says why ONE writer) and its arenas
        if (const char *v = lookup("DART_WRITE_THREADS")) write_threads = std::max(1, atoi(v));
        if (const char *v = lookup("DART_FMT_THREADS")) fmt_threads = std::max(1, atoi(v));
        { const char *v = lookup("DART_WRITE"); write_mmap = v && strcmp(v, "mmap") == 0; }          // default pwrite (measured on tmpfs: 5.1 GB/s against 3.2 GB/s through a shared mapping)
        pinned = env_on("DART_PINNED");
        return RUN;
    }
};

// ---------------------------------------------------------------------------------------------
// which pipeline a library takes
// ---------------------------------------------------------------------------------------------
static bool check_read_format(const char *fn)   // CheckReadFormat, Mapping.cpp:718-726
{
    char b[1] = {0}; gzFile f = gzopen(fn, "rb");
    if (!f) return false;
    gzread(f, b, 1); gzclose(f);
    return b[0] == '@';
}

static bool starts_with_bgzf(const char *fn)
{
    unsigned char h[18 + 256]; FILE *f = fopen(fn, "rb");
    if (!f) return false;
    const size_t got = fread(h, 1, sizeof h, f); fclose(f);
    if (got < 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || h[3] != 4) return false;
    const size_t xlen = (size_t)h[10] | (size_t)h[11] << 8;
    for (size_t x = 12; x + 4 <= 12 + xlen && x + 4 <= got;) { const size_t slen = (size_t)h[x + 2] | (size_t)h[x + 3] << 8; if (h[x] == 'B' && h[x + 1] == 'C' && slen == 2) return true; x += 4 + slen; }
    return false;
}

// What the rule below needs to know about a read file.
struct FileProbe {
    bool gz = false;        // the name ends in ".gz" (what follows the path's last '.' is "gz")
    bool fastq = false;     // its first byte, inflated if need be, is '@'
    bool bgzf = false;      // it begins with a BGZF block
    long long size = -1;    // st_size; -1 = stat failed
};
static FileProbe probe(const std::string &fn)
{
    FileProbe f; struct stat st;
    f.gz = fn.substr(fn.find_last_of('.') + 1) == "gz";
    f.fastq = check_read_format(fn.c_str());
    f.bgzf = f.gz && starts_with_bgzf(fn.c_str());
    if (stat(fn.c_str(), &st) == 0) f.size = (long long)st.st_size;
    return f;
}

// The pipelines a library may take; they are tried in this order: BGZF inflated on the device, .gz inflated whole, then plain FASTQ in parallel or -- for
// whatever is left -- streaming.  The first two can still turn the library down when its turn comes (GzDevPlan::make refusing; FastqIndex::ok false after
// the inflation) and the next one is tried.
struct PipelineChoice {
    bool gz_device = false, gz_whole = false;
    bool plain = false;          // the last candidate is the parallel pipeline on plain FASTQ; false: it is the streaming pipeline
    // the first library only, before the device is touched: the slot pool is started when mate 1 alone looks like the parallel pipeline's -- also when a .gz
    // mate 2 makes the library stream after all
    bool head_pool = false;
};
// m2 == nullptr: one file.  libdeflate: the system has it (lib_deflate().ok()).
static PipelineChoice choose_pipelines(const Config &c, const FileProbe &m1, const FileProbe *m2, bool libdeflate)
{
    PipelineChoice ch;
    const bool may_parallel = !c.bam_streams && !c.streaming;
    // BGZF FASTQ inflated on the device: every file is FASTQ .gz with a BGZF block in front
    ch.gz_device = c.device_gz;
    // .gz FASTQ inflated whole: every file is FASTQ .gz of at most half of DART_GZ_WHOLE_MAX_GB
    ch.gz_whole = may_parallel && !c.gz_stream && libdeflate && c.gz_whole_max != 0;
    for (const FileProbe *m : {&m1, m2}) {
        if (!m) continue;
        if (!m->gz || !m->bgzf || !m->fastq) ch.gz_device = false;
        if (!m->gz || !m->fastq || m->size < 0 || (size_t)m->size > c.gz_whole_max / 2) ch.gz_whole = false;
    }
    // plain FASTQ through the parallel pipeline: mate 1 plain FASTQ, mate 2 not .gz (its format is compared when the library is opened); all else streams
    const bool m1_plain = may_parallel && m1.fastq && !m1.gz;
    ch.plain = m1_plain && (!m2 || !m2->gz);
    ch.head_pool = ch.gz_device || ch.gz_whole || m1_plain;
    return ch;
}
