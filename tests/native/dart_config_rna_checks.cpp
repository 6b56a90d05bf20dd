// CPU checks of the DART_RNA_METRICS switches as `dart` reads them before it touches the device (dart_amd/csrc/host/dart_config.h): Config::parse over command
// lines and environments -- the defaults, every value read once, the refusal without the sort and its place among the other stages' (behind the QC's), the
// output's path, and the usage text, which the switch does not touch.  Built and run by tests/test_dart_config_rna_host.py (once plain, once with
// -fsanitize=address,undefined).  No libdartgpu: dg_params is filled by hand.
#include "dart_config.h"
#include <map>
#include <memory>

static long bad = 0, n_checks = 0;
#define CHECK(x) do { n_checks++; if (!(x)) { bad++; printf("line %d: %s\n", __LINE__, #x); } } while (0)

static std::map<std::string, std::string> g_env;
static const char *table_lookup(const char *k) { auto it = g_env.find(k); return it == g_env.end() ? nullptr : it->second.c_str(); }

struct Run { Config c; int rc = 0; std::string out, err; };
static std::unique_ptr<Run> parse(std::vector<std::string> args, std::map<std::string, std::string> env)
{
    static std::vector<std::vector<std::string>> keep;      // Config keeps pointers into argv and the environment
    static std::vector<std::map<std::string, std::string>> keep_env;
    args.insert(args.begin(), "dart");
    keep.push_back(args); keep_env.push_back(env);
    g_env = keep_env.back();
    std::vector<char *> argv;
    for (auto &s : keep.back()) argv.push_back(&s[0]);
    argv.push_back(nullptr);
    std::unique_ptr<Run> x(new Run());
    dg_params p; memset(&p, 0, sizeof p);
    p.max_dup = 100; p.max_intron = 500000; p.min_intron = 5;
    char *ob = nullptr, *eb = nullptr; size_t on = 0, en = 0;
    FILE *out = open_memstream(&ob, &on), *err = open_memstream(&eb, &en);
    x->rc = x->c.parse((int)argv.size() - 1, argv.data(), table_lookup, p, out, err);
    fclose(out); fclose(err);
    x->out.assign(ob, on); x->err.assign(eb, en);
    free(ob); free(eb);
    return x;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: dart_config_rna_checks <scratch directory>\n"); return 1; }
    const std::string dir = argv[1], fq = dir + "/r.fq";
    { FILE *f = fopen(fq.c_str(), "w"); if (!f) { perror(fq.c_str()); return 1; } fputs("@r\nACGT\n+\nIIII\n", f); fclose(f); }
    const std::vector<std::string> bo = {"-i", "idx", "-f", fq, "-bo", dir + "/o.bam"}, o = {"-i", "idx", "-f", fq, "-o", dir + "/o.sam"};
    const std::map<std::string, std::string> sorted = {{"DART_DEVICE_BAM", "1"}, {"DART_SORT_BAM", "1"}};
    auto plus = [](std::map<std::string, std::string> m, std::initializer_list<std::pair<const std::string, std::string>> more) { for (auto &kv : more) m[kv.first] = kv.second; return m; };
    // off by default, and with an empty value; the defaults are there whether or not the switch is on
    { auto x = parse(bo, sorted); CHECK(x->rc == RUN && !x->c.rna_gtf && x->c.rna_path.empty() && x->c.rna_exclude == 0x904 && x->c.rna_min_mapq == 0 && x->c.rna_min_cov == 100 && x->err.empty()); }
    { auto x = parse(bo, plus(sorted, {{"DART_RNA_METRICS", ""}})); CHECK(x->rc == RUN && !x->c.rna_gtf && x->c.rna_path.empty()); }
    { auto x = parse(o, {}); CHECK(x->rc == RUN && !x->c.rna_gtf && x->c.rna_path.empty() && x->c.rna_exclude == 0x904 && x->c.rna_min_cov == 100); }
    { auto x = parse(o, {{"DART_RNA_METRICS", ""}}); CHECK(x->rc == RUN && !x->c.rna_gtf); }
    // on: the path follows the output's name; the three values in decimal, hexadecimal and octal
    { auto x = parse(bo, plus(sorted, {{"DART_RNA_METRICS", "a.gtf"}}));
      CHECK(x->rc == RUN && x->c.rna_gtf && std::string(x->c.rna_gtf) == "a.gtf" && x->c.rna_path == dir + "/o.bam.rna_metrics.txt" && x->c.rna_exclude == 0x904 && x->c.rna_min_mapq == 0 && x->c.rna_min_cov == 100 && x->err.empty() && x->out.empty()); }
    { auto x = parse(bo, plus(sorted, {{"DART_RNA_METRICS", "/p/a.gtf"}, {"DART_RNA_EXCLUDE", "0x704"}, {"DART_RNA_MIN_MAPQ", "010"}, {"DART_RNA_MIN_COV", "0"}}));
      CHECK(x->rc == RUN && x->c.rna_gtf && x->c.rna_exclude == 0x704 && x->c.rna_min_mapq == 8 && x->c.rna_min_cov == 0); }
    { auto x = parse(bo, plus(sorted, {{"DART_RNA_METRICS", "a.gtf"}, {"DART_RNA_EXCLUDE", "4"}, {"DART_RNA_MIN_MAPQ", "60"}, {"DART_RNA_MIN_COV", "0x100000000"}}));
      CHECK(x->rc == RUN && x->c.rna_exclude == 4 && x->c.rna_min_mapq == 60 && x->c.rna_min_cov == 0x100000000ull); }
    { auto x = parse(bo, plus(sorted, {{"DART_RNA_EXCLUDE", "0"}, {"DART_RNA_MIN_MAPQ", "3"}, {"DART_RNA_MIN_COV", "7"}})); CHECK(x->rc == RUN && !x->c.rna_gtf && x->c.rna_path.empty() && x->c.rna_exclude == 0 && x->c.rna_min_mapq == 3 && x->c.rna_min_cov == 7); }
    // beside the other stages behind the sort, and beside the gene counts with a GTF of their own: each keeps its own values and its own path
    { auto x = parse(bo, plus(sorted, {{"DART_RNA_METRICS", "a.gtf"}, {"DART_RNA_EXCLUDE", "0x100"}, {"DART_QC", "1"}, {"DART_PILEUP", "1"}, {"DART_COVERAGE", "2"}, {"DART_MARK_DUPLICATES", "1"}, {"DART_BAM_INDEX", "1"},
                                      {"DART_GENE_COUNTS", "b.gtf"}, {"DART_BAM_TAGS", "MD"}}));
      CHECK(x->rc == RUN && x->c.rna_gtf && x->c.qc && x->c.pileup && x->c.coverage == 2 && x->c.rna_exclude == 0x100 && x->c.qc_exclude == 0x904 && x->c.pu_exclude == 0x704 && x->c.cov_exclude == 0x704 && x->c.mark_dups && x->c.bam_index);
      CHECK(x->c.gene_gtf && std::string(x->c.gene_gtf) == "b.gtf" && std::string(x->c.rna_gtf) == "a.gtf" && x->c.bam_tags == DG_TAG_MD);
      CHECK(x->c.rna_path == dir + "/o.bam.rna_metrics.txt" && x->c.qc_path == dir + "/o.bam.qc.txt" && x->c.genes_path == dir + "/o.bam.genes.tab" && x->c.bai_path == dir + "/o.bam.bai"); }
    // the refusals: one line, exit 1, the three forms of a missing switch; the sort's own error comes first
    const std::string T = " needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing\n";
    { auto x = parse(bo, {{"DART_RNA_METRICS", "a.gtf"}, {"DART_DEVICE_BAM", "1"}}); CHECK(x->rc == 1 && x->out.empty() && x->err == "Error! DART_RNA_METRICS=a.gtf" + T); }
    { auto x = parse(bo, {{"DART_RNA_METRICS", "a.gtf"}}); CHECK(x->rc == 1 && x->out.empty() && x->err == "Error! DART_RNA_METRICS=a.gtf" + T); }
    { auto x = parse(o, {{"DART_RNA_METRICS", "a.gtf"}}); CHECK(x->rc == 1 && x->out.empty() && x->err == "Error! DART_RNA_METRICS=a.gtf" + T); }
    { auto x = parse(bo, {{"DART_RNA_METRICS", "a.gtf"}, {"DART_SORT_BAM", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1: DART_DEVICE_BAM=1 is missing\n"); }
    { auto x = parse(o, {{"DART_RNA_METRICS", "a.gtf"}, {"DART_SORT_BAM", "1"}, {"DART_DEVICE_BAM", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1: -bo is missing\n"); }
    // its place among the checks: behind the QC's and in front of the tags' -- a run that fails several reports the first
    { auto x = parse(bo, {{"DART_RNA_METRICS", "a.gtf"}, {"DART_QC", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_QC=1" + T); }
    { auto x = parse(bo, {{"DART_RNA_METRICS", "a.gtf"}, {"DART_PILEUP", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_PILEUP=1" + T); }
    { auto x = parse(bo, {{"DART_RNA_METRICS", "a.gtf"}, {"DART_BAM_INDEX", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_BAM_INDEX=1" + T); }
    { auto x = parse(bo, {{"DART_RNA_METRICS", "a.gtf"}, {"DART_BAM_TAGS", "MD"}}); CHECK(x->rc == 1 && x->err == "Error! DART_RNA_METRICS=a.gtf" + T); }
    // the usage text does not know the switch: the same bytes with and without it, 22 lines
    { auto a = parse({"-h"}, {}), b = parse({"-h"}, plus(sorted, {{"DART_RNA_METRICS", "a.gtf"}}));
      CHECK(a->rc == 0 && b->rc == 0 && a->out == b->out && a->err.empty() && b->err.empty());
      CHECK(std::count(a->out.begin(), a->out.end(), '\n') == 22 && a->out.find("RNA") == std::string::npos && a->out.find("rna") == std::string::npos); }
    printf("checks=%ld bad=%ld\n", n_checks, bad);
    return bad ? 1 : 0;
}
