// CPU checks of the DART_QC switches as `dart` reads them before it touches the device (dart_amd/csrc/host/dart_config.h): Config::parse over command lines and
// environments -- the defaults, every value read once, the refusals without the sort and their place among the other stages' (behind the allele counts'), the
// output's path, and the usage text, which the switch does not touch.  Built and run by tests/test_dart_config_qc_host.py (once plain, once with
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
    g_env = env;
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
    if (argc != 2) { fprintf(stderr, "usage: dart_config_qc_checks <scratch directory>\n"); return 1; }
    const std::string dir = argv[1], fq = dir + "/r.fq";
    { FILE *f = fopen(fq.c_str(), "w"); if (!f) { perror(fq.c_str()); return 1; } fputs("@r\nACGT\n+\nIIII\n", f); fclose(f); }
    const std::vector<std::string> bo = {"-i", "idx", "-f", fq, "-bo", dir + "/o.bam"}, o = {"-i", "idx", "-f", fq, "-o", dir + "/o.sam"};
    const std::map<std::string, std::string> sorted = {{"DART_DEVICE_BAM", "1"}, {"DART_SORT_BAM", "1"}};
    auto plus = [](std::map<std::string, std::string> m, std::initializer_list<std::pair<const std::string, std::string>> more) { for (auto &kv : more) m[kv.first] = kv.second; return m; };
    // off by default; the filter's defaults are there whether or not the switch is on
    { auto x = parse(bo, sorted); CHECK(x->rc == RUN && !x->c.qc && x->c.qc_path.empty() && x->c.qc_exclude == 0x904 && x->c.qc_min_mapq == 0 && x->err.empty()); }
    { auto x = parse(bo, plus(sorted, {{"DART_QC", "0"}})); CHECK(x->rc == RUN && !x->c.qc && x->c.qc_path.empty()); }
    { auto x = parse(o, {}); CHECK(x->rc == RUN && !x->c.qc && x->c.qc_path.empty() && x->c.qc_exclude == 0x904); }
    // on: the path follows the output's name; the two values in decimal, hexadecimal and octal
    { auto x = parse(bo, plus(sorted, {{"DART_QC", "1"}})); CHECK(x->rc == RUN && x->c.qc && x->c.qc_path == dir + "/o.bam.qc.txt" && x->c.qc_exclude == 0x904 && x->c.qc_min_mapq == 0 && x->err.empty() && x->out.empty()); }
    { auto x = parse(bo, plus(sorted, {{"DART_QC", "1"}, {"DART_QC_EXCLUDE", "0x704"}, {"DART_QC_MIN_MAPQ", "010"}})); CHECK(x->rc == RUN && x->c.qc && x->c.qc_exclude == 0x704 && x->c.qc_min_mapq == 8); }
    { auto x = parse(bo, plus(sorted, {{"DART_QC", "1"}, {"DART_QC_EXCLUDE", "4"}, {"DART_QC_MIN_MAPQ", "60"}})); CHECK(x->rc == RUN && x->c.qc_exclude == 4 && x->c.qc_min_mapq == 60); }
    { auto x = parse(bo, plus(sorted, {{"DART_QC_EXCLUDE", "0"}, {"DART_QC_MIN_MAPQ", "3"}})); CHECK(x->rc == RUN && !x->c.qc && x->c.qc_path.empty() && x->c.qc_exclude == 0 && x->c.qc_min_mapq == 3); }
    // beside the other stages behind the sort: each keeps its own values and its own path
    { auto x = parse(bo, plus(sorted, {{"DART_QC", "1"}, {"DART_QC_EXCLUDE", "0x100"}, {"DART_PILEUP", "1"}, {"DART_COVERAGE", "2"}, {"DART_MARK_DUPLICATES", "1"}, {"DART_BAM_INDEX", "1"}}));
      CHECK(x->rc == RUN && x->c.qc && x->c.pileup && x->c.coverage == 2 && x->c.qc_exclude == 0x100 && x->c.pu_exclude == 0x704 && x->c.cov_exclude == 0x704 && x->c.mark_dups && x->c.bam_index);
      CHECK(x->c.qc_path == dir + "/o.bam.qc.txt" && x->c.sites_path == dir + "/o.bam.sites.tsv" && x->c.md_path == dir + "/o.bam.markdup.txt" && x->c.bai_path == dir + "/o.bam.bai"); }
    // the refusals: one line, exit 1, the three forms of a missing switch; the sort's own error comes first
    const std::string T = " needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing\n";
    { auto x = parse(bo, {{"DART_QC", "1"}, {"DART_DEVICE_BAM", "1"}}); CHECK(x->rc == 1 && x->out.empty() && x->err == "Error! DART_QC=1" + T); }
    { auto x = parse(bo, {{"DART_QC", "1"}}); CHECK(x->rc == 1 && x->out.empty() && x->err == "Error! DART_QC=1" + T); }
    { auto x = parse(o, {{"DART_QC", "1"}}); CHECK(x->rc == 1 && x->out.empty() && x->err == "Error! DART_QC=1" + T); }
    { auto x = parse(bo, {{"DART_QC", "1"}, {"DART_SORT_BAM", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1: DART_DEVICE_BAM=1 is missing\n"); }
    { auto x = parse(o, {{"DART_QC", "1"}, {"DART_SORT_BAM", "1"}, {"DART_DEVICE_BAM", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1: -bo is missing\n"); }
    // its place among the checks: behind the index's, the coverage's, the duplicate marking's and the allele counts' -- a run that fails several reports the first
    { auto x = parse(bo, {{"DART_QC", "1"}, {"DART_PILEUP", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_PILEUP=1" + T); }
    { auto x = parse(bo, {{"DART_QC", "1"}, {"DART_MARK_DUPLICATES", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_MARK_DUPLICATES=1" + T); }
    { auto x = parse(bo, {{"DART_QC", "1"}, {"DART_COVERAGE", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_COVERAGE=1" + T); }
    { auto x = parse(bo, {{"DART_QC", "1"}, {"DART_BAM_INDEX", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_BAM_INDEX=1" + T); }
    { auto x = parse(bo, plus(sorted, {{"DART_QC", "1"}, {"DART_PILEUP", "1"}, {"DART_PILEUP_MIN_ALT", "0"}})); CHECK(x->rc == 1 && x->err == "Error! DART_PILEUP_MIN_ALT=0: a site has at least one observation of its top allele\n"); }
    // the usage text does not know the switch: the same bytes with and without it, 22 lines, the -bo line's list of stages as it was
    { auto a = parse({"-h"}, {}), b = parse({"-h"}, plus(sorted, {{"DART_QC", "1"}}));
      CHECK(a->rc == 0 && b->rc == 0 && a->out == b->out && a->err.empty() && b->err.empty());
      CHECK(std::count(a->out.begin(), a->out.end(), '\n') == 22 && a->out.find("QC") == std::string::npos && a->out.find("qc") == std::string::npos);
      CHECK(a->out.find("DART_MARK_DUPLICATES=1: flag 0x400 set on the device)\n         -j            splice junction output filename [junctions.tab]\n") != std::string::npos); }
    printf("checks=%ld bad=%ld\n", n_checks, bad);
    return bad ? 1 : 0;
}
