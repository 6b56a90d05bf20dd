// CPU checks of the DART_BAM_TAGS switch as `dart` reads it before it touches the device (dart_amd/csrc/host/dart_config.h): Config::parse over command lines and
// environments -- off by default, the parse table of the comma list (every subset in every order, 1 and all, the words it does not know and which of them the message
// names), the refusal without the sort and its place among the other stages' (behind the QC tables'), and the usage text, which the switch does not touch.  Built
// and run by tests/test_dart_config_tags_host.py (once plain, once with -fsanitize=address,undefined).  No libdartgpu: dg_params is filled by hand.
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
    if (argc != 2) { fprintf(stderr, "usage: dart_config_tags_checks <scratch directory>\n"); return 1; }
    const std::string dir = argv[1], fq = dir + "/r.fq";
    { FILE *f = fopen(fq.c_str(), "w"); if (!f) { perror(fq.c_str()); return 1; } fputs("@r\nACGT\n+\nIIII\n", f); fclose(f); }
    const std::vector<std::string> bo = {"-i", "idx", "-f", fq, "-bo", dir + "/o.bam"}, o = {"-i", "idx", "-f", fq, "-o", dir + "/o.sam"};
    const std::map<std::string, std::string> sorted = {{"DART_DEVICE_BAM", "1"}, {"DART_SORT_BAM", "1"}};
    auto plus = [](std::map<std::string, std::string> m, std::initializer_list<std::pair<const std::string, std::string>> more) { for (auto &kv : more) m[kv.first] = kv.second; return m; };
    const uint32_t MD = DG_TAG_MD, NM = DG_TAG_NM, TS = DG_TAG_TS;
    CHECK(MD == 1u && NM == 2u && TS == 4u);
    // off by default
    { auto x = parse(bo, sorted); CHECK(x->rc == RUN && x->c.bam_tags == 0u && x->err.empty()); }
    { auto x = parse(o, {}); CHECK(x->rc == RUN && x->c.bam_tags == 0u); }
    // the parse table: what the value gives
    const struct { const char *value; uint32_t bits; } good[] = {
        {"1", MD | NM | TS}, {"all", MD | NM | TS}, {"MD", MD}, {"NM", NM}, {"ts", TS}, {"MD,NM", MD | NM}, {"NM,MD", MD | NM}, {"MD,ts", MD | TS}, {"ts,MD", MD | TS}, {"NM,ts", NM | TS},
        {"ts,NM", NM | TS}, {"MD,NM,ts", MD | NM | TS}, {"ts,NM,MD", MD | NM | TS}, {"NM,ts,MD", MD | NM | TS}, {"MD,MD", MD}, {"ts,ts,NM,ts", NM | TS}};
    for (const auto &g : good) {
        auto x = parse(bo, plus(sorted, {{"DART_BAM_TAGS", g.value}}));
        CHECK(x->rc == RUN && x->c.bam_tags == g.bits && x->err.empty() && x->out.empty());
        std::string w; CHECK(Config::parse_bam_tags(g.value, w) == g.bits && w.empty());
    }
    // and what it refuses: one line, exit 1, the first word that is none of the three
    const struct { const char *value, *word; } wrong[] = {
        {"0", "0"}, {"2", "2"}, {"", ""}, {"md", "md"}, {"Md", "Md"}, {"TS", "TS"}, {"nm", "nm"}, {"ALL", "ALL"}, {"all,MD", "all"}, {"1,MD", "1"}, {"MD,1", "1"}, {"MD,all", "all"}, {"MD,", ""},
        {",MD", ""}, {"MD,,NM", ""}, {"MD, NM", " NM"}, {"MD NM", "MD NM"}, {"MD;NM", "MD;NM"}, {"MD,XS", "XS"}, {"XS,YS", "XS"}, {"MD,NM,ts,NH", "NH"}, {"MDZ", "MDZ"}, {"M", "M"}, {"yes", "yes"}};
    for (const auto &w : wrong) {
        auto x = parse(bo, plus(sorted, {{"DART_BAM_TAGS", w.value}}));
        CHECK(x->rc == 1 && x->out.empty() && x->err == std::string("Error! DART_BAM_TAGS=") + w.value + ": \"" + w.word + "\" is none of MD, NM, ts (a comma list of them; 1 or all: all three)\n");
        std::string got = "?"; CHECK(Config::parse_bam_tags(w.value, got) == 0u && got == w.word);
    }
    // a bad word is reported whether or not the sort is there; a good value without the sort: the other switches' wording, the three forms of a missing switch
    { auto x = parse(bo, {{"DART_BAM_TAGS", "MD,XS"}}); CHECK(x->rc == 1 && x->err.find("\"XS\" is none of MD, NM, ts") != std::string::npos); }
    const std::string T = " needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing\n";
    { auto x = parse(bo, {{"DART_BAM_TAGS", "all"}, {"DART_DEVICE_BAM", "1"}}); CHECK(x->rc == 1 && x->out.empty() && x->err == "Error! DART_BAM_TAGS=all" + T); }
    { auto x = parse(bo, {{"DART_BAM_TAGS", "MD,ts"}}); CHECK(x->rc == 1 && x->out.empty() && x->err == "Error! DART_BAM_TAGS=MD,ts" + T); }
    { auto x = parse(o, {{"DART_BAM_TAGS", "1"}}); CHECK(x->rc == 1 && x->out.empty() && x->err == "Error! DART_BAM_TAGS=1" + T); }
    // the sort's own error comes first
    { auto x = parse(bo, {{"DART_BAM_TAGS", "all"}, {"DART_SORT_BAM", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1: DART_DEVICE_BAM=1 is missing\n"); }
    { auto x = parse(o, {{"DART_BAM_TAGS", "all"}, {"DART_SORT_BAM", "1"}, {"DART_DEVICE_BAM", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1: -bo is missing\n"); }
    // its place among the checks: behind the index's, the coverage's, the duplicate marking's, the allele counts' and the QC tables' -- a run that fails several reports the first
    { auto x = parse(bo, {{"DART_BAM_TAGS", "all"}, {"DART_QC", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_QC=1" + T); }
    { auto x = parse(bo, {{"DART_BAM_TAGS", "all"}, {"DART_PILEUP", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_PILEUP=1" + T); }
    { auto x = parse(bo, {{"DART_BAM_TAGS", "all"}, {"DART_MARK_DUPLICATES", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_MARK_DUPLICATES=1" + T); }
    { auto x = parse(bo, {{"DART_BAM_TAGS", "all"}, {"DART_COVERAGE", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_COVERAGE=1" + T); }
    { auto x = parse(bo, {{"DART_BAM_TAGS", "all"}, {"DART_BAM_INDEX", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_BAM_INDEX=1" + T); }
    // beside the other stages behind the sort: each keeps its own values; the switch opens no file of its own
    { auto x = parse(bo, plus(sorted, {{"DART_BAM_TAGS", "NM,ts"}, {"DART_QC", "1"}, {"DART_PILEUP", "1"}, {"DART_COVERAGE", "2"}, {"DART_MARK_DUPLICATES", "1"}, {"DART_BAM_INDEX", "1"}}));
      CHECK(x->rc == RUN && x->c.bam_tags == (NM | TS) && x->c.qc && x->c.pileup && x->c.coverage == 2 && x->c.mark_dups && x->c.bam_index);
      CHECK(x->c.qc_path == dir + "/o.bam.qc.txt" && x->c.sites_path == dir + "/o.bam.sites.tsv" && x->c.md_path == dir + "/o.bam.markdup.txt" && x->c.bai_path == dir + "/o.bam.bai"); }
    // the usage text does not know the switch: the same bytes with and without it
    { auto a = parse({"-h"}, {}), b = parse({"-h"}, plus(sorted, {{"DART_BAM_TAGS", "all"}}));
      CHECK(a->rc == 0 && b->rc == 0 && a->out == b->out && a->err.empty() && b->err.empty());
      CHECK(!a->out.empty() && a->out.find("TAGS") == std::string::npos && a->out.find("calmd") == std::string::npos); }
    printf("checks=%ld bad=%ld\n", n_checks, bad);
    return bad ? 1 : 0;
}
