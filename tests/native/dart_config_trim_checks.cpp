// CPU checks of the DART_TRIM_* switches as `dart` reads them before it touches the device (dart_amd/csrc/host/dart_config.h): Config::parse over command lines
// and environments -- off by default, every switch and its default, the adapter names, a bad adapter and the other values that end the run with their names,
// the statistics file's path, and the refusal without the device parser or without a device formatter.  Built and run by
// tests/test_dart_config_trim_host.py (once plain, once with -fsanitize=address,undefined).  No libdartgpu: dg_params is filled by hand.
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
static std::string adapter(const dg_trim &t, int i) { return std::string(t.adapter[i], t.n_adapter[i]); }

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: dart_config_trim_checks <scratch directory>\n"); return 1; }
    const std::string dir = argv[1], fq = dir + "/r.fq";
    { FILE *f = fopen(fq.c_str(), "w"); if (!f) { perror(fq.c_str()); return 1; } fputs("@r\nACGT\n+\nIIII\n", f); fclose(f); }
    const std::vector<std::string> bo = {"-i", "idx", "-f", fq, "-bo", dir + "/o.bam"}, o = {"-i", "idx", "-f", fq, "-o", dir + "/o.sam"};
    auto plus = [](std::map<std::string, std::string> m, std::initializer_list<std::pair<const std::string, std::string>> more) { for (auto &kv : more) m[kv.first] = kv.second; return m; };
    const std::map<std::string, std::string> dev_sam = {{"DART_DEVICE_FASTQ", "1"}, {"DART_DEVICE_SAM", "1"}}, dev_bam = {{"DART_DEVICE_FASTQ", "1"}, {"DART_DEVICE_BAM", "1"}};
    // off by default: the defaults are there all the same; the tuning switches alone turn nothing on
    { auto x = parse(o, {}); const dg_trim &t = x->c.trim_par;
      CHECK(x->rc == RUN && !x->c.trim && x->c.trim_path.empty() && x->err.empty());
      CHECK(t.flags == 0 && t.qual3 == 0 && t.qual5 == 0 && t.qual_base == 33 && t.min_overlap == 3 && t.max_err_permille == 100 && t.poly_mask == 0 && t.poly_min == 10 && t.min_len == 20);
      CHECK(t.n_adapter[0] == 0 && t.n_adapter[1] == 0); }
    { auto x = parse(o, {{"DART_TRIM_MIN_LEN", "30"}, {"DART_TRIM_ERR", "50"}, {"DART_TRIM_MIN_OVERLAP", "5"}, {"DART_TRIM_POLY_MIN", "12"}, {"DART_TRIM_ADAPTER", ""}, {"DART_TRIM_QUAL", "0"}, {"DART_TRIM_POLY", ""}});
      CHECK(x->rc == RUN && !x->c.trim && x->c.trim_par.min_len == 30 && x->c.trim_par.max_err_permille == 50 && x->c.trim_par.min_overlap == 5 && x->c.trim_par.poly_min == 12); }
    // each of the four turns the stage on; the path follows the output's name, with -o and with -bo
    { auto x = parse(o, plus(dev_sam, {{"DART_TRIM_ADAPTER", "ACGTTGCA"}})); const dg_trim &t = x->c.trim_par;
      CHECK(x->rc == RUN && x->c.trim && adapter(t, 0) == "ACGTTGCA" && adapter(t, 1) == "ACGTTGCA" && x->c.trim_path == dir + "/o.sam.trim.txt" && x->err.empty() && x->out.empty());
      CHECK(t.qual3 == 0 && t.qual5 == 0 && t.poly_mask == 0 && t.min_len == 20 && t.min_overlap == 3 && t.max_err_permille == 100 && t.qual_base == 33); }
    { auto x = parse(bo, plus(dev_bam, {{"DART_TRIM_QUAL", "20"}})); CHECK(x->rc == RUN && x->c.trim && x->c.trim_par.qual3 == 20 && x->c.trim_par.qual5 == 0 && x->c.trim_par.n_adapter[0] == 0 && x->c.trim_path == dir + "/o.bam.trim.txt"); }
    { auto x = parse(o, plus(dev_sam, {{"DART_TRIM_QUAL5", "15"}})); CHECK(x->rc == RUN && x->c.trim && x->c.trim_par.qual5 == 15 && x->c.trim_par.qual3 == 0); }
    { auto x = parse(o, plus(dev_sam, {{"DART_TRIM_POLY", "G"}})); CHECK(x->rc == RUN && x->c.trim && x->c.trim_par.poly_mask == 4u && x->c.trim_par.poly_min == 10); }
    { auto x = parse(o, plus(dev_sam, {{"DART_TRIM_POLY", "gAt"}, {"DART_TRIM_POLY_MIN", "7"}})); CHECK(x->rc == RUN && x->c.trim_par.poly_mask == 13u && x->c.trim_par.poly_min == 7); }
    // the adapter names; the second adapter defaults to the first and may be set alone
    const struct { const char *name, *bases; } named[3] = {{"illumina", "AGATCGGAAGAGC"}, {"nextera", "CTGTCTCTTATA"}, {"smallrna", "TGGAATTCTCGG"}};
    for (const auto &n : named) {
        auto x = parse(o, plus(dev_sam, {{"DART_TRIM_ADAPTER", n.name}}));
        CHECK(x->rc == RUN && x->c.trim && adapter(x->c.trim_par, 0) == n.bases && adapter(x->c.trim_par, 1) == n.bases);
        auto y = parse(o, plus(dev_sam, {{"DART_TRIM_ADAPTER", "ACGT"}, {"DART_TRIM_ADAPTER2", n.name}}));
        CHECK(y->rc == RUN && adapter(y->c.trim_par, 0) == "ACGT" && adapter(y->c.trim_par, 1) == n.bases);
    }
    { auto x = parse(o, plus(dev_sam, {{"DART_TRIM_ADAPTER2", "GGGTTT"}})); CHECK(x->rc == RUN && x->c.trim && x->c.trim_par.n_adapter[0] == 0 && adapter(x->c.trim_par, 1) == "GGGTTT"); }
    { auto x = parse(o, plus(dev_sam, {{"DART_TRIM_ADAPTER", std::string(64, 'A')}})); CHECK(x->rc == RUN && x->c.trim_par.n_adapter[0] == 64 && adapter(x->c.trim_par, 1) == std::string(64, 'A')); }
    // every switch at once
    { auto x = parse(o, plus(dev_sam, {{"DART_TRIM_ADAPTER", "illumina"}, {"DART_TRIM_ADAPTER2", "nextera"}, {"DART_TRIM_QUAL", "25"}, {"DART_TRIM_QUAL5", "10"}, {"DART_TRIM_POLY", "GA"},
                                       {"DART_TRIM_POLY_MIN", "15"}, {"DART_TRIM_MIN_OVERLAP", "4"}, {"DART_TRIM_ERR", "125"}, {"DART_TRIM_MIN_LEN", "36"}}));
      const dg_trim &t = x->c.trim_par;
      CHECK(x->rc == RUN && x->c.trim && adapter(t, 0) == "AGATCGGAAGAGC" && adapter(t, 1) == "CTGTCTCTTATA" && t.qual3 == 25 && t.qual5 == 10 && t.poly_mask == 5u && t.poly_min == 15);
      CHECK(t.min_overlap == 4 && t.max_err_permille == 125 && t.min_len == 36 && t.qual_base == 33 && t.flags == 0); }
    // a bad adapter, and the other values that cannot be used: the run ends, the switch is named, one line, whether or not the stage is on
    const struct { const char *name, *value; } refused[] = {{"DART_TRIM_ADAPTER", "ACGN"}, {"DART_TRIM_ADAPTER", "acgt"}, {"DART_TRIM_ADAPTER", "truseq"}, {"DART_TRIM_ADAPTER", "AC GT"},
                                                            {"DART_TRIM_ADAPTER2", "ACGU"}, {"DART_TRIM_QUAL", "94"}, {"DART_TRIM_QUAL", "-1"}, {"DART_TRIM_QUAL", "high"}, {"DART_TRIM_QUAL5", "20x"},
                                                            {"DART_TRIM_POLY", "GX"}, {"DART_TRIM_POLY", "1"}, {"DART_TRIM_POLY_MIN", "0"}, {"DART_TRIM_MIN_OVERLAP", "0"}, {"DART_TRIM_MIN_OVERLAP", "65"},
                                                            {"DART_TRIM_ERR", "1001"}, {"DART_TRIM_ERR", "0.1"}, {"DART_TRIM_MIN_LEN", "0"}, {"DART_TRIM_MIN_LEN", ""}, {"DART_TRIM_MIN_LEN", "1001"}};
    for (const auto &r : refused) for (int with = 0; with < 2; with++) {
        auto x = parse(o, plus(with ? plus(dev_sam, {{"DART_TRIM_QUAL", "20"}}) : std::map<std::string, std::string>(), {{r.name, r.value}}));
        CHECK(x->rc == 1 && x->out.empty() && x->err.rfind(std::string("Error! ") + r.name + "=" + r.value + ": ", 0) == 0 && std::count(x->err.begin(), x->err.end(), '\n') == 1);
    }
    { auto x = parse(o, plus(dev_sam, {{"DART_TRIM_ADAPTER", std::string(65, 'A')}})); CHECK(x->rc == 1 && x->err.rfind("Error! DART_TRIM_ADAPTER=", 0) == 0 && x->err.find("at most 64") != std::string::npos); }
    // the refusal: the stage needs the device parser and a device formatter; one line that says which is missing; untrimmed reads are never mapped silently
    const std::map<std::string, std::string> on = {{"DART_TRIM_ADAPTER", "illumina"}};
    const struct { const std::vector<std::string> *args; std::map<std::string, std::string> env; const char *missing; } no[] = {
        {&o, {}, "DART_DEVICE_FASTQ=1 is missing"}, {&o, {{"DART_DEVICE_SAM", "1"}}, "DART_DEVICE_FASTQ=1 is missing"}, {&o, {{"DART_DEVICE_FASTQ", "1"}}, "DART_DEVICE_SAM=1 is missing"},
        {&o, {{"DART_DEVICE_FASTQ", "1"}, {"DART_DEVICE_BAM", "1"}}, "DART_DEVICE_SAM=1 is missing"}, {&bo, {{"DART_DEVICE_FASTQ", "1"}, {"DART_DEVICE_SAM", "1"}}, "DART_DEVICE_BAM=1 is missing"},
        {&bo, {{"DART_DEVICE_BAM", "1"}}, "DART_DEVICE_FASTQ=1 is missing"}, {&bo, {}, "DART_DEVICE_BAM=1 is missing"},
        {&o, {{"DART_DEVICE_FASTQ", "1"}, {"DART_DEVICE_SAM", "1"}, {"DART_STREAMING", "1"}}, "DART_STREAMING is set"}};
    for (const auto &n : no) for (const char *sw : {"DART_TRIM_ADAPTER", "DART_TRIM_QUAL", "DART_TRIM_QUAL5", "DART_TRIM_POLY"}) {
        auto x = parse(*n.args, plus(n.env, {{sw, strcmp(sw, "DART_TRIM_ADAPTER") == 0 ? "illumina" : strcmp(sw, "DART_TRIM_POLY") == 0 ? "G" : "20"}}));
        CHECK(x->rc == 1 && x->out.empty() && x->err.rfind("Error! DART_TRIM_* needs the device parser and a device formatter", 0) == 0 && x->err.find(n.missing) != std::string::npos);
        CHECK(std::count(x->err.begin(), x->err.end(), '\n') == 1);
    }
    { auto x = parse(bo, plus(dev_bam, {{"DART_TRIM_ADAPTER", "illumina"}})); CHECK(x->rc == RUN && x->c.trim && x->c.device_bam && x->c.device_fastq); }
    { auto x = parse(o, plus(dev_sam, {{"DART_TRIM_ADAPTER", "illumina"}})); CHECK(x->rc == RUN && x->c.trim && x->c.device_sam && x->c.device_fastq); }
    // the same job without the switches is not refused
    for (const auto &n : no) { auto x = parse(*n.args, n.env); CHECK(x->rc == RUN && !x->c.trim); }
    // the usage text does not know the switches
    { auto a = parse({"-h"}, {}), b = parse({"-h"}, on);
      CHECK(a->rc == 0 && b->rc == 0 && a->out == b->out && a->err.empty() && b->err.empty() && a->out.find("TRIM") == std::string::npos); }
    printf("checks=%ld bad=%ld\n", n_checks, bad);
    return bad ? 1 : 0;
}
