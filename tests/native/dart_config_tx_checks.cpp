// CPU checks of the DART_TX_QUANT switches as `dart` reads them before it touches the device (dart_amd/csrc/host/dart_config.h): Config::parse over command
// lines and environments -- the defaults, every value read once, the output's path with -o and with -bo, no need of the sort, the values that end the run with
// their names, and the usage text, which the switch does not touch.  Built and run by tests/test_dart_config_tx_host.py (once plain, once with
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
    if (argc != 2) { fprintf(stderr, "usage: dart_config_tx_checks <scratch directory>\n"); return 1; }
    const std::string dir = argv[1], fq = dir + "/r.fq";
    { FILE *f = fopen(fq.c_str(), "w"); if (!f) { perror(fq.c_str()); return 1; } fputs("@r\nACGT\n+\nIIII\n", f); fclose(f); }
    const std::vector<std::string> bo = {"-i", "idx", "-f", fq, "-bo", dir + "/o.bam"}, o = {"-i", "idx", "-f", fq, "-o", dir + "/o.sam"};
    auto plus = [](std::map<std::string, std::string> m, std::initializer_list<std::pair<const std::string, std::string>> more) { for (auto &kv : more) m[kv.first] = kv.second; return m; };
    const std::map<std::string, std::string> on = {{"DART_TX_QUANT", "a.gtf"}};
    // off by default, and with an empty value; the defaults are there whether or not the switch is on
    { auto x = parse(o, {}); CHECK(x->rc == RUN && !x->c.tx_gtf && x->c.tx_path.empty() && x->c.tx_strand == 0 && x->c.tx_frag_mean == 200 && x->c.tx_max_rounds == 1000 && x->err.empty()); }
    { auto x = parse(o, {{"DART_TX_QUANT", ""}}); CHECK(x->rc == RUN && !x->c.tx_gtf && x->c.tx_path.empty()); }
    { auto x = parse(bo, {{"DART_TX_STRAND", "2"}, {"DART_TX_FRAG_MEAN", "350"}, {"DART_TX_MAX_ROUNDS", "0"}}); CHECK(x->rc == RUN && !x->c.tx_gtf && x->c.tx_path.empty() && x->c.tx_strand == 2 && x->c.tx_frag_mean == 350 && x->c.tx_max_rounds == 0); }
    // on, with -o and with -bo, in both pipelines' settings, without the sort: the path follows the output's name
    { auto x = parse(o, on); CHECK(x->rc == RUN && x->c.tx_gtf && std::string(x->c.tx_gtf) == "a.gtf" && x->c.tx_path == dir + "/o.sam.transcripts.tab" && x->c.tx_strand == 0 && x->c.tx_frag_mean == 200 && x->c.tx_max_rounds == 1000 && x->err.empty() && x->out.empty()); }
    { auto x = parse(bo, on); CHECK(x->rc == RUN && x->c.tx_gtf && x->c.tx_path == dir + "/o.bam.transcripts.tab" && !x->c.sort_bam); }
    { auto x = parse(o, plus(on, {{"DART_STREAMING", "1"}})); CHECK(x->rc == RUN && x->c.tx_gtf && x->c.streaming); }
    { auto x = parse(bo, plus(on, {{"DART_DEVICE_BAM", "1"}, {"DART_SORT_BAM", "1"}, {"DART_RNA_METRICS", "b.gtf"}, {"DART_GENE_COUNTS", "c.gtf"}}));
      CHECK(x->rc == RUN && std::string(x->c.tx_gtf) == "a.gtf" && std::string(x->c.rna_gtf) == "b.gtf" && std::string(x->c.gene_gtf) == "c.gtf");
      CHECK(x->c.tx_path == dir + "/o.bam.transcripts.tab" && x->c.rna_path == dir + "/o.bam.rna_metrics.txt" && x->c.genes_path == dir + "/o.bam.genes.tab"); }
    // the values: decimal, hexadecimal, octal; the bounds of each
    { auto x = parse(o, plus(on, {{"DART_TX_STRAND", "1"}, {"DART_TX_FRAG_MEAN", "0x100"}, {"DART_TX_MAX_ROUNDS", "010"}})); CHECK(x->rc == RUN && x->c.tx_strand == 1 && x->c.tx_frag_mean == 256 && x->c.tx_max_rounds == 8); }
    { auto x = parse(o, plus(on, {{"DART_TX_STRAND", "0"}, {"DART_TX_FRAG_MEAN", "1"}, {"DART_TX_MAX_ROUNDS", "4294967295"}})); CHECK(x->rc == RUN && x->c.tx_strand == 0 && x->c.tx_frag_mean == 1 && x->c.tx_max_rounds == 4294967295u); }
    // a bad value ends the run and is named, whether or not the stage is on; nothing else is printed
    const struct { const char *name, *value; } refused[] = {{"DART_TX_STRAND", "3"}, {"DART_TX_STRAND", "-1"}, {"DART_TX_STRAND", "forward"}, {"DART_TX_STRAND", ""}, {"DART_TX_STRAND", "1x"}, {"DART_TX_STRAND", " 1"},
                                                            {"DART_TX_FRAG_MEAN", "0"}, {"DART_TX_FRAG_MEAN", "2e2"}, {"DART_TX_FRAG_MEAN", "4294967296"}, {"DART_TX_FRAG_MEAN", "99999999999999999999999"},
                                                            {"DART_TX_MAX_ROUNDS", "-5"}, {"DART_TX_MAX_ROUNDS", "many"}, {"DART_TX_MAX_ROUNDS", "4294967296"}, {"DART_TX_MAX_ROUNDS", "+3"}};
    for (const auto &r : refused) for (int with = 0; with < 2; with++) {
        auto x = parse(with ? o : bo, plus(with ? on : std::map<std::string, std::string>(), {{r.name, r.value}}));
        CHECK(x->rc == 1 && x->out.empty() && x->err.rfind(std::string("Error! ") + r.name + "=" + r.value + ": ", 0) == 0 && std::count(x->err.begin(), x->err.end(), '\n') == 1);
    }
    // the first bad value is the one named
    { auto x = parse(o, plus(on, {{"DART_TX_STRAND", "9"}, {"DART_TX_MAX_ROUNDS", "x"}})); CHECK(x->rc == 1 && x->err.rfind("Error! DART_TX_STRAND=9: ", 0) == 0); }
    // the usage text does not know the switch: the same bytes with and without it, 22 lines
    { auto a = parse({"-h"}, {}), b = parse({"-h"}, on);
      CHECK(a->rc == 0 && b->rc == 0 && a->out == b->out && a->err.empty() && b->err.empty());
      CHECK(std::count(a->out.begin(), a->out.end(), '\n') == 22 && a->out.find("TX_QUANT") == std::string::npos && a->out.find("transcripts.tab") == std::string::npos); }
    printf("checks=%ld bad=%ld\n", n_checks, bad);
    return bad ? 1 : 0;
}
