// CPU checks of the DART_MARKDUP_UMI and DART_UMI switches as `dart` reads them before it touches the device (dart_amd/csrc/host/dart_config.h): Config::parse over command lines
// and environments -- off by default, exact and edit1, the separator and its default, the values that end the run with their names, the refusal without
// DART_MARK_DUPLICATES=1, the place among the other checks; DART_UMI, DART_UMI_SKIP and DART_UMI_SEP with their refusals.  Built and run by tests/test_dart_config_umi_host.py (once plain, once with
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
    if (argc != 2) { fprintf(stderr, "usage: dart_config_umi_checks <scratch directory>\n"); return 1; }
    const std::string dir = argv[1], fq = dir + "/r.fq";
    { FILE *f = fopen(fq.c_str(), "w"); if (!f) { perror(fq.c_str()); return 1; } fputs("@r\nACGT\n+\nIIII\n", f); fclose(f); }
    const std::vector<std::string> bo = {"-i", "idx", "-f", fq, "-bo", dir + "/o.bam"}, o = {"-i", "idx", "-f", fq, "-o", dir + "/o.sam"};
    const std::map<std::string, std::string> sorted = {{"DART_DEVICE_BAM", "1"}, {"DART_SORT_BAM", "1"}}, marked = {{"DART_DEVICE_BAM", "1"}, {"DART_SORT_BAM", "1"}, {"DART_MARK_DUPLICATES", "1"}};
    auto plus = [](std::map<std::string, std::string> m, std::initializer_list<std::pair<const std::string, std::string>> more) { for (auto &kv : more) m[kv.first] = kv.second; return m; };
    // off by default, with and without the marking; the separator's default is there all the same
    { auto x = parse(bo, marked); CHECK(x->rc == RUN && x->c.mark_dups && x->c.md_umi == 0 && x->c.md_umi_sep == '_' && x->err.empty()); }
    { auto x = parse(bo, sorted); CHECK(x->rc == RUN && !x->c.mark_dups && x->c.md_umi == 0 && x->c.md_umi_sep == '_'); }
    { auto x = parse(o, {}); CHECK(x->rc == RUN && x->c.md_umi == 0); }
    // exact and edit1; the counts go where the plain marking's go
    { auto x = parse(bo, plus(marked, {{"DART_MARKDUP_UMI", "exact"}})); CHECK(x->rc == RUN && x->c.mark_dups && x->c.md_umi == 1 && x->c.md_umi_sep == '_' && x->c.md_path == dir + "/o.bam.markdup.txt" && x->err.empty() && x->out.empty()); }
    { auto x = parse(bo, plus(marked, {{"DART_MARKDUP_UMI", "edit1"}})); CHECK(x->rc == RUN && x->c.md_umi == 2 && x->c.md_umi_sep == '_'); }
    // the separator: one byte, ':' for names that carry the UMI as their last field; alone it turns nothing on
    { auto x = parse(bo, plus(marked, {{"DART_MARKDUP_UMI", "edit1"}, {"DART_MARKDUP_UMI_SEP", ":"}})); CHECK(x->rc == RUN && x->c.md_umi == 2 && x->c.md_umi_sep == ':'); }
    { auto x = parse(bo, plus(marked, {{"DART_MARKDUP_UMI_SEP", "#"}})); CHECK(x->rc == RUN && x->c.md_umi == 0 && x->c.md_umi_sep == '#'); }
    for (const char *v : {"", "__", "::"}) { auto x = parse(bo, plus(marked, {{"DART_MARKDUP_UMI", "exact"}, {"DART_MARKDUP_UMI_SEP", v}}));
      CHECK(x->rc == 1 && x->out.empty() && x->err == std::string("Error! DART_MARKDUP_UMI_SEP=") + v + ": one byte\n"); }
    // another value: the run ends, the switch is named, one line
    for (const char *v : {"", "1", "0", "EXACT", "edit2", "edit1 "}) { auto x = parse(bo, plus(marked, {{"DART_MARKDUP_UMI", v}}));
      CHECK(x->rc == 1 && x->out.empty() && x->err == std::string("Error! DART_MARKDUP_UMI=") + v + ": exact or edit1\n"); }
    // refused without DART_MARK_DUPLICATES=1, whatever else is there; the marking's own refusal comes first
    const std::string T = " needs DART_MARK_DUPLICATES=1 (and with it DART_SORT_BAM=1): DART_MARK_DUPLICATES=1 is missing\n";
    { auto x = parse(bo, plus(sorted, {{"DART_MARKDUP_UMI", "exact"}})); CHECK(x->rc == 1 && x->out.empty() && x->err == "Error! DART_MARKDUP_UMI=exact" + T); }
    { auto x = parse(bo, plus(sorted, {{"DART_MARKDUP_UMI", "edit1"}, {"DART_MARK_DUPLICATES", "0"}})); CHECK(x->rc == 1 && x->err == "Error! DART_MARKDUP_UMI=edit1" + T); }
    { auto x = parse(bo, {{"DART_MARKDUP_UMI", "edit1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_MARKDUP_UMI=edit1" + T); }
    { auto x = parse(o, {{"DART_MARKDUP_UMI", "exact"}}); CHECK(x->rc == 1 && x->err == "Error! DART_MARKDUP_UMI=exact" + T); }
    { auto x = parse(bo, {{"DART_MARKDUP_UMI", "exact"}, {"DART_MARK_DUPLICATES", "1"}}); CHECK(x->rc == 1 && x->err == "Error! DART_MARK_DUPLICATES=1 needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing\n"); }
    // behind the marking's check and in front of the allele counts'
    { auto x = parse(bo, plus(sorted, {{"DART_MARKDUP_UMI", "exact"}, {"DART_PILEUP", "1"}, {"DART_PILEUP_MIN_ALT", "0"}})); CHECK(x->rc == 1 && x->err == "Error! DART_MARKDUP_UMI=exact" + T); }
    // beside the other stages behind the sort
    { auto x = parse(bo, plus(marked, {{"DART_MARKDUP_UMI", "edit1"}, {"DART_QC", "1"}, {"DART_PILEUP", "1"}, {"DART_COVERAGE", "2"}, {"DART_BAM_INDEX", "1"}}));
      CHECK(x->rc == RUN && x->c.md_umi == 2 && x->c.qc && x->c.pileup && x->c.coverage == 2 && x->c.bam_index && x->c.md_path == dir + "/o.bam.markdup.txt"); }
    // ---- DART_UMI, DART_UMI_SKIP, DART_UMI_SEP: the inline cut inside the upload ----
    const std::map<std::string, std::string> dev_bam = {{"DART_DEVICE_FASTQ", "1"}, {"DART_DEVICE_BAM", "1"}}, dev_sam = {{"DART_DEVICE_FASTQ", "1"}, {"DART_DEVICE_SAM", "1"}};
    // off by default; the tuning switches' defaults are there all the same
    { auto x = parse(o, dev_sam); const dg_umi &u = x->c.umi_par; CHECK(x->rc == RUN && !x->c.umi && !x->c.cuts() && x->c.trim_path.empty() && u.len[0] == 0 && u.len[1] == 0 && u.skip[0] == 0 && u.skip[1] == 0 && u.sep == '_' && u.flags == 0); }
    // one and two lengths, the linker, the separator; the statistics file follows the output's name; trimming beside it
    { auto x = parse(o, plus(dev_sam, {{"DART_UMI", "8"}})); const dg_umi &u = x->c.umi_par;
      CHECK(x->rc == RUN && x->c.umi && x->c.cuts() && !x->c.trim && u.len[0] == 8 && u.len[1] == 0 && u.skip[0] == 0 && u.skip[1] == 0 && u.sep == '_' && x->c.trim_path == dir + "/o.sam.trim.txt" && x->err.empty() && x->out.empty()); }
    { auto x = parse(bo, plus(dev_bam, {{"DART_UMI", "6,4"}, {"DART_UMI_SKIP", "3,2"}, {"DART_UMI_SEP", "#"}})); const dg_umi &u = x->c.umi_par;
      CHECK(x->rc == RUN && x->c.umi && u.len[0] == 6 && u.len[1] == 4 && u.skip[0] == 3 && u.skip[1] == 2 && u.sep == '#' && x->c.trim_path == dir + "/o.bam.trim.txt"); }
    { auto x = parse(o, plus(dev_sam, {{"DART_UMI", "0,21"}, {"DART_UMI_SKIP", "5"}})); CHECK(x->rc == RUN && x->c.umi_par.len[0] == 0 && x->c.umi_par.len[1] == 21 && x->c.umi_par.skip[0] == 5 && x->c.umi_par.skip[1] == 0); }
    { auto x = parse(o, plus(dev_sam, {{"DART_UMI", "8"}, {"DART_TRIM_QUAL", "20"}})); CHECK(x->rc == RUN && x->c.umi && x->c.trim && x->c.trim_par.qual3 == 20 && x->c.trim_path == dir + "/o.sam.trim.txt"); }
    // DART_MARKDUP_UMI_SEP defaults to DART_UMI_SEP
    { auto x = parse(bo, plus(marked, {{"DART_DEVICE_FASTQ", "1"}, {"DART_UMI", "8"}, {"DART_UMI_SEP", "#"}, {"DART_MARKDUP_UMI", "exact"}})); CHECK(x->rc == RUN && x->c.umi && x->c.md_umi == 1 && x->c.md_umi_sep == '#' && x->c.umi_par.sep == '#'); }
    { auto x = parse(bo, plus(marked, {{"DART_DEVICE_FASTQ", "1"}, {"DART_UMI", "8"}, {"DART_UMI_SEP", "#"}, {"DART_MARKDUP_UMI", "exact"}, {"DART_MARKDUP_UMI_SEP", ":"}})); CHECK(x->rc == RUN && x->c.md_umi_sep == ':' && x->c.umi_par.sep == '#'); }
    // values that cannot be used: the run ends, the switch is named, one line
    const struct { const char *name, *value; } refused[] = {{"DART_UMI", ""}, {"DART_UMI", "0"}, {"DART_UMI", "0,0"}, {"DART_UMI", "11,11"}, {"DART_UMI", "22"}, {"DART_UMI", "8,"}, {"DART_UMI", "8,4,2"}, {"DART_UMI", "-8"},
                                                            {"DART_UMI", "eight"}, {"DART_UMI", "8 "}, {"DART_UMI_SKIP", "x"}, {"DART_UMI_SKIP", "1001"}, {"DART_UMI_SKIP", "3;2"}, {"DART_UMI_SEP", ""}, {"DART_UMI_SEP", "__"},
                                                            {"DART_UMI_SEP", " "}, {"DART_UMI_SEP", "\t"}, {"DART_UMI_SEP", "/"}, {"DART_UMI_SEP", "A"}, {"DART_UMI_SEP", "N"}, {"DART_UMI_SEP", "+"}, {"DART_UMI_SEP", "-"}};
    for (const auto &r : refused) {
        auto x = parse(o, plus(plus(dev_sam, {{"DART_UMI", "8"}}), {{r.name, r.value}}));
        CHECK(x->rc == 1 && x->out.empty() && x->err.rfind(std::string("Error! ") + r.name + "=" + r.value + ": ", 0) == 0 && std::count(x->err.begin(), x->err.end(), '\n') == 1);
    }
    { auto x = parse(o, plus(dev_sam, {{"DART_UMI_SKIP", "3"}})); CHECK(x->rc == 1 && x->err == "Error! DART_UMI_SKIP=3 needs DART_UMI: DART_UMI is missing\n"); }
    // the refusal: the cut needs the device parser and a device formatter; reads that still carry their UMIs are never mapped silently
    const struct { const std::vector<std::string> *args; std::map<std::string, std::string> env; const char *missing; } no[] = {
        {&o, {}, "DART_DEVICE_FASTQ=1 is missing"}, {&o, {{"DART_DEVICE_SAM", "1"}}, "DART_DEVICE_FASTQ=1 is missing"}, {&o, {{"DART_DEVICE_FASTQ", "1"}}, "DART_DEVICE_SAM=1 is missing"},
        {&bo, {{"DART_DEVICE_FASTQ", "1"}, {"DART_DEVICE_SAM", "1"}}, "DART_DEVICE_BAM=1 is missing"}, {&bo, {{"DART_DEVICE_BAM", "1"}}, "DART_DEVICE_FASTQ=1 is missing"}, {&bo, {}, "DART_DEVICE_BAM=1 is missing"},
        {&o, {{"DART_DEVICE_FASTQ", "1"}, {"DART_DEVICE_SAM", "1"}, {"DART_STREAMING", "1"}}, "DART_STREAMING is set"}};
    for (const auto &n : no) {
        auto x = parse(*n.args, plus(n.env, {{"DART_UMI", "8"}}));
        CHECK(x->rc == 1 && x->out.empty() && x->err.rfind("Error! DART_UMI needs the device parser and a device formatter", 0) == 0 && x->err.find(n.missing) != std::string::npos && std::count(x->err.begin(), x->err.end(), '\n') == 1);
        auto y = parse(*n.args, n.env); CHECK(y->rc == RUN && !y->c.umi);
    }
    // the usage text does not know the switches (its bytes are pinned by the suite): the same with and without them
    { auto a = parse({"-h"}, {}), b = parse({"-h"}, plus(marked, {{"DART_MARKDUP_UMI", "edit1"}}));
      CHECK(a->rc == 0 && b->rc == 0 && a->out == b->out && a->err.empty() && b->err.empty() && a->out.find("UMI") == std::string::npos); }
    printf("checks=%ld bad=%ld\n", n_checks, bad);
    return bad ? 1 : 0;
}
