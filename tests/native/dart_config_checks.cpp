// CPU checks of what `dart` decides before it touches the device (dart_amd/csrc/host/dart_config.h): Config::parse over a table of command lines and
// environments -- every message with its stream and exit code, every clamp at both edges, what follows from the switches -- and choose_pipelines over
// the cross product of file kind x mates x output x DART_STREAMING x device switches, against the rule as the program stated it before there was one
// function for it (parent_rule below: the line numbers are those of dart_main.cpp at commit 4913dbb).
// Test infrastructure: tests/test_dart_config_host.py builds it with g++ (once plain, once with -fsanitize=address,undefined) and runs it with a scratch
// directory as its argument.  No libdartgpu: dg_params is filled by hand.
#include "dart_config.h"
#include <map>
#include <memory>

static long bad = 0, n_checks = 0;
#define CHECK(x) do { n_checks++; if (!(x)) { bad++; printf("line %d: %s\n", __LINE__, #x); } } while (0)

static std::map<std::string, std::string> g_env;
static const char *table_lookup(const char *k) { auto it = g_env.find(k); return it == g_env.end() ? nullptr : it->second.c_str(); }

static dg_params hand_filled()
{
    dg_params p; memset(&p, 0, sizeof p);
    p.max_dup = 100; p.max_intron = 500000; p.min_intron = 5; p.max_mismatch = 0;
    return p;
}

// how Config::parse ended, and what it wrote to the two streams it was given
struct Parsed { enum Kind { Run, Exit, Error } kind = Run; int code = 0; std::string out, err; };
struct Run { Config c; Parsed r; };
// args: the words behind the program's name
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
    char *ob = nullptr, *eb = nullptr; size_t on = 0, en = 0;
    FILE *out = open_memstream(&ob, &on), *err = open_memstream(&eb, &en);
    const int rc = x->c.parse((int)argv.size() - 1, argv.data(), table_lookup, hand_filled(), out, err);
    fclose(out); fclose(err);
    x->r.kind = rc == RUN ? Parsed::Run : rc == 0 ? Parsed::Exit : Parsed::Error; x->r.code = rc == RUN ? 0 : rc;      // (anything but RUN is the exit code: 0 or 1)
    CHECK(rc == RUN || rc == 0 || rc == 1);
    x->r.out.assign(ob, on); x->r.err.assign(eb, en);
    free(ob); free(eb);
    return x;
}

static const char *USAGE_100 =
    "\nDART v1.4.6 (Hsin-Nan Lin & Wen-Lian Hsu)\n\n"
    "Usage: dart -i Index_Prefix -f <ReadFile_A1 ReadFile_B1 ...> [-f2 <ReadFile_A2 ReadFile_B2 ...>] -o|-bo Alignment_Output\n\n"
    "Options: -t INT        number of threads [4]\n"
    "         -f            files with #1 mates reads\n"
    "         -f2           files with #2 mates reads\n"
    "         -mis INT      maximal number of mismatches in an alignment\n"
    "         -max_dup INT  maximal number of repetitive fragments (between 100-10000) [100]\n"
    "         -o            alignment filename in SAM format\n"
    "         -bo           alignment filename in BAM format\n"
    "                       (DART_DEVICE_BAM=1 DART_SORT_BAM=1: coordinate-sorted on the device; DART_BAM_INDEX=1 beside them: its .bai too; DART_COVERAGE=1 or 2: its bedGraph, or one per strand; DART_MARK_DUPLICATES=1: flag 0x400 set on the device)\n"
    "         -j            splice junction output filename [junctions.tab]\n"
    "         -m            output multiple alignments [false]\n"
    "         -all_sj       detect all splice junction regardless of mapq score [false]\n"
    "         -p            paired-end reads are interlaced in the same file\n"
    "         -unique       output unique alignments\n"
    "         -max_intron   the maximal intron size [500000]\n"
    "         -min_intron   the minimal intron size [10]\n"
    "         -v            version\n"
    "\n";

static bool is(const Parsed &r, Parsed::Kind k, int code, const std::string &out, const std::string &err) { return r.kind == k && r.code == code && r.out == out && r.err == err; }

static void messages_and_exits(const std::string &fq, const std::string &dir)
{
    const std::vector<std::string> ok = {"-i", "idx", "-f", fq};
    auto with = [&](std::vector<std::string> more) { std::vector<std::string> a = ok; a.insert(a.end(), more.begin(), more.end()); return a; };
    // usage, -h, -v: stdout, exit 0
    CHECK(is(parse({}, {})->r, Parsed::Exit, 0, USAGE_100, ""));
    CHECK(is(parse({"-h"}, {})->r, Parsed::Exit, 0, USAGE_100, ""));
    CHECK(is(parse({"-h", "-x"}, {})->r, Parsed::Exit, 0, USAGE_100, ""));
    CHECK(is(parse({"-v"}, {})->r, Parsed::Exit, 0, "DART v1.4.6\n\n", ""));
    CHECK(is(parse(with({"--version", "-x"}), {})->r, Parsed::Exit, 0, "DART v1.4.6\n\n", ""));
    // an unknown parameter: the message on stderr, the usage on stdout (with -max_dup as it stands by then), exit 1
    CHECK(is(parse(with({"-x"}), {})->r, Parsed::Error, 1, USAGE_100, "Error! Unknow parameter: -x\n"));
    { std::string u = USAGE_100; u.replace(u.find("[100]"), 5, "[2000]");
      CHECK(is(parse({"-max_dup", "2000", "-what"}, {})->r, Parsed::Error, 1, u, "Error! Unknow parameter: -what\n")); }
    // no reads; mate files that do not pair up
    CHECK(is(parse({"-i", "idx"}, {})->r, Parsed::Error, 1, USAGE_100, "Error! Please specify a valid read input!\n"));
    CHECK(is(parse({"-i", "idx", "-f", "a", "b", "-f2", "c"}, {})->r, Parsed::Error, 1, "", "Error! Paired-end reads input numbers do not match!\nRead1:\n\ta\n\tb\nRead2:\n\tc\n"));
    // CheckInputFiles / CheckOutputFileName: exit 0, as the reference
    CHECK(is(parse({"-i", "idx", "-f", dir + "/nosuch.fq", "-f2", dir + "/nosuch2.fq"}, {})->r, Parsed::Exit, 0, "", "Cannot access file:[" + dir + "/nosuch.fq]\nCannot access file:[" + dir + "/nosuch2.fq]\n"));
    CHECK(is(parse(with({"-o", dir}), {})->r, Parsed::Exit, 0, "Warning: " + dir + " is a directory!\n", ""));
    CHECK(is(parse(with({"-o", "/dev/null"}), {})->r, Parsed::Exit, 0, "Warning: /dev/null is not a regular file!\n", ""));
    CHECK(is(parse(with({"-o", dir + "/new.sam"}), {})->r, Parsed::Run, 0, "", ""));
    // a missing input is reported before a switch that lacks its partner (the sequence of the checks is the program's)
    CHECK(is(parse({"-i", "idx", "-f", dir + "/nosuch.fq"}, {{"DART_SORT_BAM", "1"}})->r, Parsed::Exit, 0, "", "Cannot access file:[" + dir + "/nosuch.fq]\n"));
    // the thread-count warning: stdout, and the run goes on with 4
    { auto x = parse(with({"-t", "0"}), {}); CHECK(is(x->r, Parsed::Run, 0, "Warning! Thread number should be a positive number!\n", "") && x->c.threads == 4); }
    { auto x = parse(with({"-t", "-2"}), {}); CHECK(is(x->r, Parsed::Run, 0, "Warning! Thread number should be a positive number!\n", "") && x->c.threads == 4); }
    { auto x = parse(with({"-t", "1"}), {}); CHECK(is(x->r, Parsed::Run, 0, "", "") && x->c.threads == 1); }
    // DART_SORT_BAM: three wordings
    const std::string S = "Error! DART_SORT_BAM=1 needs -bo and DART_DEVICE_BAM=1: ";
    CHECK(is(parse(with({"-o", "o"}), {{"DART_SORT_BAM", "1"}})->r, Parsed::Error, 1, "", S + "both are missing\n"));
    CHECK(is(parse(with({"-o", "o"}), {{"DART_SORT_BAM", "1"}, {"DART_DEVICE_BAM", "0"}})->r, Parsed::Error, 1, "", S + "both are missing\n"));
    CHECK(is(parse(with({"-o", "o"}), {{"DART_SORT_BAM", "1"}, {"DART_DEVICE_BAM", "1"}})->r, Parsed::Error, 1, "", S + "-bo is missing\n"));
    CHECK(is(parse(with({"-bo", "o"}), {{"DART_SORT_BAM", "1"}})->r, Parsed::Error, 1, "", S + "DART_DEVICE_BAM=1 is missing\n"));
    CHECK(is(parse(with({"-bo", "o"}), {{"DART_SORT_BAM", "1"}, {"DART_DEVICE_BAM", "1"}})->r, Parsed::Run, 0, "", ""));
    CHECK(is(parse(with({"-bo", "o"}), {{"DART_SORT_BAM", "0"}})->r, Parsed::Run, 0, "", ""));
    // DART_BAM_INDEX, DART_COVERAGE, DART_MARK_DUPLICATES without the sort; the sort's own error comes first
    const std::string T = " needs DART_SORT_BAM=1 (and with it -bo and DART_DEVICE_BAM=1): DART_SORT_BAM=1 is missing\n";
    const std::map<std::string, std::string> dev = {{"DART_DEVICE_BAM", "1"}};
    auto plus = [](std::map<std::string, std::string> e, const char *k, const char *v) { e[k] = v; return e; };
    CHECK(is(parse(with({"-bo", "o"}), plus(dev, "DART_BAM_INDEX", "1"))->r, Parsed::Error, 1, "", "Error! DART_BAM_INDEX=1" + T));
    CHECK(is(parse(with({"-bo", "o"}), plus(dev, "DART_COVERAGE", "1"))->r, Parsed::Error, 1, "", "Error! DART_COVERAGE=1" + T));
    CHECK(is(parse(with({"-bo", "o"}), plus(dev, "DART_COVERAGE", "2"))->r, Parsed::Error, 1, "", "Error! DART_COVERAGE=2" + T));
    CHECK(is(parse(with({"-bo", "o"}), plus(dev, "DART_COVERAGE", "3"))->r, Parsed::Error, 1, "", "Error! DART_COVERAGE=3 is neither 1 (one track) nor 2 (one track per strand)\n"));
    CHECK(is(parse(with({"-bo", "o"}), plus(plus(dev, "DART_SORT_BAM", "1"), "DART_COVERAGE", "-1"))->r, Parsed::Error, 1, "", "Error! DART_COVERAGE=-1 is neither 1 (one track) nor 2 (one track per strand)\n"));
    CHECK(is(parse(with({"-bo", "o"}), plus(dev, "DART_MARK_DUPLICATES", "1"))->r, Parsed::Error, 1, "", "Error! DART_MARK_DUPLICATES=1" + T));
    CHECK(is(parse(with({"-bo", "o"}), {{"DART_BAM_INDEX", "1"}, {"DART_COVERAGE", "3"}, {"DART_MARK_DUPLICATES", "1"}})->r, Parsed::Error, 1, "", "Error! DART_BAM_INDEX=1" + T));
    CHECK(is(parse(with({"-o", "o"}), {{"DART_SORT_BAM", "1"}, {"DART_BAM_INDEX", "1"}})->r, Parsed::Error, 1, "", S + "both are missing\n"));
}

static void clamps_and_values(const std::string &fq)
{
    const std::vector<std::string> ok = {"-i", "idx", "-f", fq};
    auto with = [&](std::vector<std::string> more) { std::vector<std::string> a = ok; a.insert(a.end(), more.begin(), more.end()); return a; };
    auto cfg = [&](std::vector<std::string> more, std::map<std::string, std::string> env) { auto x = parse(with(more), env); CHECK(x->r.kind == Parsed::Run); return x; };
    // -max_dup: 100..10000
    for (auto kv : std::vector<std::pair<const char *, int>>{{"99", 100}, {"100", 100}, {"101", 101}, {"9999", 9999}, {"10000", 10000}, {"10001", 10000}, {"-7", 100}})
        CHECK(cfg({"-max_dup", kv.first}, {})->c.p.max_dup == kv.second);
    CHECK(cfg({}, {})->c.p.max_dup == 100);
    // -max_intron: at least 100000
    for (auto kv : std::vector<std::pair<const char *, int>>{{"99999", 100000}, {"100000", 100000}, {"100001", 100001}, {"0", 100000}, {"2000000", 2000000}})
        CHECK(cfg({"-max_intron", kv.first}, {})->c.p.max_intron == kv.second);
    CHECK(cfg({"-min_intron", "3", "-mis", "7"}, {})->c.p.min_intron == 3 && cfg({"-min_intron", "3", "-mis", "7"}, {})->c.p.max_mismatch == 7);
    // DART_BATCH: at least 4000 and even
    for (auto kv : std::vector<std::pair<const char *, size_t>>{{"0", 4000}, {"3999", 4000}, {"4000", 4000}, {"4001", 4000}, {"4002", 4002}, {"4003", 4002}, {"1000000", 1000000}, {"1000001", 1000000}})
        CHECK(cfg({}, {{"DART_BATCH", kv.first}})->c.batch_reads == kv.second);
    CHECK(cfg({}, {})->c.batch_reads == 500000);
    // DART_INFLIGHT: at least 1, default 2
    for (auto kv : std::vector<std::pair<const char *, int>>{{"-5", 1}, {"0", 1}, {"1", 1}, {"2", 2}, {"3", 3}, {"x", 1}})
        CHECK(cfg({}, {{"DART_INFLIGHT", kv.first}})->c.inflight == kv.second);
    CHECK(cfg({}, {})->c.inflight == 2);
    // DART_SAME_DEVICE_TIMES: 1..8, unset = 0
    for (auto kv : std::vector<std::pair<const char *, int>>{{"-1", 1}, {"0", 1}, {"1", 1}, {"2", 2}, {"8", 8}, {"9", 8}, {"100", 8}})
        CHECK(cfg({}, {{"DART_SAME_DEVICE_TIMES", kv.first}})->c.same_device_times == kv.second);
    CHECK(cfg({}, {})->c.same_device_times == 0);
    // DART_SORT_PIECE_MB: raw
    CHECK(cfg({}, {})->c.sort_piece_mb == 256.0);
    CHECK(cfg({}, {{"DART_SORT_PIECE_MB", "-1"}})->c.sort_piece_mb == -1.0);
    CHECK(cfg({}, {{"DART_SORT_PIECE_MB", "junk"}})->c.sort_piece_mb == 0.0);
    CHECK(cfg({}, {{"DART_SORT_PIECE_MB", "1e30"}})->c.sort_piece_mb == 1e30);
    // DART_GPUS raw (its clamp needs the device count); the others
    { auto x = cfg({}, {{"DART_GPUS", "-3"}}); CHECK(x->c.has_gpus && x->c.gpus == -3); CHECK(!cfg({}, {})->c.has_gpus); }
    { auto x = cfg({}, {{"DART_WRITE_THREADS", "0"}, {"DART_FMT_THREADS", "0"}, {"DART_WRITE", "mmap"}, {"DART_PINNED", "1"}});
      CHECK(x->c.write_threads == 1 && x->c.fmt_threads == 1 && x->c.write_mmap && x->c.pinned); }
    { auto x = cfg({}, {{"DART_WRITE", "pwrite"}, {"DART_PINNED", "0"}}); CHECK(x->c.write_threads == 1 && x->c.fmt_threads == 0 && !x->c.write_mmap && !x->c.pinned); }
    { auto x = cfg({}, {{"DART_GZ_WHOLE_MAX_GB", "0.5"}}); CHECK(x->c.gz_whole_max == (size_t)1 << 29); CHECK(cfg({}, {})->c.gz_whole_max == (size_t)8 << 30); CHECK(cfg({}, {{"DART_GZ_WHOLE_MAX_GB", "0"}})->c.gz_whole_max == 0); }
    // set to anything, "0" included: DART_STREAMING, DART_GZ_STREAM, DART_TIMING
    { auto x = cfg({}, {{"DART_STREAMING", "0"}, {"DART_GZ_STREAM", ""}, {"DART_TIMING", "0"}}); CHECK(x->c.streaming && x->c.gz_stream && x->c.timing); }
    { auto x = cfg({}, {}); CHECK(!x->c.streaming && !x->c.gz_stream && !x->c.timing && !x->c.sync_aids && !x->c.has_expected_reads && !x->c.device_sj); }
    { auto x = cfg({}, {{"DART_EXPECTED_READS", "12345"}, {"DART_SYNC_AIDS", "1"}, {"DART_DEVICE_SJ", "1"}}); CHECK(x->c.has_expected_reads && x->c.expected_reads == 12345 && x->c.sync_aids && x->c.device_sj); }
    { auto x = cfg({}, {{"DART_COVERAGE_EXCLUDE", "0x4"}, {"DART_COVERAGE_MIN_MAPQ", "010"}}); CHECK(x->c.cov_exclude == 4 && x->c.cov_min_mapq == 8); CHECK(cfg({}, {})->c.cov_exclude == 0x704 && cfg({}, {})->c.cov_min_mapq == 0); }
    // -o after -bo and -bo after -o: the last one wins, file name and format
    { auto x = cfg({"-bo", "a.bam", "-o", "b.sam"}, {}); CHECK(!x->c.bam && std::string(x->c.out) == "b.sam" && !x->c.bam_streams && std::string(x->c.bam_host_note) == ""); }
    { auto x = cfg({"-o", "b.sam", "-bo", "a.bam"}, {}); CHECK(x->c.bam && std::string(x->c.out) == "a.bam" && x->c.bam_streams && std::string(x->c.bam_host_note) == ", bam=host"); }
    CHECK(std::string(cfg({}, {})->c.out) == "output.sam" && std::string(cfg({}, {})->c.sj) == "junctions.tab");
    CHECK(std::string(cfg({"-j", std::string(300, 'j')}, {})->c.sj) == std::string(255, 'j'));
    // paired: -p, or as many -f2 files as -f files
    CHECK(cfg({}, {})->c.p.paired == 0 && cfg({"-p"}, {})->c.p.paired == 1 && cfg({"-f2", fq}, {})->c.p.paired == 1 && cfg({"-f2", fq}, {})->c.two_files() && !cfg({"-p"}, {})->c.two_files());
    CHECK(cfg({"-m", "-all_sj", "-unique", "-silent"}, {})->c.p.multi_hit == 1 && cfg({"-m", "-all_sj"}, {})->c.p.all_sj == 1 && cfg({"-unique", "-silent"}, {})->c.unique && cfg({"-unique", "-silent"}, {})->c.silent);
    // DART_DEVICE_BAM counts with -bo only; DART_BGZF_DYNAMIC counts beside it only; the `bam=` note
    { auto x = cfg({"-o", "o"}, {{"DART_DEVICE_BAM", "1"}, {"DART_BGZF_DYNAMIC", "1"}}); CHECK(!x->c.device_bam && !x->c.bgzf_dynamic && !x->c.bam_streams && std::string(x->c.bam_dev_note) == ""); }
    { auto x = cfg({"-bo", "o"}, {{"DART_BGZF_DYNAMIC", "1"}}); CHECK(!x->c.device_bam && !x->c.bgzf_dynamic && x->c.bam_streams && std::string(x->c.bam_dev_note) == ""); }
    { auto x = cfg({"-bo", "o"}, {{"DART_DEVICE_BAM", "1"}}); CHECK(x->c.device_bam && !x->c.bgzf_dynamic && !x->c.bam_streams && std::string(x->c.bam_dev_note) == ", bam=device"); }
    { auto x = cfg({"-bo", "o"}, {{"DART_DEVICE_BAM", "1"}, {"DART_BGZF_DYNAMIC", "1"}}); CHECK(x->c.device_bam && x->c.bgzf_dynamic && std::string(x->c.bam_dev_note) == ", bam=device+dyn"); }
    { auto x = cfg({"-bo", "o"}, {{"DART_DEVICE_BAM", "1"}, {"DART_SORT_BAM", "1"}}); CHECK(x->c.sort_bam && std::string(x->c.bam_dev_note) == ", bam=device+sorted"); }
    { auto x = cfg({"-bo", "o"}, {{"DART_DEVICE_BAM", "1"}, {"DART_SORT_BAM", "1"}, {"DART_BGZF_DYNAMIC", "1"}}); CHECK(std::string(x->c.bam_dev_note) == ", bam=device+sorted+dyn"); }
    // DART_DEVICE_SAM: -bo switches it off; DART_DEVICE_FASTQ: -bo without DART_DEVICE_BAM switches it off
    const std::map<std::string, std::string> dsf = {{"DART_DEVICE_SAM", "1"}, {"DART_DEVICE_FASTQ", "1"}};
    { auto x = cfg({"-o", "o"}, dsf); CHECK(x->c.device_sam && x->c.device_fastq); }
    { auto x = cfg({"-bo", "o"}, dsf); CHECK(!x->c.device_sam && !x->c.device_fastq); }
    { auto x = cfg({"-bo", "o"}, {{"DART_DEVICE_SAM", "1"}, {"DART_DEVICE_FASTQ", "1"}, {"DART_DEVICE_BAM", "1"}}); CHECK(!x->c.device_sam && x->c.device_fastq); }
    // the sorted file's companions: paths and strand flags
    { auto x = cfg({"-bo", "d/o.bam"}, {{"DART_DEVICE_BAM", "1"}, {"DART_SORT_BAM", "1"}, {"DART_BAM_INDEX", "1"}, {"DART_COVERAGE", "2"}, {"DART_MARK_DUPLICATES", "1"}, {"DART_GENE_COUNTS", "a.gtf"}});
      CHECK(x->c.bai_path == "d/o.bam.bai" && x->c.md_path == "d/o.bam.markdup.txt" && x->c.genes_path == "d/o.bam.genes.tab" && x->c.coverage == 2 && x->c.cov_tracks.size() == 2);
      CHECK(x->c.cov_tracks.size() == 2 && x->c.cov_tracks[0] == std::make_pair(std::string("d/o.bam.plus.bedgraph"), (uint32_t)DG_COV_STRAND_PLUS) && x->c.cov_tracks[1] == std::make_pair(std::string("d/o.bam.minus.bedgraph"), (uint32_t)DG_COV_STRAND_MINUS)); }
    { auto x = cfg({"-bo", "o"}, {{"DART_DEVICE_BAM", "1"}, {"DART_SORT_BAM", "1"}, {"DART_COVERAGE", "1"}});
      CHECK(x->c.bai_path.empty() && x->c.md_path.empty() && x->c.genes_path.empty() && x->c.cov_tracks.size() == 1 && x->c.cov_tracks[0] == std::make_pair(std::string("o.bedgraph"), 0u)); }
    // DART_GENE_COUNTS empty = unset; its companions
    { auto x = cfg({}, {{"DART_GENE_COUNTS", ""}, {"DART_GENE_FEATURE", ""}}); CHECK(x->c.gene_gtf == nullptr && x->c.genes_path.empty() && std::string(x->c.gene_feature) == "exon" && x->c.gene_min_mapq == 4); }
    { auto x = cfg({"-o", "o.sam"}, {{"DART_GENE_COUNTS", "g.gtf"}, {"DART_GENE_FEATURE", "CDS"}, {"DART_GENE_MIN_MAPQ", "0"}}); CHECK(std::string(x->c.gene_gtf) == "g.gtf" && x->c.genes_path == "o.sam.genes.tab" && std::string(x->c.gene_feature) == "CDS" && x->c.gene_min_mapq == 0); }
    // DART_DEVICE_GZ: all four preconditions, then each one missing
    const std::map<std::string, std::string> gz = {{"DART_DEVICE_GZ", "1"}, {"DART_DEVICE_FASTQ", "1"}, {"DART_DEVICE_SAM", "1"}};
    auto minus = [](std::map<std::string, std::string> e, const char *k) { e.erase(k); return e; };
    auto plus = [](std::map<std::string, std::string> e, const char *k, const char *v) { e[k] = v; return e; };
    CHECK(cfg({"-o", "o"}, gz)->c.device_gz);
    CHECK(cfg({"-bo", "o"}, plus(gz, "DART_DEVICE_BAM", "1"))->c.device_gz);
    CHECK(!cfg({"-o", "o"}, minus(gz, "DART_DEVICE_GZ"))->c.device_gz);
    CHECK(!cfg({"-o", "o"}, minus(gz, "DART_DEVICE_FASTQ"))->c.device_gz);            // 1: DART_DEVICE_FASTQ
    CHECK(!cfg({"-o", "o"}, minus(gz, "DART_DEVICE_SAM"))->c.device_gz);              // 2: a device formatter
    CHECK(!cfg({"-bo", "o"}, gz)->c.device_gz);                                       // 3: no -bo that streams (and -bo has switched DART_DEVICE_SAM off)
    CHECK(!cfg({"-o", "o"}, plus(gz, "DART_STREAMING", "1"))->c.device_gz);           // 4: no DART_STREAMING
    CHECK(!cfg({"-bo", "o"}, plus(plus(gz, "DART_DEVICE_BAM", "1"), "DART_STREAMING", "0"))->c.device_gz);
}

// ---- the pipeline choice ----
// The rule as dart_main.cpp stated it at commit 4913dbb, twice: the head start for library 0 (lines 644-656) and the library loop (823-872 with
// open_lib, 674-695); gz_device_candidate is 637-643, gz_whole_candidate 612-622.  What the program did with a library, in the terms of both statements:
struct ParentSays {
    bool try_gz_device, try_gz_whole, fast_host;      // the loop: plan.make is called; the files are inflated whole (or were, at the head); the parallel pipeline else the streaming one
    bool pool, pre_plain, pre_gz;                     // the head start, if this is library 0: the slot pool starts; the plain files are indexed; the .gz files are inflated
};
static ParentSays parent_rule(const Config &c, const FileProbe &a, const FileProbe *b, bool libdeflate)
{
    const bool streaming_env = c.streaming;
    auto gz_device_candidate = [&]() {                                           // 637-643
        if (!c.device_gz) return false;                                          // 638
        if (!a.gz || !a.bgzf || !a.fastq) return false;                          // 641
        if (b && (!b->gz || !b->bgzf || !b->fastq)) return false;                // 641
        return true;
    };
    auto gz_whole_candidate = [&]() {                                            // 612-622
        if (c.bam_streams || streaming_env || c.gz_stream || !libdeflate || c.gz_whole_max == 0) return false;      // 613
        for (const FileProbe *f : {&a, b}) {                                     // 617-620
            if (!f) continue;
            if (!f->gz || !f->fastq || f->size < 0 || (size_t)f->size > c.gz_whole_max / 2) return false;           // 619
        }
        return true;
    };
    ParentSays s = {};
    bool fast_first = false, gz_first = false, gz_device_first = false;
    if (gz_device_candidate()) fast_first = gz_device_first = true;              // 648
    else if (!c.bam_streams && !streaming_env && !a.gz && a.fastq) {             // 649
        fast_first = true;                                                       // 650
        if (!b || !b->gz) s.pre_plain = true;                                    // 651
    } else if (gz_whole_candidate()) { fast_first = gz_first = true; s.pre_gz = true; }      // 652-654
    s.pool = fast_first;                                                         // 668
    s.try_gz_device = gz_device_candidate();                                     // 823
    s.try_gz_whole = gz_first || (gz_device_first && gz_whole_candidate());      // 842-843 for library 0 (a later library: gz_whole_candidate alone, checked below)
    s.fast_host = a.fastq && !a.gz && !c.bam_streams && !streaming_env && (!b || !b->gz);      // 692
    return s;
}

enum Pipeline { PIPE_GZ_DEVICE, PIPE_GZ_WHOLE, PIPE_PLAIN, PIPE_STREAMING };
static std::vector<Pipeline> order_of(const PipelineChoice &ch)      // the candidates in the order they are tried (dart_config.h states it)
{
    std::vector<Pipeline> o;
    if (ch.gz_device) o.push_back(PIPE_GZ_DEVICE);
    if (ch.gz_whole) o.push_back(PIPE_GZ_WHOLE);
    o.push_back(ch.plain ? PIPE_PLAIN : PIPE_STREAMING);
    return o;
}

static FileProbe kind(int k, long long size = 1000)      // 0 plain FASTQ, 1 .gz FASTQ, 2 BGZF FASTQ, 3 plain FASTA
{
    FileProbe f; f.size = size;
    f.gz = k == 1 || k == 2; f.bgzf = k == 2; f.fastq = k != 3;
    return f;
}

static void pipeline_choice(const std::string &fq)
{
    const char *outs[3][2] = {{"-o", nullptr}, {"-bo", nullptr}, {"-bo", "DART_DEVICE_BAM"}};
    long cases = 0;
    for (int k1 = 0; k1 < 4; k1++) for (int mates = 0; mates < 4; mates++) for (int o = 0; o < 3; o++) for (int streaming = 0; streaming < 2; streaming++) for (int dev = 0; dev < 2; dev++)
        for (int no_ld = 0; no_ld < 2; no_ld++) for (int gzs = 0; gzs < 2; gzs++) {
            std::map<std::string, std::string> env;
            if (outs[o][1]) env[outs[o][1]] = "1";
            if (streaming) env["DART_STREAMING"] = "1";
            if (dev) { env["DART_DEVICE_GZ"] = "1"; env["DART_DEVICE_FASTQ"] = "1"; env["DART_DEVICE_SAM"] = "1"; }
            if (gzs) env["DART_GZ_STREAM"] = "1";
            auto x = parse({"-i", "idx", "-f", fq, outs[o][0], "out"}, env);
            CHECK(x->r.kind == Parsed::Run);
            const Config &c = x->c;
            // mates: 0 one file; 1 two files, mate 2 plain FASTQ; 2 two files, mate 2 compressed as mate 1 is (gz for a plain mate 1); 3 mixed: the other compression, or FASTA beside FASTQ
            const FileProbe m1 = kind(k1);
            FileProbe m2 = mates == 1 ? kind(0) : mates == 2 ? kind(k1 == 2 ? 2 : 1) : kind(k1 == 0 ? 3 : k1 == 3 ? 1 : k1 == 1 ? 2 : 0);
            const FileProbe *p2 = mates ? &m2 : nullptr;
            const PipelineChoice ch = choose_pipelines(c, m1, p2, !no_ld);      // (no_ld: a system without libdeflate)
            const ParentSays want = parent_rule(c, m1, p2, !no_ld);
            cases++;
            const std::vector<Pipeline> order = order_of(ch);
            CHECK(ch.gz_device == want.try_gz_device);
            CHECK(ch.gz_whole == want.try_gz_whole);
            CHECK(ch.plain == want.fast_host);
            // the head start for library 0: the pool; what the first candidate begins
            CHECK(ch.head_pool == want.pool);
            CHECK((order[0] == PIPE_PLAIN) == want.pre_plain);
            CHECK((order[0] == PIPE_GZ_WHOLE) == want.pre_gz);
        }
    CHECK(cases == 4 * 4 * 3 * 2 * 2 * 2 * 2);
    // a later library tries whole-file inflation whenever gz_whole_candidate holds (843: lib > 0): the same list serves, since for library 0 the two agree (above)
    // hand-worked cases, one per outcome and per oddity
    auto choice = [&](std::vector<std::string> out, std::map<std::string, std::string> env, FileProbe a, const FileProbe *b, bool ld = true) {
        out.insert(out.begin(), {"-i", "idx", "-f", fq}); auto x = parse(out, env); CHECK(x->r.kind == Parsed::Run); return choose_pipelines(x->c, a, b, ld); };
    auto is_list = [](const PipelineChoice &ch, std::vector<Pipeline> want, bool pool) { return order_of(ch) == want && ch.head_pool == pool; };
    const std::map<std::string, std::string> dev = {{"DART_DEVICE_GZ", "1"}, {"DART_DEVICE_FASTQ", "1"}, {"DART_DEVICE_SAM", "1"}};
    const FileProbe plain = kind(0), gz = kind(1), bgzf = kind(2), fasta = kind(3);
    CHECK(is_list(choice({"-o", "o"}, {}, plain, nullptr), {PIPE_PLAIN}, true));                                  // 649-651, 692
    CHECK(is_list(choice({"-o", "o"}, {}, plain, &plain), {PIPE_PLAIN}, true));
    CHECK(is_list(choice({"-o", "o"}, {}, plain, &gz), {PIPE_STREAMING}, true));                                  // 650 against 692: the pool starts, the library streams
    CHECK(is_list(choice({"-o", "o"}, {}, plain, &fasta), {PIPE_PLAIN}, true));                                   // 692 does not look at mate 2's format: open_lib refuses the library (685)
    CHECK(is_list(choice({"-o", "o"}, {}, fasta, nullptr), {PIPE_STREAMING}, false));                             // 649: not FASTQ
    CHECK(is_list(choice({"-o", "o"}, {}, gz, &gz), {PIPE_GZ_WHOLE, PIPE_STREAMING}, true));                      // 652, 842
    CHECK(is_list(choice({"-o", "o"}, {}, gz, &plain), {PIPE_STREAMING}, false));                                 // 619: every file must be .gz
    CHECK(is_list(choice({"-o", "o"}, {}, gz, &gz, false), {PIPE_STREAMING}, false));                             // 613: no libdeflate
    CHECK(is_list(choice({"-o", "o"}, {{"DART_GZ_STREAM", "1"}}, gz, nullptr), {PIPE_STREAMING}, false));         // 613
    CHECK(is_list(choice({"-o", "o"}, {{"DART_GZ_WHOLE_MAX_GB", "0"}}, gz, nullptr), {PIPE_STREAMING}, false));   // 613
    { const FileProbe big = kind(1, ((long long)4 << 30) + 1), fits = kind(1, (long long)4 << 30), unknown = kind(1, -1);      // 619: half of the 8 GB per file
      CHECK(is_list(choice({"-o", "o"}, {}, big, nullptr), {PIPE_STREAMING}, false));
      CHECK(is_list(choice({"-o", "o"}, {}, fits, nullptr), {PIPE_GZ_WHOLE, PIPE_STREAMING}, true));
      CHECK(is_list(choice({"-o", "o"}, {}, unknown, nullptr), {PIPE_STREAMING}, false)); }
    CHECK(is_list(choice({"-o", "o"}, dev, bgzf, &bgzf), {PIPE_GZ_DEVICE, PIPE_GZ_WHOLE, PIPE_STREAMING}, true)); // 648, 823, 843 (gz_device_first)
    CHECK(is_list(choice({"-o", "o"}, dev, bgzf, &gz), {PIPE_GZ_WHOLE, PIPE_STREAMING}, true));                   // 641: every file must begin with a BGZF block
    CHECK(is_list(choice({"-o", "o"}, dev, bgzf, &bgzf, false), {PIPE_GZ_DEVICE, PIPE_STREAMING}, true));
    CHECK(is_list(choice({"-o", "o"}, {}, bgzf, &bgzf), {PIPE_GZ_WHOLE, PIPE_STREAMING}, true));                  // 638: without the switch BGZF is a .gz file like any other
    CHECK(is_list(choice({"-bo", "o"}, {}, plain, nullptr), {PIPE_STREAMING}, false));                            // 560: -bo without DART_DEVICE_BAM streams
    CHECK(is_list(choice({"-bo", "o"}, {}, gz, nullptr), {PIPE_STREAMING}, false));
    CHECK(is_list(choice({"-bo", "o"}, {{"DART_DEVICE_BAM", "1"}}, plain, &plain), {PIPE_PLAIN}, true));
    CHECK(is_list(choice({"-bo", "o"}, {{"DART_DEVICE_BAM", "1"}}, gz, nullptr), {PIPE_GZ_WHOLE, PIPE_STREAMING}, true));
    CHECK(is_list(choice({"-o", "o"}, {{"DART_STREAMING", "0"}}, plain, nullptr), {PIPE_STREAMING}, false));      // 649: the variable set to anything
    CHECK(is_list(choice({"-o", "o"}, {{"DART_STREAMING", "1"}}, gz, &gz), {PIPE_STREAMING}, false));
}

// probe() on files of each kind
static void probes(const std::string &dir)
{
    auto put = [&](const char *name, const std::string &bytes) { const std::string p = dir + "/" + name; FILE *f = fopen(p.c_str(), "wb"); fwrite(bytes.data(), 1, bytes.size(), f); fclose(f); return p; };
    const std::string rec = "@r0/1\nACGT\n+\nIIII\n";
    auto gz_of = [&](const char *name, const std::string &text) { const std::string p = dir + "/" + name; gzFile g = gzopen(p.c_str(), "wb"); gzwrite(g, text.data(), (unsigned)text.size()); gzclose(g); return p; };
    { const FileProbe f = probe(put("a.fq", rec)); CHECK(!f.gz && f.fastq && !f.bgzf && f.size == (long long)rec.size()); }
    { const FileProbe f = probe(put("a.fa", ">r0/1\nACGT\n")); CHECK(!f.gz && !f.fastq && !f.bgzf && f.size == 11); }
    { const FileProbe f = probe(gz_of("b.fq.gz", rec)); CHECK(f.gz && f.fastq && !f.bgzf && f.size > 0); }
    { const FileProbe f = probe(gz_of("b.fa.gz", ">r0\nAC\n")); CHECK(f.gz && !f.fastq && !f.bgzf); }
    { const FileProbe f = probe(gz_of("c.fq", rec)); CHECK(!f.gz && f.fastq && !f.bgzf); }    // compressed, but not by name: the readers treat it as plain
    { const FileProbe f = probe(dir + "/nosuch.gz"); CHECK(f.gz && !f.fastq && !f.bgzf && f.size == -1); }
    // a BGZF block: gzip header with FEXTRA and the BC subfield, a stored deflate block
    auto bgzf_of = [&](const std::string &text, bool bc_first) {
        std::string d; d += (char)1; d += (char)(text.size() & 255); d += (char)(text.size() >> 8); d += (char)(~text.size() & 255); d += (char)((~text.size() >> 8) & 255); d += text;
        const std::string other = std::string("XY\x03\x00", 4) + "abc";
        std::string extra = bc_first ? std::string("BC\x02\x00\x00\x00", 6) + other : other + std::string("BC\x02\x00\x00\x00", 6);
        const size_t bsize = 12 + extra.size() + d.size() + 8 - 1;
        extra[bc_first ? 4 : other.size() + 4] = (char)(bsize & 255); extra[bc_first ? 5 : other.size() + 5] = (char)(bsize >> 8);
        std::string m("\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff", 10); m += (char)(extra.size() & 255); m += (char)(extra.size() >> 8); m += extra; m += d;
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)text.data(), (uInt)text.size()), isize = (uint32_t)text.size();
        for (uint32_t v : {crc, isize}) for (int k = 0; k < 4; k++) m += (char)(v >> (8 * k) & 255);
        return m;
    };
    { const FileProbe f = probe(put("d.fq.gz", bgzf_of(rec, true))); CHECK(f.gz && f.fastq && f.bgzf); }
    { const FileProbe f = probe(put("e.fq.gz", bgzf_of(rec, false))); CHECK(f.gz && f.fastq && f.bgzf); }
    { const FileProbe f = probe(put("f.fq", bgzf_of(rec, true))); CHECK(!f.gz && f.fastq && !f.bgzf); }       // BGZF, but not .gz by name: never the device's
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: %s scratch_dir\n", argv[0]); return 2; }
    const std::string dir = argv[1], fq = dir + "/reads.fq";
    { FILE *f = fopen(fq.c_str(), "wb"); fputs("@r0/1\nACGT\n+\nIIII\n", f); fclose(f); }
    messages_and_exits(fq, dir);
    clamps_and_values(fq);
    pipeline_choice(fq);
    probes(dir);
    printf("checks %ld  bad=%ld\n", n_checks, bad);
    return bad ? 1 : 0;
}
