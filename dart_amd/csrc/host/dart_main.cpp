// dart_amd/csrc/host/dart_main.cpp -- `dart`: DART's command line over libdartgpu (C ABI only).
//
// Host-side mirror of the reference's driver for the north-star path:
//   flags + defaults + messages + exit codes   main.cpp:96-239
//   index files                                 bwt_index.cpp:15-159,229-251
//   FASTA/FASTQ(.gz) readers, chunking, mate-2 reverse complement   GetData.cpp:44-247
//   SAM header/records, statistics, junctions.tab   Mapping.cpp:208-369,567-577,683-716,741-751,806-822
// Everything between "chunk read" and "records formatted" (Mapping.cpp:598-639) is dg_map_batch.
// -bo: BAM through bam_writer.h (the reference hands its SAM lines to htslib).  `dart index ref.fa prefix`: index_cmd.h over libdartindex.so.
// Out of scope and refused with a message: `update`.
//
// Batches are much larger than the reference's 4000-read chunks (a GPU launch needs >= 10^5 reads);
// output order is input order, which equals the reference at -t 1.  -t keeps its
// meaning for the host side: threads that format SAM text.  DART_GPUS=n spreads batches over n
// devices, DART_INFLIGHT=k (default 1) contexts per device (dg_clone); parsing (one thread per mate file),
// mapping + formatting (one worker per context) and the ordered writer run as a pipeline; DART_BATCH=reads sets the batch size; DART_TIMING=1 prints the stage times.
//
// The flags and every DART_* variable are read once, into Config (dart_config.h, which also says which pipeline a library takes: choose_pipelines); what lives
// across libraries is one Job (fast_fastq.h) that main owns and hands to both pipelines; main itself is the list of stages below.
#include "dartgpu.h"
#include <zlib.h>
#include <sys/stat.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "dart_config.h"
#include "fast_fastq.h"
#include "gtf.h"
#include "bam_writer.h"
#include "index_cmd.h"

// ---------------------------------------------------------------------------------------------
// index files
// ---------------------------------------------------------------------------------------------
// What the host keeps of the index: the chromosome table of PREFIX.ann (names for the SAM header and the records, offsets for
// junctions.tab).  The three big files (.bwt, .sa, .pac) go from the page cache to HBM inside dg_init_files; the host never holds them.
struct HostIndex {
    std::vector<std::string> names; std::vector<int64_t> off, len;
    int64_t l_pac = 0;
};

static bool file_exists(const std::string &fn) { FILE *f = fopen(fn.c_str(), "r"); if (!f) return false; fclose(f); return true; }

static bool load_ann(const std::string &prefix, HostIndex &ix)      // bwt_index.cpp:37-89 (bns_restore_core)
{
    FILE *f = fopen((prefix + ".ann").c_str(), "r");
    if (!f) return false;
    long long xx; int n; unsigned seed;
    if (fscanf(f, "%lld%d%u", &xx, &n, &seed) != 3) { fclose(f); return false; }
    ix.l_pac = xx;
    int64_t total = 0;
    for (int i = 0; i < n; i++) {
        unsigned gi; char name[1024]; int c, l, na;
        if (fscanf(f, "%u%1023s", &gi, name) != 2) { fclose(f); return false; }
        while ((c = fgetc(f)) != '\n' && c != EOF) {}
        if (fscanf(f, "%lld%d%d", &xx, &l, &na) != 3) { fclose(f); return false; }
        ix.names.push_back(name); ix.off.push_back(total); ix.len.push_back(l); total += l;
    }
    fclose(f);
    return n > 0;
}

// ---------------------------------------------------------------------------------------------
// readers
// ---------------------------------------------------------------------------------------------
struct Entry { std::string header, seq; int rlen = 0; };

struct Source {
    FILE *fp = nullptr; gzFile gz = nullptr; bool fastq = true;
    char *buf = nullptr; size_t cap = 0;
    // block reader for plain FASTQ: lines are handed out as (pointer into the block, length incl. newline), like getline
    // without the copy and the per-call locking; a line stays valid until the next call
    char *blk = nullptr; size_t blk_cap = 0, blk_beg = 0, blk_end = 0; bool blk_eof = false;
    void refill() {                                  // what is left moves to the front, then the next bytes of the stream behind it
        if (!blk) { blk_cap = (size_t)8 << 20; blk = (char *)malloc(blk_cap + 1); }
        if (blk_beg > 0) { memmove(blk, blk + blk_beg, blk_end - blk_beg); blk_end -= blk_beg; blk_beg = 0; }
        if (blk_end == blk_cap) { blk_cap *= 2; blk = (char *)realloc(blk, blk_cap + 1); }
        const size_t got = fill(blk_cap - blk_end);
        if (got == 0) blk_eof = true;
        blk_end += got;
    }
    ssize_t block_line(char **line) {
        while (true) {
            char *nl = blk_end > blk_beg ? (char *)memchr(blk + blk_beg, '\n', blk_end - blk_beg) : nullptr;
            if (nl) { *line = blk + blk_beg; const ssize_t len = nl - (blk + blk_beg) + 1; blk_beg += (size_t)len; return len; }
            if (blk_eof) {
                if (blk_end == blk_beg) return -1;
                *line = blk + blk_beg; const ssize_t len = (ssize_t)(blk_end - blk_beg); blk_beg = blk_end; return len;   // last line without newline
            }
            refill();
        }
    }
    // gz: a thread of its own inflates 2 MB pieces ahead of the parser (zlib is the slower of the two: the parser then never waits for it to start)
    struct Inflater {
        std::thread th; std::mutex mu; std::condition_variable cv;
        std::deque<std::vector<char>> q; bool done = false, stop = false; std::vector<char> cur; size_t cur_pos = 0;
        void start(gzFile g) {
            th = std::thread([this, g]() {
                while (true) {
                    std::vector<char> b((size_t)2 << 20);
                    const int got = gzread(g, b.data(), (unsigned)b.size());
                    std::unique_lock<std::mutex> lk(mu);
                    if (got <= 0) { done = true; cv.notify_all(); return; }
                    b.resize((size_t)got);
                    cv.wait(lk, [this]() { return q.size() < 8 || stop; });
                    if (stop) return;
                    q.push_back(std::move(b));
                    cv.notify_all();
                }
            });
        }
        size_t read(char *dst, size_t room) {
            if (cur_pos == cur.size()) {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [this]() { return !q.empty() || done; });
                if (q.empty()) return 0;
                cur = std::move(q.front()); q.pop_front(); cur_pos = 0;
                cv.notify_all();
            }
            const size_t n = std::min(room, cur.size() - cur_pos);
            memcpy(dst, cur.data() + cur_pos, n); cur_pos += n;
            return n;
        }
        ~Inflater() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); if (th.joinable()) th.join(); }
    };
    std::unique_ptr<Inflater> inf;
    size_t fill(size_t room) {                       // the next bytes of the (inflated) stream behind blk_end
        if (!gz) return fread(blk + blk_end, 1, room, fp);
        if (!inf) { inf.reset(new Inflater()); inf->start(gz); }
        return inf->read(blk + blk_end, room);
    }
    // gzgets(file, buffer, 1024) as a view into the block (GetData.cpp:181-210 reads every line that way): up to 1023 bytes, ending behind
    // the first newline among them; 0 = end of the stream.  (zlib inflates in large blocks here instead of once per line.)
    size_t gets_view(char **line) {
        while (true) {
            const size_t avail = blk_end - blk_beg, want = std::min<size_t>(avail, 1023);
            char *nl = want ? (char *)memchr(blk + blk_beg, '\n', want) : nullptr;
            if (nl || want == 1023 || (blk_eof && avail)) {
                *line = blk + blk_beg;
                const size_t len = nl ? (size_t)(nl - (blk + blk_beg)) + 1 : want;
                blk_beg += len;
                return len;
            }
            if (blk_eof) return 0;
            refill();
        }
    }
    ~Source() { free(buf); free(blk); }
    // GetNextEntry, GetData.cpp:77-132, its FASTA branch (plain FASTQ goes through block_line, .gz through gets_view)
    Entry next_fasta() {
        Entry e; ssize_t len;
        if ((len = getline(&buf, &cap, fp)) != -1) {
            int p1 = hdr_beg(buf, (int)len), p2 = hdr_end(buf, (int)len);
            if (p2 > p1) e.header.assign(buf + p1, buf + p2);
            while ((len = getline(&buf, &cap, fp)) != -1) {
                if (buf[0] == '>') { fseek(fp, 0 - (long)len, SEEK_CUR); break; }
                buf[len - 1] = 0; e.seq += buf;
            }
            e.rlen = (int)e.seq.size();
        }
        return e;
    }
};

// A run of reads in flat buffers (no per-read allocation: with one std::string per field the allocator, not the
// parsing, was the cost): read k = header [hoff[k],hoff[k+1]), bases [soff[k],soff[k+1]), qualities [qoff[k],qoff[k+1]).
struct Reads {
    std::string hdr, seq, qual;
    std::vector<uint32_t> hoff{0}, soff{0}, qoff{0};
    size_t size() const { return soff.size() - 1; }
    int rlen(size_t k) const { return (int)(soff[k + 1] - soff[k]); }
    void add(const char *h, size_t hl, const char *s, size_t sl, bool rc) {      // a read without qualities (FASTA)
        hdr.append(h, hl); hoff.push_back((uint32_t)hdr.size());
        if (rc) { const size_t o = seq.size(); seq.resize(o + sl); for (size_t i = 0; i < sl; i++) seq[o + i] = comp_base_f(s[sl - 1 - i]); }
        else seq.append(s, sl);
        soff.push_back((uint32_t)seq.size());
        qoff.push_back((uint32_t)qual.size());
    }
    void add_from(const Reads &r, size_t k) {             // copy read k of r
        hdr.append(r.hdr, r.hoff[k], r.hoff[k + 1] - r.hoff[k]); hoff.push_back((uint32_t)hdr.size());
        seq.append(r.seq, r.soff[k], r.soff[k + 1] - r.soff[k]); soff.push_back((uint32_t)seq.size());
        qual.append(r.qual, r.qoff[k], r.qoff[k + 1] - r.qoff[k]); qoff.push_back((uint32_t)qual.size());
    }
};

// one read from a Source appended to R (mate 2 of a pair: reverse-complemented, qualities reversed, GetData.cpp:160-166);
// false = end of the stream (an entry of length 0, as in the reference).  Plain FASTQ is parsed straight into the flat
// buffers; FASTA and gz go through the Entry readers above.
// gzGetNextEntry, GetData.cpp:181-210, parsed straight into the flat buffers: every line is a gzgets of at most 1023 bytes; a header line
// must start with '@' or '>' and name something; the sequence is the next line without its last byte; FASTQ: two more lines, the second
// holds the qualities (cut to the read length).  FASTA through this reader has ONE sequence line per record, as in the reference.
static bool read_into_gz(Source &s, Reads &R, bool rc)
{
    char *ln; size_t len = s.gets_view(&ln);
    if (len == 0) return false;
    len = strnlen(ln, len);                               // (the reference measures its buffer with strlen)
    const int p1 = hdr_beg(ln, (int)len), p2 = hdr_end(ln, (int)len);
    if (!(p2 - p1 > 0 && (ln[0] == '@' || ln[0] == '>'))) return false;      // an entry of length 0 ends the stream
    const size_t h0 = R.hdr.size(), s0 = R.seq.size();
    R.hdr.append(ln + p1, (size_t)(p2 - p1));
    size_t sl = s.gets_view(&ln);
    sl = sl ? strnlen(ln, sl) : 1;                        // (end of the stream behind a header: an empty line)
    const int rlen = (int)sl - 1;
    if (rlen <= 0) { R.hdr.resize(h0); return false; }
    if (rc) { R.seq.resize(s0 + (size_t)rlen); for (int i = 0; i < rlen; i++) R.seq[s0 + i] = comp_base_f(ln[rlen - 1 - i]); }
    else R.seq.append(ln, (size_t)rlen);
    if (s.fastq) {
        char *q = nullptr; size_t ql = 0;
        if (s.gets_view(&q) != 0) ql = s.gets_view(&q);
        if (ql == 0) q = nullptr;
        const size_t take = std::min<size_t>((size_t)rlen, q ? strnlen(q, ql) : 0), q0 = R.qual.size();
        if (rc) { R.qual.resize(q0 + take); for (size_t i = 0; i < take; i++) R.qual[q0 + i] = q[take - 1 - i]; }
        else if (take) R.qual.append(q, take);
    }
    R.hoff.push_back((uint32_t)R.hdr.size()); R.soff.push_back((uint32_t)R.seq.size()); R.qoff.push_back((uint32_t)R.qual.size());
    return true;
}

static bool read_into(Source &s, Reads &R, bool rc)
{
    if (s.gz) return read_into_gz(s, R, rc);
    if (!s.fastq) {
        Entry e = s.next_fasta();
        if (e.rlen == 0) return false;
        R.add(e.header.data(), e.header.size(), e.seq.data(), e.seq.size(), rc);
        return true;
    }
    char *ln;                                             // GetNextEntry, GetData.cpp:77-132 (FASTQ branch)
    ssize_t len = s.block_line(&ln);
    if (len == -1) return false;
    const int p1 = hdr_beg(ln, (int)len), p2 = hdr_end(ln, (int)len);
    const size_t h0 = R.hdr.size(), s0 = R.seq.size();
    if (p2 > p1) R.hdr.append(ln + p1, (size_t)(p2 - p1));
    ssize_t rl = s.block_line(&ln);
    const int rlen = rl == -1 ? 0 : (int)rl - 1;
    if (rlen > 0) {
        if (rc) { R.seq.resize(s0 + (size_t)rlen); for (int i = 0; i < rlen; i++) R.seq[s0 + i] = comp_base_f(ln[rlen - 1 - i]); }
        else R.seq.append(ln, (size_t)rlen);
    }
    if (rl != -1) {
        if (s.block_line(&ln) == -1) {}
        ssize_t ql = s.block_line(&ln);
        if (ql < 0) ql = 0;
        if (rlen > 0) {
            const size_t take = std::min<size_t>((size_t)rlen, ql > 0 ? strnlen(ln, (size_t)ql) : 0), q0 = R.qual.size();
            if (rc) { R.qual.resize(q0 + take); for (size_t i = 0; i < take; i++) R.qual[q0 + i] = ln[take - 1 - i]; }
            else R.qual.append(ln, take);
        }
    }
    if (rlen <= 0) { R.hdr.resize(h0); R.seq.resize(s0); return false; }     // an entry of length 0 ends the stream
    R.hoff.push_back((uint32_t)R.hdr.size()); R.soff.push_back((uint32_t)R.seq.size()); R.qoff.push_back((uint32_t)R.qual.size());
    return true;
}

// A Source parsed by its own thread, BLOCK reads at a time (the two mate files are parsed concurrently; mate 2 is
// reverse-complemented there too).  The consumer walks the blocks in file order.
struct Prefetch {
    static const size_t BLOCK = 16384;
    Source *src = nullptr; bool rc = false;
    std::thread th; std::mutex mu; std::condition_variable cv;
    std::deque<std::unique_ptr<Reads>> q; bool eof = false, stop = false;
    std::unique_ptr<Reads> cur; size_t pos = 0;
    void start(Source *s, bool revcomp_mate) {
        src = s; rc = revcomp_mate;
        th = std::thread([this]() {
            while (true) {
                std::unique_ptr<Reads> blk(new Reads());
                blk->seq.reserve(BLOCK * 160); blk->qual.reserve(BLOCK * 160); blk->hdr.reserve(BLOCK * 24);
                bool end = false;
                while (blk->size() < BLOCK) if (!read_into(*src, *blk, rc)) { end = true; break; }
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [this]() { return q.size() < 64 || stop; });
                if (stop) return;
                if (blk->size()) q.push_back(std::move(blk));
                if (end) { eof = true; cv.notify_all(); return; }
                cv.notify_all();
            }
        });
    }
    // appends the next read to R; false at the end of the stream
    bool next_into(Reads &R) {
        if (!cur || pos == cur->size()) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [this]() { return !q.empty() || eof; });
            if (q.empty()) return false;
            cur = std::move(q.front()); q.pop_front(); pos = 0;
            cv.notify_all();
        }
        R.add_from(*cur, pos++);
        return true;
    }
    void finish() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); if (th.joinable()) th.join(); }
    ~Prefetch() { finish(); }
};

// GetNextChunk, GetData.cpp:134-179: one reference-sized chunk appended to `out`
static int next_chunk(Source &s1, Source *s2, bool pair_end, Reads &out, Prefetch *p1 = nullptr, Prefetch *p2 = nullptr)
{
    int count = 0, base = 0;
    while (true) {
        if (!(p1 ? p1->next_into(out) : read_into(s1, out, false))) break;
        base += out.rlen(out.size() - 1); count++;
        if (!(p2 ? p2->next_into(out) : read_into(s2 ? *s2 : s1, out, pair_end))) break;
        base += out.rlen(out.size() - 1); count++;
        if (count == 4000 || base > 1000000) break;
    }
    return count;
}

// ---------------------------------------------------------------------------------------------
// SAM text
// ---------------------------------------------------------------------------------------------
// which formatter ran and its seconds, for the DART_TIMING line of the parallel pipeline
static std::string fast_format_text(const Config &c, const FastStats &f)
{
    char b[384];
    if ((c.device_sam || c.device_bam) && f.fq_device) snprintf(b, sizeof b, "format=device %.3f s (sum over workers: names and qualities resident in HBM, dg_batch_format_sam_resident %.3f s of which kernels %.3f s, text download %.3f s; %zu batches, %.4f s per batch on its worker's path)",
                                              f.t_dev_call + f.t_download, f.t_dev_call, f.t_dev_kernels, f.t_download, f.n_batches, (f.t_dev_call + f.t_download) / (double)std::max<size_t>(1, f.n_batches));
    else if (c.device_sam || c.device_bam) snprintf(b, sizeof b, "format=device %.3f s (sum over workers: gather names and qualities %.3f s, dg_batch_format_sam %.3f s of which kernels %.3f s, text download %.3f s; %zu batches, %.4f s per batch on its worker's path)",
                               f.t_gather + f.t_dev_call + f.t_download, f.t_gather, f.t_dev_call, f.t_dev_kernels, f.t_download, f.n_batches, (f.t_gather + f.t_dev_call + f.t_download) / (double)std::max<size_t>(1, f.n_batches));
    else snprintf(b, sizeof b, "format=host %.3f s", f.t_fmt);
    return b;
}

// the assemble field of the same line: without DART_DEVICE_FASTQ it is what it always was; with the switch it names who cut the text into batches
static std::string fast_assemble_text(const Config &c, const FastStats &f)
{
    char b[384];
    if (!c.device_fastq) snprintf(b, sizeof b, "assemble %.3f s (of which page-locked allocation %.3f s)", f.t_asm, f.t_alloc);
    else if (f.fq_device) snprintf(b, sizeof b, "assemble=device %.3f s (sum over workers: dg_batch_upload_fastq %.3f s of which kernels %.3f s; batch ranges and views on the host %.3f s, of which page-locked allocation %.3f s)",
                                   f.t_fq_call, f.t_fq_call, f.t_fq_kernels, f.t_asm, f.t_alloc);
    else snprintf(b, sizeof b, "assemble=host %.3f s (a record without bases: the host assembles; of which page-locked allocation %.3f s)", f.t_asm, f.t_alloc);
    return b;
}

// ---------------------------------------------------------------------------------------------
// the stages of main.  A stage returns RUN (dart_config.h), or the exit code where main would have returned.
// ---------------------------------------------------------------------------------------------
struct Output { FILE *sam = nullptr; BamWriter bam; };      // -o: the SAM file (its header written); -bo: the BAM writer

// A run that fails leaves no output a user could take for a complete one.  Which files go, by where it failed:
//
//   failure point                                           at            BAM closed here   <out>   <out>.bai   tracks + .markdup.txt
//   a library fails / mates differ in format / a library
//     streams / merge, sort, markdup, a piece, the .bai     BEFORE_CLOSE  yes               yes     yes         yes      (DART_SORT_BAM only:
//   the same without DART_SORT_BAM                          BEFORE_CLOSE  no                stays   -           -         an unsorted run keeps
//   bam.close() itself fails                                CLOSE_FAILED  no (not twice)    yes*    yes         yes       its partial file)
//   a coverage track, the site table or the QC fails (BAM and
//     .bai are complete)                                    AFTER_CLOSE   no                stays   stays       yes      (<out>.sites.tsv, <out>.qc.txt and <out>.rna_metrics.txt go with the tracks)
//
//   * with DART_SORT_BAM; without it the file stays, and none of the others can exist.  (<out>.genes.tab is the gene stage's own.)
enum AbandonAt { BEFORE_CLOSE, CLOSE_FAILED, AFTER_CLOSE };
static void abandon_outputs(const Config &c, Output &o, AbandonAt at)
{
    if (at != AFTER_CLOSE) {
        if (!c.sort_bam) return;
        if (at == BEFORE_CLOSE) (void)o.bam.close();
        remove(c.out);
        if (c.bam_index) remove(c.bai_path.c_str());
    }
    for (const auto &t : c.cov_tracks) remove(t.first.c_str());      // (no failed run leaves a track or the duplicates' counts, stale ones included)
    if (c.mark_dups) remove(c.md_path.c_str());
    if (c.pileup) remove(c.sites_path.c_str());
    if (c.qc) remove(c.qc_path.c_str());
    if (c.rna_gtf) remove(c.rna_path.c_str());
}

// The contexts: one root per device (the index files go to its HBM inside dg_init_files, main.cpp:231-235 / bwt_index.cpp:147-159), clones
// for the batches in flight.  The look-up aids are built in the background while the first batches are mapped (DART_SYNC_AIDS=1: before).
// Then the gene annotation and the chromosome names to every root.
static int make_contexts(Job &job, const HostIndex &ix, const GtfAnnotation &gtf, const GtfTranscripts &rna, const GtfTranscripts &txq, int n_gpu)
{
    {
        const std::string pb = std::string(job.cfg.index) + ".bwt", ps = std::string(job.cfg.index) + ".sa", pp = std::string(job.cfg.index) + ".pac";
        dg_index_files files;
        files.bwt_path = pb.c_str(); files.sa_path = ps.c_str(); files.pac_path = pp.c_str();
        files.l_pac = ix.l_pac; files.n_chr = (int32_t)ix.names.size(); files.chr_off = ix.off.data(); files.chr_len = ix.len.data();
        {   // the size of the job, from the sizes of its input files: ~250 bytes per FASTQ read of 2x101 (a quarter of that gzipped; FASTA: half).
            // A coarse figure is all the library needs: it decides between lean and full look-up aids at some hundred million reads.
            // An input whose size cannot be known (a FIFO, process substitution, /dev/stdin, a failed stat) makes the whole job "unknown" (0): the library then
            // builds the full aids -- a very large piped job must not run its seeding stage at half speed for its whole length
            uint64_t bytes = 0; struct stat st; bool known = true;
            for (auto &v : {&job.cfg.f1, &job.cfg.f2}) for (auto &fn : *v) {
                if (stat(fn.c_str(), &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) bytes += (uint64_t)st.st_size * (fn.size() > 3 && fn.substr(fn.size() - 3) == ".gz" ? 4u : 1u);
                else known = false;
            }
            files.expected_reads = known ? std::max<uint64_t>(1, bytes / 250) : 0;
            if (job.cfg.has_expected_reads) files.expected_reads = job.cfg.expected_reads;
        }
        const int init_flags = job.cfg.sync_aids ? 0 : DG_INIT_ASYNC_AIDS;
        job.roots.assign(n_gpu, nullptr);
        std::vector<int> st(n_gpu, 0); std::vector<std::string> msg(n_gpu);
        std::vector<std::thread> th;
        for (int d = 0; d < n_gpu; d++) th.emplace_back([&, d]() { job.roots[d] = dg_init_files(&files, &job.cfg.p, job.cfg.same_device_times ? 0 : d, init_flags, &st[d]); if (!job.roots[d]) msg[d] = dg_last_error(nullptr); });
        for (auto &t : th) t.join();
        for (int d = 0; d < n_gpu; d++) if (!job.roots[d]) {
            if (st[d] == DG_ERR_ARG) fprintf(stderr, "\n\nError! Index files are corrupt!\n"); else fprintf(stderr, "\nError! GPU %d: %s\n", d, msg[d].c_str());
            for (auto r : job.roots) if (r) dg_destroy(r);
            return st[d] == DG_ERR_ARG ? 0 : 1;
        }
        for (int d = 0; d < n_gpu; d++) {
            job.ctx.push_back(job.roots[d]);
            for (int k = 1; k < job.cfg.inflight; k++) {
                int st2 = 0; dg_ctx *cl = dg_clone(job.roots[d], &st2);
                if (!cl) { fprintf(stderr, "Error! GPU %d: %s\n", d, dg_last_error(nullptr)); return 1; }
                job.ctx.push_back(cl); job.clones.push_back(cl);
            }
        }
    }
    if (job.cfg.gene_gtf) {      // the annotation goes to every root; its job.clones count with it
        dg_gene_annot ann; ann.n_genes = (uint32_t)gtf.genes.size(); ann.pad = 0; ann.n_exons = gtf.exons.size(); ann.exons = gtf.exons.data();
        for (dg_ctx *r : job.roots) if (dg_gene_set_annotation(r, &ann, nullptr)) {
            fprintf(stderr, "Error! DART_GENE_COUNTS=%s: %s\n", job.cfg.gene_gtf, dg_last_error(r));
            for (auto x : job.clones) dg_destroy(x);
            for (auto x : job.roots) dg_destroy(x);
            return 1;
        }
    }
    if (job.cfg.rna_gtf) {       // the transcripts go to every root too
        dg_rna_annot ann; ann.n_tx = (uint32_t)rna.tx.size(); ann.pad = 0; ann.n_exons = rna.exons.size(); ann.tx = rna.tx.data(); ann.exons = rna.exons.data();
        for (dg_ctx *r : job.roots) if (dg_rna_set_annotation(r, &ann, nullptr, nullptr)) {
            fprintf(stderr, "Error! DART_RNA_METRICS=%s: %s\n", job.cfg.rna_gtf, dg_last_error(r));
            for (auto x : job.clones) dg_destroy(x);
            for (auto x : job.roots) dg_destroy(x);
            return 1;
        }
    }
    if (job.cfg.tx_gtf) {        // and the expression stage's transcripts
        dg_rna_annot ann; ann.n_tx = (uint32_t)txq.tx.size(); ann.pad = 0; ann.n_exons = txq.exons.size(); ann.tx = txq.tx.data(); ann.exons = txq.exons.data();
        for (dg_ctx *r : job.roots) if (dg_tx_set_annotation(r, &ann, nullptr, nullptr)) {
            fprintf(stderr, "Error! DART_TX_QUANT=%s: %s\n", job.cfg.tx_gtf, dg_last_error(r));
            for (auto x : job.clones) dg_destroy(x);
            for (auto x : job.roots) dg_destroy(x);
            return 1;
        }
    }
    job.names = ix.names;
    if (job.cfg.device_sam || job.cfg.device_bam || job.cfg.device_sj) {
        std::vector<uint32_t> noff{0}; std::string nflat;
        for (const std::string &nm : ix.names) { nflat += nm; noff.push_back((uint32_t)nflat.size()); }
        for (dg_ctx *r : job.roots) if (dg_set_chr_names(r, (int)ix.names.size(), noff.data(), nflat.data())) { fprintf(stderr, "Error! %s\n", dg_last_error(r)); return 1; }
    }
    return RUN;
}

// The header text, and the SAM file or the BAM writer open with it written.
static int open_output(Job &job, const HostIndex &ix, Output &o)
{
    std::string hdr_text = std::string("@PG\tID:Dart\tPN:Dart\tVN:") + VersionStr + "\n";      // Mapping.cpp:741-751
    if (job.cfg.sort_bam) hdr_text = "@HD\tVN:1.6\tSO:coordinate\n" + hdr_text;
    for (size_t i = 0; i < ix.names.size(); i++) hdr_text += "@SQ\tSN:" + ix.names[i] + "\tLN:" + std::to_string((long long)ix.len[i]) + "\n";
    if (job.cfg.bam) {
        if (!o.bam.open(job.cfg.out, hdr_text, ix.names, std::vector<int64_t>(ix.len.begin(), ix.len.end()), job.cfg.threads)) { fprintf(stderr, "Cannot write %s\n", job.cfg.out); return 1; }
    } else {
        o.sam = fopen(job.cfg.out, "w+");     // (read access too: the parallel pipeline maps the file to write it)
        if (!o.sam) { fprintf(stderr, "Cannot write %s\n", job.cfg.out); return 1; }
        fwrite(hdr_text.data(), 1, hdr_text.size(), o.sam);
    }
    BamWriter *bw = &o.bam;
    if (job.cfg.device_bam) job.bam_sink = [bw](const char *p, size_t n, long long records, long long refused) { return bw->add_bgzf_blocks(p, n, records, refused); };
    return RUN;
}

// The read files of a library when they go through the host's readers.  Plain FASTQ goes through the parallel host pipeline (fast_fastq.h); FASTA, .gz, -bo
// and DART_STREAMING=1 through the streaming one: one thread per mate file inflates (zlib, 1 MB at a time) and parses into flat buffers.
struct LibIO { Source s1, s2; Prefetch pf1, pf2; bool sep = false, gz = false, fastq = false, fast_host = false; int state = -1; };
// state: 0 = opened, 1 = a file cannot be opened (the library is skipped, Mapping.cpp:765-779), 2 = mates in different formats
static std::unique_ptr<LibIO> open_lib(const Config &c, size_t lib, const FileProbe &m1, const FileProbe *m2, const PipelineChoice &ch)
{
    std::unique_ptr<LibIO> io(new LibIO());
    LibIO &L = *io;
    const std::string &fn = c.f1[lib];
    L.gz = m1.gz; L.fastq = m1.fastq;
    L.s1.fastq = L.s2.fastq = L.fastq;
    if (L.gz) L.s1.gz = gzopen(fn.c_str(), "rb"); else L.s1.fp = fopen(fn.c_str(), "r");
    if (m2) {
        L.sep = true;
        if (L.fastq != m2->fastq) { fprintf(stderr, "Error! %s and %s are with different format...\n", fn.c_str(), c.f2[lib].c_str()); L.state = 2; return io; }
        if (L.gz) L.s2.gz = gzopen(c.f2[lib].c_str(), "rb"); else L.s2.fp = fopen(c.f2[lib].c_str(), "r");
    }
    if ((!L.s1.fp && !L.s1.gz) || (L.sep && !L.s2.fp && !L.s2.gz)) { L.state = 1; return io; }
    if (L.s1.gz) gzbuffer(L.s1.gz, 1u << 20);
    if (L.s2.gz) gzbuffer(L.s2.gz, 1u << 20);
    L.fast_host = ch.plain;
    if (L.sep && !L.fast_host) { L.pf1.start(&L.s1, false); L.pf2.start(&L.s2, true); }      // (separate mate files: paired, mate 2 reverse-complemented)
    L.state = 0;
    return io;
}

// What is known and begun of a library before its turn; for library 0 that is before the device is touched.
struct LibPlan {
    FileProbe m1, m2; PipelineChoice choice;
    FastqIndex pre;                         // library 0: its read files are mapped and indexed (or inflated whole) while the HIP runtime starts, the genome index loads and dg_init_files runs
    std::unique_ptr<LibIO> io;              // library 0 when it streams: opened before the index goes to the GPU, so that its files are read meanwhile
    const FileProbe *mate2(const Config &c) const { return c.two_files() ? &m2 : nullptr; }
    void look(const Config &c, size_t lib) {
        m1 = probe(c.f1[lib]); if (c.two_files()) m2 = probe(c.f2[lib]);
        choice = choose_pipelines(c, m1, mate2(c), m1.gz && lib_deflate().ok());      // (libdeflate is looked for only where a .gz file could use it)
    }
};

// One library through the parallel pipeline, by whichever of its three ways in: the call, its place in the SAM file, its failure and its `[dart timing]` line.
static int run_fast_stage(Job &job, Output &o, size_t lib, FastqIndex *pre, GzDevPlan *plan, bool inflated_whole)
{
    if (job.cfg.two_files()) job.pair_end = true;
    // the parallel pipeline's place in the output: the SAM file's descriptor and offset; with DART_DEVICE_BAM the blocks go through job.bam_sink instead
    job.sam_fd = -1; job.sam_off = 0;
    if (o.sam) { fflush(o.sam); job.sam_off = (uint64_t)ftello(o.sam); job.sam_fd = fileno(o.sam); }
    std::string ferr; FastStats fst;
    const int frc = run_fast_library(job, job.cfg.f1[lib].c_str(), job.cfg.two_files() ? job.cfg.f2[lib].c_str() : nullptr, pre, plan, fst, ferr);
    if (o.sam) fseeko(o.sam, (off_t)job.sam_off, SEEK_SET);
    if (frc) {   // under DART_SORT_BAM no partial file is left, and a store that could not grow says which switch asked for the memory
        abandon_outputs(job.cfg, o, BEFORE_CLOSE);
        if (job.cfg.sort_bam && frc == DG_ERR_CAPACITY) fprintf(stderr, "\nError! DART_SORT_BAM=1: the records do not fit in device memory: %s\n", ferr.c_str());
        else fprintf(stderr, "\nError! GPU mapping failed (%d): %s\n", frc, ferr.c_str());
        return 1;
    }
    job.sort_ordinal_base += fst.n_batches;
    if (job.cfg.timing) {
        char mid[256];
        if (plan) snprintf(mid, sizeof mid, "gz=device (check pass over every block %.3f s; %zu chunks, waits for the tail chain %.3f s summed over workers)", fst.t_gz_check, plan->chunks.size(), fst.t_gz_tail);
        else snprintf(mid, sizeof mid, "%s %.3f s", inflated_whole ? "inflate (libdeflate, whole files) + index" : "index", fst.t_index);
        fprintf(stderr, "[dart timing] start-up %.3f s (%s), %s, %s, map (sum over workers) %.3f s, %s, write %.3f s%s\n", job.start_up_s, dg_init_report(job.roots[0]), mid,
                fast_assemble_text(job.cfg, fst).c_str(), fst.t_map, fast_format_text(job.cfg, fst).c_str(), fst.t_write, job.cfg.bam_dev_note);
    }
    return RUN;
}

// ---- the streaming pipeline: reader thread -> mapping workers (one per context) -> ordered writer ----
// Contexts = devices x DART_INFLIGHT (dg_clone: contexts of a device share its index), so the next batch is
// parsed, and the previous one formatted and written, while the GPUs map.  Output order = input order.
struct Streaming {
    struct Batch { Reads rd; int odd = 0; std::unique_ptr<dg_read_out[]> ro; std::unique_ptr<dg_report_out[]> po; std::unique_ptr<uint32_t[]> cig; std::unique_ptr<dg_sj_out[]> sj;   // new T[n]: no zero fill
                   size_t n_reads = 0; size_t used[3] = {0, 0, 0}; int rc = 0; std::string err; size_t seq = 0; std::vector<TextBuf> outs; std::vector<Counters> cts; double t_dev = 0; };
    Job &job; const Config &c; LibIO &L; Output &o;
    std::mutex mu; std::condition_variable cv_in, cv_out, cv_space;
    std::deque<std::unique_ptr<Batch>> inq; std::map<size_t, std::unique_ptr<Batch>> done;
    bool reader_done = false, failed = false; size_t in_flight = 0;
    const size_t max_in_flight;
    double t_read = 0, t_map = 0, t_fmt = 0, t_write = 0;
    int bad_rc = 0; std::string bad_msg;      // the batch that failed
    Streaming(Job &j, LibIO &l, Output &out) : job(j), c(j.cfg), L(l), o(out), max_in_flight(j.ctx.size() + 2) {}

    void read_all() {
        bool eof = false; size_t seqno = 0;
        while (!eof) {
            // an odd chunk (only the last can be) is mapped on its own, unpaired (Mapping.cpp:598)
            const double t = now_s();
            std::unique_ptr<Batch> b(new Batch());
            b->rd.seq.reserve(c.batch_reads * 110); b->rd.qual.reserve(c.batch_reads * 110); b->rd.hdr.reserve(c.batch_reads * 16);
            while (b->rd.size() < c.batch_reads) {
                int n = next_chunk(L.s1, L.sep ? &L.s2 : nullptr, job.pair_end, b->rd, L.sep ? &L.pf1 : nullptr, L.sep ? &L.pf2 : nullptr);
                if (n == 0) { eof = true; break; }
                if (n & 1) { b->odd = n; eof = true; break; }
            }
            t_read += now_s() - t;
            if (b->rd.size() == 0) break;
            b->seq = seqno++;
            std::unique_lock<std::mutex> lk(mu);
            cv_space.wait(lk, [&]() { return in_flight < max_in_flight || failed; });
            if (failed) break;
            in_flight++; inq.push_back(std::move(b));
            cv_in.notify_one();
        }
        std::lock_guard<std::mutex> lk(mu);
        reader_done = true; cv_in.notify_all(); cv_out.notify_all();
    }
    // device formatter: the text of the reads [first, first + n) that x has just mapped, appended to the batch's (Reads holds names and qualities in the call's flat form)
    int device_text(Batch &b, dg_ctx *x, int first, int n_pair_mode) {
        const double t = now_s();
        dg_sam_text in; in.hdr_off = b.rd.hoff.data() + first; in.hdr = b.rd.hdr.data(); in.qual_off = b.rd.qoff.data() + first; in.qual = L.fastq ? b.rd.qual.data() : nullptr; in.n_pair_mode = n_pair_mode;
        size_t nb = 0; uint64_t ct[3] = {0, 0, 0};
        int rc = dg_batch_format_sam(x, &in, c.unique ? DG_SAM_UNIQUE_ONLY : 0u, &nb, ct, nullptr);
        if (!rc) {
            TextBuf &out = b.outs[0];
            out.need(nb);
            rc = dg_batch_download_sam(x, out.b + out.n, nb);
            out.n += nb;
            b.cts[0].unmapped += (long long)ct[0]; b.cts[0].unique += (long long)ct[1]; b.cts[0].paired += (long long)ct[2];
        }
        b.t_dev += now_s() - t;
        return rc;
    }
    void map_one(Batch &b, dg_ctx *x) {
        const int n = (int)b.rd.size(), n_even = n - b.odd;
        const std::vector<uint32_t> &off = b.rd.soff; std::vector<uint16_t> rl(n); const std::string &flat = b.rd.seq;   // the parsed bases are the device input
        for (int k = 0; k < n; k++) {
            if (b.rd.rlen(k) > DG_MAX_RLEN) { b.rc = DG_ERR_ARG; b.err = "read longer than DG_MAX_RLEN"; return; }
            rl[k] = (uint16_t)b.rd.rlen(k);
        }
        b.ro.reset(new dg_read_out[n]); b.n_reads = (size_t)n;
        size_t caps[3] = { (size_t)n * 4 + 1024, (size_t)n * 16 + 4096, (size_t)n + 1024 };
        bool gene_even_counted = false;    // DART_GENE_COUNTS: likewise, the first part's units
        bool tx_even_counted = false;      // DART_TX_QUANT: likewise
        bool sj_even_counted = false;      // DART_DEVICE_SJ: a batch runs in two parts (pairs, then an odd tail); the first part's tuples are counted once, also when the second part makes the batch run again
        for (int attempt = 0; attempt < 2; attempt++) {
            b.po.reset(new dg_report_out[caps[0]]); b.cig.reset(new uint32_t[caps[1]]); if (!c.device_sj) b.sj.reset(new dg_sj_out[caps[2]]);
            size_t used1[3] = {0, 0, 0}, used2[3] = {0, 0, 0};
            dg_params p = c.p; p.paired = job.pair_end ? 1 : 0;
            dg_set_params(x, &p);
            if (c.device_sam) { b.outs = std::vector<TextBuf>(1); b.cts.assign(1, Counters()); b.t_dev = 0; }
            int rc = n_even ? dg_map_batch(x, n_even, off.data(), rl.data(), flat.data(), b.ro.get(), b.po.get(), b.cig.get(), b.sj.get(), caps, used1) : 0;
            if (rc == 0 && n_even && c.device_sj && !sj_even_counted) { rc = sj_accumulate(job, x); sj_even_counted = rc == 0; }
            if (rc == 0 && n_even && c.gene_gtf && !gene_even_counted) { rc = gene_accumulate(job, x, job.pair_end ? n_even : 0); gene_even_counted = rc == 0; }
            if (rc == 0 && n_even && c.tx_gtf && !tx_even_counted) { rc = tx_accumulate(job, x, job.pair_end ? n_even : 0); tx_even_counted = rc == 0; }
            if (rc == 0 && n_even && c.device_sam) rc = device_text(b, x, 0, job.pair_end ? n_even : 0);
            if (rc == 0 && b.odd) {
                p.paired = 0; dg_set_params(x, &p);
                size_t caps2[3] = { caps[0] - used1[0], caps[1] - used1[1], caps[2] - used1[2] };
                rc = dg_map_batch(x, b.odd, off.data() + n_even, rl.data() + n_even, flat.data(), b.ro.get() + n_even, b.po.get() + used1[0],
                                  b.cig.get() + used1[1], c.device_sj ? nullptr : b.sj.get() + used1[2], caps2, used2);
                if (rc == 0 && c.device_sj) rc = sj_accumulate(job, x);
                if (rc == 0 && c.gene_gtf) rc = gene_accumulate(job, x, 0);
                if (rc == 0 && c.tx_gtf) rc = tx_accumulate(job, x, 0);
                if (rc == 0 && c.device_sam) rc = device_text(b, x, n_even, 0);      // (before the offsets below are rebased: the device holds the batch's own)
                if (rc == DG_ERR_CAPACITY) for (int q = 0; q < 3; q++) used2[q] += used1[q];
                else {
                    for (int k = n_even; k < n; k++) { b.ro[k].rep_off += (int32_t)used1[0]; b.ro[k].sj_off += (int32_t)used1[2]; }
                    for (size_t k = 0; k < used2[0]; k++) b.po[used1[0] + k].cigar_off += (uint32_t)used1[1];
                    if (!c.device_sj) for (size_t k = 0; k < used2[2]; k++) b.sj[used1[2] + k].read_idx += n_even;
                }
            }
            if (rc == DG_ERR_CAPACITY && attempt == 0) {       // `used` holds the need: grow once and repeat
                for (int q = 0; q < 3; q++) caps[q] = std::max(caps[q], used1[q] + used2[q]) * 2 + 1024;
                continue;
            }
            b.rc = rc; if (rc) b.err = dg_last_error(x);
            for (int q = 0; q < 3; q++) b.used[q] = used1[q] + used2[q];
            return;
        }
    }
    void format_one(Batch &b) {
        const int n = (int)b.rd.size(), n_pair_mode = job.pair_end ? n - b.odd : 0;
        const int nt = std::max(1, std::min(c.threads, n / 2000 + 1));
        b.outs = std::vector<TextBuf>(nt); b.cts.assign(nt, Counters());
        std::vector<RView> V(n);      // the stored reads as the formatter sees them (mate 2 was reverse-complemented by its parser)
        for (int k = 0; k < n; k++) V[k] = RView{b.rd.hdr.data() + b.rd.hoff[k], b.rd.seq.data() + b.rd.soff[k], b.rd.qual.data() + b.rd.qoff[k], b.rd.hoff[k + 1] - b.rd.hoff[k], b.rd.soff[k + 1] - b.rd.soff[k], b.rd.qoff[k + 1] - b.rd.qoff[k], false};
        std::vector<std::thread> ft;
        int per = ((n + nt - 1) / nt + 1) & ~1;
        for (int t = 0; t < nt; t++) {
            const int lo = std::min(n, t * per), hi = std::min(n, (t + 1) * per);
            ft.emplace_back([&, t, lo, hi]() { format_views(V.data(), lo, hi, n_pair_mode, b.ro.get(), b.po.get(), b.cig.get(), job.names, c.unique, c.multi, L.fastq, b.outs[t], b.cts[t]); });
        }
        for (auto &t : ft) t.join();
        b.rd = Reads();                                      // the text is all the writer needs
    }
    void work(dg_ctx *x) {
        while (true) {
            std::unique_ptr<Batch> b;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_in.wait(lk, [&]() { return !inq.empty() || reader_done || failed; });
                if (failed || inq.empty()) return;
                b = std::move(inq.front()); inq.pop_front();
            }
            double t = now_s();
            map_one(*b, x);
            double tm = now_s() - t; t = now_s();
            if (!b->rc && !c.device_sam) format_one(*b);
            double tf = now_s() - t;
            if (c.device_sam) { tm -= b->t_dev; tf = b->t_dev; b->rd = Reads(); }
            std::lock_guard<std::mutex> lk(mu);
            t_map += tm; t_fmt += tf;
            if (b->rc) failed = true;
            const size_t k = b->seq;
            done[k] = std::move(b);
            cv_out.notify_all(); if (failed) { cv_in.notify_all(); cv_space.notify_all(); }
        }
    }
    // the ordered writer (the caller's thread); false: a batch failed (bad_rc, bad_msg)
    bool write_all() {
        size_t next_out = 0;
        while (true) {
            std::unique_ptr<Batch> b;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_out.wait(lk, [&]() { return done.count(next_out) || failed || (reader_done && in_flight == 0); });
                if (done.count(next_out)) { b = std::move(done[next_out]); done.erase(next_out); }
                else if (failed) { for (auto &kv : done) if (kv.second->rc) { bad_rc = kv.second->rc; bad_msg = kv.second->err; } return false; }
                else return true;
            }
            if (b->rc) { bad_rc = b->rc; bad_msg = b->err; std::lock_guard<std::mutex> lk(mu); failed = true; cv_in.notify_all(); cv_space.notify_all(); return false; }
            const double t = now_s();
            const size_t n = b->n_reads;
            if (c.bam) {                                     // Mapping.cpp:655-662: every SAM line -> one BAM record
                std::vector<std::pair<const char *, size_t>> chunks;
                for (size_t t2 = 0; t2 < b->outs.size(); t2++) chunks.emplace_back(b->outs[t2].b, b->outs[t2].n);
                o.bam.add_sam_chunks(chunks);
            }
            for (size_t t2 = 0; t2 < b->outs.size(); t2++) {
                if (!c.bam) fwrite(b->outs[t2].b, 1, b->outs[t2].n, o.sam);
                job.total.unique += b->cts[t2].unique; job.total.unmapped += b->cts[t2].unmapped; job.total.paired += b->cts[t2].paired;
            }
            batch_written(job, (long long)n, b->sj.get(), b->used[2]);
            t_write += now_s() - t;
            next_out++;
            std::lock_guard<std::mutex> lk(mu);
            in_flight--; cv_space.notify_all();
        }
    }
};

static int run_streaming_stage(Job &job, Output &o, LibIO &L)
{
    Streaming s(job, L, o);
    std::thread reader([&s]() { s.read_all(); });
    std::vector<std::thread> workers;
    for (dg_ctx *x : job.ctx) workers.emplace_back([&s, x]() { s.work(x); });
    const bool good = s.write_all();
    reader.join();
    L.pf1.finish(); L.pf2.finish();
    for (auto &w : workers) w.join();
    if (!good) { fprintf(stderr, "\nError! GPU mapping failed (%d): %s\n", s.bad_rc, s.bad_msg.c_str()); return 1; }
    if (job.cfg.timing) fprintf(stderr, "[dart timing] read+parse %.3f s, map (sum over workers) %.3f s, format=%s %.3f s, write %.3f s%s\n", s.t_read, s.t_map, job.cfg.device_sam ? "device" : "host", s.t_fmt, s.t_write, job.cfg.bam_host_note);
    return RUN;
}

// One library: the pipelines it may take are tried in their order (choose_pipelines); the first that takes it runs it.
static int run_library(Job &job, Output &o, size_t lib, LibPlan &plan)
{
    const char *f1 = job.cfg.f1[lib].c_str(), *f2 = job.cfg.two_files() ? job.cfg.f2[lib].c_str() : nullptr;
    if (plan.choice.gz_device) {   // BGZF FASTQ inflated on the device: the plan's check pass decides
        GzDevPlan gz;
        if (gz.make(f1, f2, job.pair_end || job.cfg.two_files(), job.cfg.batch_reads, job.ctx[0])) return run_fast_stage(job, o, lib, nullptr, &gz, false);
    }
    if (plan.choice.gz_whole) {   // .gz FASTQ inflated whole: the parallel pipeline on the inflated text (library 0's files have been inflating since before the GPU was touched)
        if (lib == 0 && !plan.choice.gz_device) plan.pre.wait();
        else plan.pre.run(f1, f2, job.cfg.threads, true, job.cfg.gz_whole_max);
        if (plan.pre.ok) {
            const int rc = run_fast_stage(job, o, lib, &plan.pre, nullptr, true);
            if (rc == RUN) { plan.pre.m1.close_now(); plan.pre.m2.close_now(); }
            return rc;
        }
    }
    if (!plan.io) plan.io = open_lib(job.cfg, lib, plan.m1, plan.mate2(job.cfg), plan.choice);      // (library 0 may have been opened before the index went to the GPU: its files are being inflated and parsed since)
    LibIO &L = *plan.io;
    if (L.state == 2) { abandon_outputs(job.cfg, o, BEFORE_CLOSE); return 1; }      // (under DART_SORT_BAM no failed run leaves a file)
    if (L.state == 1) return RUN;
    if (job.cfg.sort_bam && !L.fast_host) {
        fprintf(stderr, "\nError! DART_SORT_BAM=1: %s takes the streaming pipeline (FASTA, a streamed .gz, DART_STREAMING), which has no sorted output\n", f1);
        abandon_outputs(job.cfg, o, BEFORE_CLOSE);
        return 1;
    }
    if (job.cfg.cuts() && !L.fast_host) {      // (untrimmed reads are never mapped silently)
        fprintf(stderr, "\nError! DART_TRIM_* / DART_UMI: %s takes the streaming pipeline (FASTA, a streamed .gz), where nothing is trimmed\n", f1);
        abandon_outputs(job.cfg, o, BEFORE_CLOSE);
        return 1;
    }
    if (L.sep) job.pair_end = true;
    const int rc = L.fast_host ? run_fast_stage(job, o, lib, &plan.pre, nullptr, false) : run_streaming_stage(job, o, L);
    if (rc != RUN) return rc;
    if (L.s1.fp) fclose(L.s1.fp);
    if (L.s2.fp) fclose(L.s2.fp);
    L.s1.inf.reset(); L.s2.inf.reset();              // (the inflater threads end before their files are closed)
    if (L.s1.gz) gzclose(L.s1.gz);
    if (L.s2.gz) gzclose(L.s2.gz);
    return RUN;
}

// DART_SORT_BAM: the clones' stores into their root's, one sort, and the sorted array out in pieces of whole BGZF blocks: compress -> download -> write;
// DART_MARK_DUPLICATES, then DART_BAM_TAGS, before the first piece, DART_BAM_INDEX behind the last
static int finish_sorted_bam(Job &job, Output &o)
{
    dg_ctx *root = job.roots[0];
    auto fail = [&](const char *lead, const char *what) { abandon_outputs(job.cfg, o, BEFORE_CLOSE); fprintf(stderr, "%s%s\n", lead, what); return 1; };      // (lead: the message up to its last word)
    auto sort_fail = [&](int rc) { return fail(rc == DG_ERR_CAPACITY ? "\nError! DART_SORT_BAM=1: the records do not fit in device memory: " : "\nError! DART_SORT_BAM=1: ", dg_last_error(root)); };
    const double ts0 = now_s();
    int rc = 0;
    for (int k = 1; k < job.cfg.inflight; k++) if ((rc = dg_bam_sort_merge(root, job.ctx[(size_t)k]))) return sort_fail(rc);
    size_t n_sorted = 0, n_raw = 0; float fin_ms = 0.f;
    if ((rc = dg_bam_sort_finish(root, &n_sorted, &n_raw, &fin_ms))) return sort_fail(rc);
    // DART_MARK_DUPLICATES: the verdicts go into the sorted records before any piece is compressed
    // (DART_MARKDUP_UMI: with the UMI at the end of the name in the signature, and four more counts)
    uint64_t md_stats[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; float md_ms = 0.f; double t_md = 0.0;
    if (job.cfg.mark_dups) {
        const double tm0 = now_s();
        const int n_md = job.cfg.md_umi ? 12 : 8;
        if (job.cfg.md_umi) {
            dg_umi_rules rules; memset(&rules, 0, sizeof rules);
            rules.max_edit = job.cfg.md_umi == 2 ? 1u : 0u; rules.sep = job.cfg.md_umi_sep;
            if ((rc = dg_bam_markdup_umi_finish(root, &rules, 0u, md_stats, &md_ms))) return fail("\nError! DART_MARKDUP_UMI: ", dg_last_error(root));
        } else if ((rc = dg_bam_markdup_finish(root, 0u, md_stats, &md_ms))) return fail("\nError! DART_MARK_DUPLICATES=1: ", dg_last_error(root));
        static const char *const md_names[12] = {"examined_records", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "candidates_in_crowded_runs", "records_marked_duplicate", "largest_family",
                                                 "records_with_umi", "pair_families_of_several_umis", "umi_groups_absorbed", "crowded_umi_families"};
        FILE *mf = fopen(job.cfg.md_path.c_str(), "wb");
        bool ok = mf != nullptr;
        for (int k = 0; k < n_md && ok; k++) ok = fprintf(mf, "%s\t%llu\n", md_names[k], (unsigned long long)md_stats[k]) > 0;
        if (!(mf && fclose(mf) == 0 && ok)) return fail("Error while writing ", job.cfg.md_path.c_str());
        t_md = now_s() - tm0;
    }
    // DART_BAM_TAGS: MD, NM, ts onto the (marked) records, also before any piece is compressed; the array the pieces are cut from is the new one
    uint64_t tg_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0}; float tg_ms[2] = {0.f, 0.f}; double t_tg = 0.0;
    if (job.cfg.bam_tags) {
        const double tt0 = now_s();
        if ((rc = dg_bam_tags_finish(root, job.cfg.bam_tags, &n_raw, tg_stats, nullptr))) return fail(rc == DG_ERR_CAPACITY ? "\nError! DART_BAM_TAGS: the tagged records do not fit in device memory: " : "\nError! DART_BAM_TAGS: ", dg_last_error(root));
        (void)dg_bam_tags_device_ms(root, tg_ms);
        t_tg = now_s() - tt0;
    }
    const double ts1 = now_s();
    const size_t block = 0xff00;
    // whole blocks, at least one, at most the array (whatever the variable holds -- a huge or unparsable value included): the file is the same whatever the piece
    const size_t all_blocks = std::max<size_t>(1, (n_raw + block - 1) / block);
    const double want_blocks = job.cfg.sort_piece_mb > 0.0 ? job.cfg.sort_piece_mb * 1048576.0 / (double)block : 0.0;      // (a NaN compares false)
    const size_t piece = (want_blocks >= (double)all_blocks ? all_blocks : std::max<size_t>(1, (size_t)want_blocks)) * block;
    const size_t cap = std::min(piece, n_raw) + 31 * (std::min(piece, n_raw) / block + 1);
    char *buf = (char *)dg_host_alloc(cap ? cap : 1);
    const bool pinned = buf != nullptr;
    if (!buf) buf = (char *)malloc(cap ? cap : 1);
    if (!buf) { abandon_outputs(job.cfg, o, BEFORE_CLOSE); fprintf(stderr, "\nError! DART_SORT_BAM=1: no host memory for a piece of %zu bytes\n", cap); return 1; }
    float z_ms = 0.f; size_t n_pieces = 0, n_out = 0;
    bool wrote = true;
    for (size_t off = 0; off < n_raw && !rc && wrote; off += piece, n_pieces++) {
        size_t nb = 0; float ms = 0.f;
        rc = dg_bam_sort_compress(root, off, std::min(piece, n_raw - off), job.cfg.bgzf_dynamic ? DG_BGZF_DYNAMIC : 0u, &nb, &ms);
        if (!rc) rc = dg_batch_download_bam(root, buf, cap);
        if (!rc) { wrote = o.bam.add_bgzf_blocks(buf, nb, 0, 0); z_ms += ms; n_out += nb; }
    }
    if (pinned) dg_host_free(buf); else free(buf);
    if (rc) return sort_fail(rc);
    if (!wrote) return fail("Error while writing ", job.cfg.out);
    const double ts2 = now_s();
    // DART_BAM_INDEX: the blocks' sizes are those the pieces above left in HBM; the records' blocks begin behind the header's
    size_t bai_bytes = 0; float bai_ms = 0.f;
    if (job.cfg.bam_index) {
        if (dg_bam_index_finish(root, o.bam.first_block_offset(), nullptr, 0, &bai_bytes, nullptr, &bai_ms)) return fail("\nError! DART_BAM_INDEX=1: ", dg_last_error(root));
        std::vector<char> bai(bai_bytes ? bai_bytes : 1);
        if (dg_bam_index_download(root, bai.data(), bai_bytes)) return fail("\nError! DART_BAM_INDEX=1: ", dg_last_error(root));
        FILE *bf = fopen(job.cfg.bai_path.c_str(), "wb");
        const bool ok = bf && fwrite(bai.data(), 1, bai_bytes, bf) == bai_bytes;
        if (!(bf && fclose(bf) == 0 && ok)) return fail("Error while writing ", job.cfg.bai_path.c_str());
    }
    if (job.cfg.timing) {
        char idx_note[128] = "";
        if (job.cfg.bam_index) snprintf(idx_note, sizeof idx_note, "; index %.3f s (kernels %.3f s, %zu bytes)", now_s() - ts2, bai_ms * 1e-3, bai_bytes);
        fprintf(stderr, "[dart timing]%s: %zu records, %zu raw bytes; accumulate (sum over workers) %.3f s; merge + finish %.3f s (kernels %.3f s); compress + download + write %.3f s (BGZF kernels %.3f s, %zu pieces of %zu bytes, %zu bytes out)%s\n",
                job.cfg.bam_dev_note + 1, n_sorted, n_raw, job.sort_acc_ns.load() * 1e-9, ts1 - ts0 - t_md - t_tg, fin_ms * 1e-3, ts2 - ts1, z_ms * 1e-3, n_pieces, piece, n_out, idx_note);
        if (job.cfg.mark_dups)
            fprintf(stderr, "[dart timing] markdup: %llu examined records, %llu pairs, %llu fragments; %llu records marked (%llu pairs, %llu fragments); %.3f s (kernels %.3f s)\n",
                    (unsigned long long)md_stats[0], (unsigned long long)md_stats[1], (unsigned long long)md_stats[2], (unsigned long long)md_stats[6], (unsigned long long)md_stats[3],
                    (unsigned long long)md_stats[4], t_md, md_ms * 1e-3);
        if (job.cfg.bam_tags)
            fprintf(stderr, "[dart timing] tags: %llu records rewritten, %llu + %llu copied (not eligible, aux unreadable), %llu old tags removed, %llu mismatches, %llu inserted + deleted bases, %llu ts written, %llu + %llu introns without (no motif, conflict); %zu raw bytes; %.3f s (length pass %.3f s, write pass %.3f s)\n",
                    (unsigned long long)tg_stats[0], (unsigned long long)tg_stats[1], (unsigned long long)tg_stats[2], (unsigned long long)tg_stats[3], (unsigned long long)tg_stats[4],
                    (unsigned long long)tg_stats[5], (unsigned long long)tg_stats[6], (unsigned long long)(tg_stats[7] & 0xFFFFFFFFull), (unsigned long long)(tg_stats[7] >> 32), n_raw, t_tg,
                    tg_ms[0] * 1e-3, tg_ms[1] * 1e-3);
    }
    return RUN;
}

// DART_COVERAGE: the sorted array still lies in HBM; the BAM and its index are complete and closed, and a failure here leaves them as they are
static int write_coverage(Job &job, Output &o)
{
    dg_ctx *root = job.roots[0];
    const double tc0 = now_s();
    size_t cov_entries = 0, cov_bytes = 0; float cov_ms = 0.f;
    for (const auto &t : job.cfg.cov_tracks) {
        size_t ne = 0, nb = 0; float ms = 0.f;
        int rc = dg_bam_coverage_finish(root, t.second, job.cfg.cov_exclude, job.cfg.cov_min_mapq, &ne, &nb, nullptr, &ms);
        std::vector<char> text(nb ? nb : 1);
        if (!rc) rc = dg_bam_coverage_download(root, nullptr, 0, text.data(), nb);
        if (rc) { abandon_outputs(job.cfg, o, AFTER_CLOSE); fprintf(stderr, "\nError! DART_COVERAGE=%d: %s\n", job.cfg.coverage, dg_last_error(root)); return 1; }
        FILE *cf = fopen(t.first.c_str(), "wb");
        const bool ok = cf && fwrite(text.data(), 1, nb, cf) == nb;
        if (!(cf && fclose(cf) == 0 && ok)) { abandon_outputs(job.cfg, o, AFTER_CLOSE); fprintf(stderr, "Error while writing %s\n", t.first.c_str()); return 1; }
        cov_entries += ne; cov_bytes += nb; cov_ms += ms;
    }
    if (job.cfg.timing)
        fprintf(stderr, "[dart timing] coverage: %zu tracks, %zu entries, %zu bytes; %.3f s (kernels %.3f s; exclude 0x%x, min mapq %u)\n", job.cfg.cov_tracks.size(), cov_entries, cov_bytes, now_s() - tc0,
                cov_ms * 1e-3, job.cfg.cov_exclude, job.cfg.cov_min_mapq);
    return RUN;
}

// DART_PILEUP: the variant-site table of the sorted (and, with DART_MARK_DUPLICATES, marked) array, which still lies in HBM; the BAM and its index are complete and
// closed, and a failure here leaves them as they are
static int write_pileup(Job &job, Output &o)
{
    dg_ctx *root = job.roots[0];
    const double tp0 = now_s();
    size_t ns = 0, nb = 0; float ms = 0.f; uint64_t st[10] = {0};
    int rc = dg_bam_pileup_finish(root, 0, job.cfg.pu_exclude, job.cfg.pu_min_mapq, job.cfg.pu_min_alt, &ns, &nb, st, &ms);
    std::vector<char> text(nb ? nb : 1);
    if (!rc) rc = dg_bam_pileup_download(root, nullptr, 0, text.data(), nb);
    if (rc) { abandon_outputs(job.cfg, o, AFTER_CLOSE); fprintf(stderr, "\nError! DART_PILEUP=1: %s\n", dg_last_error(root)); return 1; }
    static const char header[] = "#chr\tpos\tref\tdepth\tdepth_rev\tA\tC\tG\tT\tN\tDEL\tINS\tA_rev\tC_rev\tG_rev\tT_rev\tN_rev\tDEL_rev\tINS_rev\n";
    FILE *pf = fopen(job.cfg.sites_path.c_str(), "wb");
    const bool ok = pf && fwrite(header, 1, sizeof header - 1, pf) == sizeof header - 1 && fwrite(text.data(), 1, nb, pf) == nb;
    if (!(pf && fclose(pf) == 0 && ok)) { abandon_outputs(job.cfg, o, AFTER_CLOSE); fprintf(stderr, "Error while writing %s\n", job.cfg.sites_path.c_str()); return 1; }
    if (job.cfg.timing)
        fprintf(stderr, "[dart timing] pileup: %llu records, %llu mismatching and %llu deleted bases, %llu insertions; %llu sites, %zu kept, %zu bytes; %.3f s (kernels %.3f s; min alt %u, exclude 0x%x, min mapq %u)\n",
                (unsigned long long)st[0], (unsigned long long)st[3], (unsigned long long)st[4], (unsigned long long)st[5], (unsigned long long)st[6], ns, nb, now_s() - tp0, ms * 1e-3,
                job.cfg.pu_min_alt, job.cfg.pu_exclude, job.cfg.pu_min_mapq);
    return RUN;
}

// DART_QC: the QC tables of the sorted (and, with DART_MARK_DUPLICATES, marked) array, which still lies in HBM; the text is made on the host from the downloaded words.
// The BAM and its index are complete and closed, and a failure here leaves them as they are
static int write_qc(Job &job, const HostIndex &ix, Output &o)
{
    dg_ctx *root = job.roots[0];
    const double tq0 = now_s();
    size_t nw = 0, nb = 0; float ms = 0.f;
    int rc = dg_bam_qc_finish(root, 0, job.cfg.qc_exclude, job.cfg.qc_min_mapq, &nw, &ms);
    std::vector<uint64_t> words(nw ? nw : 1);
    if (!rc) rc = dg_bam_qc_download(root, words.data(), nw);
    if (rc) { abandon_outputs(job.cfg, o, AFTER_CLOSE); fprintf(stderr, "\nError! DART_QC=1: %s\n", dg_last_error(root)); return 1; }
    std::vector<const char *> names; std::vector<int64_t> lens;
    for (size_t k = 0; k < ix.names.size(); k++) { names.push_back(ix.names[k].c_str()); lens.push_back((int64_t)ix.len[k]); }
    std::vector<char> text(1);
    rc = dg_bam_qc_format(words.data(), nw, (int)names.size(), names.data(), lens.data(), nullptr, 0, &nb);
    if (rc == DG_ERR_CAPACITY) { text.resize(nb ? nb : 1); rc = dg_bam_qc_format(words.data(), nw, (int)names.size(), names.data(), lens.data(), text.data(), nb, &nb); }
    if (rc) { abandon_outputs(job.cfg, o, AFTER_CLOSE); fprintf(stderr, "\nError! DART_QC=1: the tables' text could not be made (%d)\n", rc); return 1; }
    FILE *qf = fopen(job.cfg.qc_path.c_str(), "wb");
    const bool ok = qf && fwrite(text.data(), 1, nb, qf) == nb;
    if (!(qf && fclose(qf) == 0 && ok)) { abandon_outputs(job.cfg, o, AFTER_CLOSE); fprintf(stderr, "Error while writing %s\n", job.cfg.qc_path.c_str()); return 1; }
    if (job.cfg.timing)
        fprintf(stderr, "[dart timing] qc: %zu words, %zu bytes; %.3f s (kernels %.3f s; exclude 0x%x, min mapq %u)\n", nw, nb, now_s() - tq0, ms * 1e-3, job.cfg.qc_exclude, job.cfg.qc_min_mapq);
    return RUN;
}

// DART_RNA_METRICS: the RNA-seq metrics of the sorted (and, with DART_MARK_DUPLICATES and DART_BAM_TAGS, marked and tagged) array, which still lies in HBM, against
// the annotation's transcripts; the text is made on the host from the downloaded words.  The BAM and its index are complete and closed, and a failure here
// leaves them as they are
static int write_rna_metrics(Job &job, Output &o)
{
    dg_ctx *root = job.roots[0];
    const double tr0 = now_s();
    size_t nw = 0, nb = 0; float ms = 0.f;
    int rc = dg_bam_rna_finish(root, 0, job.cfg.rna_exclude, job.cfg.rna_min_mapq, job.cfg.rna_min_cov, &nw, &ms);
    std::vector<uint64_t> words(nw ? nw : 1);
    if (!rc) rc = dg_bam_rna_download(root, words.data(), nw);
    if (rc) { abandon_outputs(job.cfg, o, AFTER_CLOSE); fprintf(stderr, "\nError! DART_RNA_METRICS=%s: %s\n", job.cfg.rna_gtf, dg_last_error(root)); return 1; }
    std::vector<char> text(1);
    rc = dg_bam_rna_format(words.data(), nw, nullptr, 0, &nb);
    if (rc == DG_ERR_CAPACITY) { text.resize(nb ? nb : 1); rc = dg_bam_rna_format(words.data(), nw, text.data(), nb, &nb); }
    if (rc) { abandon_outputs(job.cfg, o, AFTER_CLOSE); fprintf(stderr, "\nError! DART_RNA_METRICS=%s: the metrics' text could not be made (%d)\n", job.cfg.rna_gtf, rc); return 1; }
    FILE *rf = fopen(job.cfg.rna_path.c_str(), "wb");
    const bool ok = rf && fwrite(text.data(), 1, nb, rf) == nb;
    if (!(rf && fclose(rf) == 0 && ok)) { abandon_outputs(job.cfg, o, AFTER_CLOSE); fprintf(stderr, "Error while writing %s\n", job.cfg.rna_path.c_str()); return 1; }
    if (job.cfg.timing)
        fprintf(stderr, "[dart timing] rna metrics: %zu words, %zu bytes; %.3f s (kernels %.3f s; exclude 0x%x, min mapq %u, min cov %llu)\n", nw, nb, now_s() - tr0, ms * 1e-3, job.cfg.rna_exclude,
                job.cfg.rna_min_mapq, (unsigned long long)job.cfg.rna_min_cov);
    return RUN;
}

// DART_DEVICE_SJ: the clones' tables into their root's, further roots' into the first (downloaded entries, counted again there), then the table is sorted,
// mapped to chromosomes and printed on the device: the text is junctions.tab
struct SjTable { std::string text; size_t entries = 0, lines = 0; float finish_ms = 0.f; };
static int finish_junctions(Job &job, SjTable &sj)
{
    auto sj_fail = [&](dg_ctx *x) { fprintf(stderr, "\nError! junction table: %s\n", dg_last_error(x)); return 1; };
    for (size_t d = 0; d < job.roots.size(); d++)
        for (int k = 1; k < job.cfg.inflight; k++) if (dg_sj_merge(job.roots[d], job.ctx[d * (size_t)job.cfg.inflight + k])) return sj_fail(job.roots[d]);
    for (size_t d = 1; d < job.roots.size(); d++) {
        size_t ne = 0;
        if (dg_sj_finish(job.roots[d], DG_SJ_ENTRIES_ONLY, &ne, nullptr, nullptr, nullptr)) return sj_fail(job.roots[d]);
        std::vector<dg_sj_entry> ent(ne ? ne : 1);
        if (dg_sj_download(job.roots[d], ent.data(), ne, nullptr, 0)) return sj_fail(job.roots[d]);
        if (dg_sj_add(job.roots[0], ent.data(), ne)) return sj_fail(job.roots[0]);
    }
    size_t nb = 0;
    if (dg_sj_finish(job.roots[0], 0, &sj.entries, &sj.lines, &nb, &sj.finish_ms)) return sj_fail(job.roots[0]);
    sj.text.resize(nb);
    if (dg_sj_download(job.roots[0], nullptr, 0, nb ? &sj.text[0] : nullptr, nb)) return sj_fail(job.roots[0]);
    return RUN;
}

// DART_GENE_COUNTS: the clones' tables into their root's (dg_gene_merge), further roots' into the first (downloaded, folded in with dg_gene_add); the host
// prints the table
static int write_gene_table(Job &job, const GtfAnnotation &gtf, unsigned long long &gene_counted)
{
    auto gene_fail = [&](dg_ctx *x) { fprintf(stderr, "\nError! gene counts: %s\n", dg_last_error(x)); return 1; };
    const size_t n_rows = 4 + gtf.genes.size();
    std::vector<uint64_t> tab(n_rows * 3, 0);
    for (size_t d = 0; d < job.roots.size(); d++)
        for (int k = 1; k < job.cfg.inflight; k++) if (dg_gene_merge(job.roots[d], job.ctx[d * (size_t)job.cfg.inflight + k])) return gene_fail(job.roots[d]);
    for (size_t d = 1; d < job.roots.size(); d++) {
        if (dg_gene_download(job.roots[d], tab.data(), n_rows)) return gene_fail(job.roots[d]);
        if (dg_gene_add(job.roots[0], tab.data(), n_rows)) return gene_fail(job.roots[0]);
    }
    if (dg_gene_download(job.roots[0], tab.data(), n_rows)) return gene_fail(job.roots[0]);
    std::string text;
    static const char *const head[4] = {"N_unmapped", "N_multimapping", "N_noFeature", "N_ambiguous"};
    for (size_t r = 0; r < n_rows; r++) {
        text += r < 4 ? std::string(head[r]) : gtf.genes[r - 4];
        for (int col = 0; col < 3; col++) { text += '\t'; text += std::to_string((unsigned long long)tab[3 * r + col]); }
        text += '\n';
        if (r >= 4) gene_counted += tab[3 * r];
    }
    FILE *gf = fopen(job.cfg.genes_path.c_str(), "wb");
    const bool ok = gf && fwrite(text.data(), 1, text.size(), gf) == text.size();
    if (!(gf && fclose(gf) == 0 && ok)) { remove(job.cfg.genes_path.c_str()); fprintf(stderr, "Error while writing %s\n", job.cfg.genes_path.c_str()); return 1; }
    return RUN;
}

// DART_TX_QUANT: the clones' class tables into their root's (dg_tx_merge), further roots' into the first (downloaded, folded in with dg_tx_add), the EM on the
// first root (dg_tx_finish); the host prints <out>.transcripts.tab from the words (dg_tx_format).  summary: the 16 summary words, ms: the device times by part
static int write_tx_table(Job &job, const GtfTranscripts &txq, uint64_t summary[16], float ms[3])
{
    auto tx_fail = [&](dg_ctx *x) { fprintf(stderr, "\nError! DART_TX_QUANT=%s: %s\n", job.cfg.tx_gtf, dg_last_error(x)); return 1; };
    for (size_t d = 0; d < job.roots.size(); d++)
        for (int k = 1; k < job.cfg.inflight; k++) if (dg_tx_merge(job.roots[d], job.ctx[d * (size_t)job.cfg.inflight + k])) return tx_fail(job.roots[d]);
    for (size_t d = 1; d < job.roots.size(); d++) {
        size_t nc = 0, nm = 0;
        if (dg_tx_classes_size(job.roots[d], &nc, &nm)) return tx_fail(job.roots[d]);
        std::vector<uint64_t> off(nc + 1), cnt(nc + 1); std::vector<uint32_t> ids(nm + 1); uint64_t w8[8];
        if (dg_tx_classes_download(job.roots[d], off.data(), ids.data(), cnt.data(), nc, nm, w8)) return tx_fail(job.roots[d]);
        if (dg_tx_add(job.roots[0], off.data(), ids.data(), cnt.data(), nc, w8)) return tx_fail(job.roots[0]);
    }
    dg_ctx *root = job.roots[0];
    size_t nw = 0;
    if (dg_tx_finish(root, 0, job.cfg.tx_frag_mean, job.cfg.tx_max_rounds, &nw, nullptr)) return tx_fail(root);
    std::vector<uint64_t> words(nw);
    if (dg_tx_download(root, words.data(), nw) || dg_tx_device_ms(root, ms)) return tx_fail(root);
    memcpy(summary, words.data() + nw - 16, 16 * sizeof(uint64_t));
    dg_rna_annot ann; ann.n_tx = (uint32_t)txq.tx.size(); ann.pad = 0; ann.n_exons = txq.exons.size(); ann.tx = txq.tx.data(); ann.exons = txq.exons.data();
    std::vector<const char *> names;
    for (const std::string &n : txq.names) names.push_back(n.c_str());
    std::vector<char> text; size_t nb = 0;
    int rc = dg_tx_format(words.data(), nw, &ann, names.data(), nullptr, 0, &nb);
    if (rc == DG_ERR_CAPACITY) { text.resize(nb ? nb : 1); rc = dg_tx_format(words.data(), nw, &ann, names.data(), text.data(), nb, &nb); }
    if (rc) { fprintf(stderr, "\nError! DART_TX_QUANT=%s: the table's text could not be made (%d)\n", job.cfg.tx_gtf, rc); return 1; }
    FILE *tf = fopen(job.cfg.tx_path.c_str(), "wb");
    const bool ok = tf && fwrite(text.data(), 1, nb, tf) == nb;
    if (!(tf && fclose(tf) == 0 && ok)) { remove(job.cfg.tx_path.c_str()); fprintf(stderr, "Error while writing %s\n", job.cfg.tx_path.c_str()); return 1; }
    return RUN;
}

// DART_TRIM_*: the statistics of every upload, summed over batches and libraries, as key<TAB>value lines in the order of dg_batch_trim_stats
static int write_trim_stats(const Job &job)
{
    static const char *const key[14] = {"reads_in", "reads_kept", "bases_in", "bases_kept", "qual5_bases", "qual3_bases", "adapter0_reads", "adapter1_reads", "adapter_bases", "poly_reads",
                                        "poly_bases", "too_short_reads", "mate_dropped_reads", "qual_skipped_reads"};
    std::string text;
    for (int k = 0; k < 14; k++) { text += key[k]; text += '\t'; text += std::to_string(job.trim_stats[k].load()); text += '\n'; }
    if (job.cfg.umi) { text += "umi_bases\t" + std::to_string(job.trim_stats[14].load()) + "\numi_dropped_reads\t" + std::to_string(job.trim_stats[15].load()) + "\n"; }      // DART_UMI: the two sums of the cut
    FILE *tf = fopen(job.cfg.trim_path.c_str(), "wb");
    const bool ok = tf && fwrite(text.data(), 1, text.size(), tf) == text.size();
    if (!(tf && fclose(tf) == 0 && ok)) { remove(job.cfg.trim_path.c_str()); fprintf(stderr, "Error while writing %s\n", job.cfg.trim_path.c_str()); return 1; }
    return RUN;
}

// Mapping.cpp:812-822 and OutputSpliceJunctions, Mapping.cpp:683-716
static void print_summary(const Job &job, const HostIndex &ix, const SjTable &sj)
{
    const long long T = job.total.total, U = job.total.unmapped;
    if (job.pair_end) fprintf(stdout, "\t# of total mapped reads = %lld (sensitivity = %.2f%%)\n\t# of paired sequences = %lld (%.2f%%)\n", T - U, (int)(10000 * (1.0 * (T - U) / T) + 0.5) / 100.0, job.total.paired, (int)(10000 * (1.0 * job.total.paired / T) + 0.5) / 100.0);
    else fprintf(stdout, "\t# of total mapped reads = %lld (sensitivity = %.2f%%)\n", T - U, (int)(10000 * (1.0 * (T - U) / T) + 0.5) / 100.0);
    fprintf(stdout, "\t# of unique mapped reads = %lld (%.2f%%)\n", job.total.unique, (int)(10000 * (1.0 * job.total.unique / T) + 0.5) / 100.0);
    if (!job.cfg.unique) fprintf(stdout, "\t# of multiple mapped reads = %lld (%.2f%%)\n", T - U - job.total.unique, (int)(10000 * (1.0 * (T - U - job.total.unique) / T) + 0.5) / 100.0);
    fprintf(stdout, "\t# of unmapped reads = %lld (%.2f%%)\n", U, (int)(10000 * (1.0 * U / T) + 0.5) / 100.0);
    FILE *jf = fopen(job.cfg.sj, "w");
    int nj = 0;
    const int nc = (int)ix.names.size();
    std::vector<int64_t> key(2 * nc); std::vector<int> who(2 * nc);
    for (int i = 0; i < nc; i++) { key[i] = ix.off[i] + ix.len[i] - 1; who[i] = i; key[2 * nc - 1 - i] = 2 * ix.l_pac - ix.off[i] - 1; who[2 * nc - 1 - i] = i; }
    if (job.cfg.device_sj) { if (jf) fwrite(sj.text.data(), 1, sj.text.size(), jf); nj = (int)sj.lines; }
    else for (auto &kv : job.sjmap) {
        const int lo = (int)(std::lower_bound(key.begin(), key.end(), kv.first.first) - key.begin());
        if (lo >= 2 * nc) continue;
        const int x = who[lo];
        if (jf) fprintf(jf, "%s\t%lld\t%lld\t%d\n", ix.names[x].c_str(), (long long)(kv.first.first + 1 - ix.off[x]), (long long)(kv.first.second + 1 - ix.off[x]), kv.second);
        nj++;
    }
    if (jf) fclose(jf);
    fprintf(stdout, "\t# of splice junctions = %d (file: %s)\n", nj, job.cfg.sj);
    fprintf(stdout, "\tAlignment output: %s\n\n", job.cfg.out);
}

// The HIP runtime maps the streams of a process onto GPU_MAX_HW_QUEUES hardware queues (its default 4) and reads the variable when it
// initialises.  The contexts in flight need a queue each (+ the copy stream, + this program's own, + two spare = 16: INTEGRATION.md 2): a
// value that is missing, unparsable or lower is raised to that, a higher one stays.  libdartgpu's load-time constructor does the same;
// a program that is linked against another build of the library still gets it from here.
static const int HW_QUEUES_NEED = 16;          // (never above 32)
static void ensure_hw_queues()
{
    const char *v = getenv("GPU_MAX_HW_QUEUES");
    char *end = nullptr;
    const long have = v ? strtol(v, &end, 10) : 0;
    if (!v || end == v || *end || have < HW_QUEUES_NEED) setenv("GPU_MAX_HW_QUEUES", std::to_string(HW_QUEUES_NEED).c_str(), 1);
}

int main(int argc, char *argv[])
{
    ensure_hw_queues();                        // before the first HIP call
    if (argc > 1 && strcmp(argv[1], "update") == 0) {          // main.cpp:120-124 runs git and make: not something a library drop-in does
        fprintf(stderr, "dart (MI355X): the 'update' sub-command is outside this build's scope\n");
        return 0;
    }
    if (argc > 1 && strcmp(argv[1], "index") == 0) {           // main.cpp:125-132
        if (argc == 4) return index_cmd::run(argv[0], argv[2], argv[3]);
        fprintf(stderr, "usage: %s index ref.fa prefix\n", argv[0]);
        return 0;
    }
    Config cfg;
    dg_params defaults;
    dg_params_default(&defaults);
    int rc = cfg.parse(argc, argv, [](const char *k) -> const char * { return getenv(k); }, defaults, stdout, stderr);
    if (rc != RUN) return rc;
    setenv("DG_BLOCKING_SYNC", "1", 0);      // the mapping threads sleep while their batch is on the GPU instead of spinning: the CPU share belongs to the parser, the formatter and the writer
    const double t_proc0 = now_s();
    Job job(cfg);
    Output out;
    LibPlan first;                          // library 0's head start
    first.look(cfg, 0);
    // what the first candidate can begin now: index the plain files, or inflate the .gz files whole (inflation on the device maps its files when its turn comes)
    const bool whole = first.choice.gz_whole;
    if (!first.choice.gz_device && (whole || first.choice.plain)) first.pre.start(cfg.f1[0].c_str(), cfg.two_files() ? cfg.f2[0].c_str() : nullptr, cfg.threads, whole, whole ? cfg.gz_whole_max : 0);
    // every device of the node maps batches (reads shard, the index is replicated; the reference's -t threads over one shared index,
    // Mapping.cpp:792-793); DART_GPUS=n restricts it to the first n
    int n_gpu = dg_device_count();
    if (n_gpu < 1) { fprintf(stderr, "Error! No HIP device (this build of dart has no CPU path)\n"); return 1; }
    if (cfg.has_gpus) n_gpu = std::min(std::max(1, cfg.gpus), n_gpu);      // (HIP_VISIBLE_DEVICES picks WHICH devices; a job of a few million reads is done before a second device has its index)
    if (cfg.same_device_times) n_gpu = cfg.same_device_times;
    if (cfg.sort_bam && n_gpu > 1) { fprintf(stderr, "DART_SORT_BAM=1: the sorted store lives on one device; 1 of %d devices is used\n", n_gpu); n_gpu = 1; }
    if (first.choice.head_pool) job.pool.start((size_t)n_gpu * cfg.inflight + 2, cfg.batch_reads, 160, cfg.pinned);
    else if (cfg.index && file_exists(std::string(cfg.index) + ".ann")) first.io = open_lib(cfg, 0, first.m1, first.mate2(cfg), first.choice);      // (a whole-file .gz library that turns out not to qualify opens its streams late: rare)
    HostIndex ix;
    if (!cfg.index || !file_exists(std::string(cfg.index) + ".ann") || !file_exists(std::string(cfg.index) + ".amb") || !file_exists(std::string(cfg.index) + ".pac")) {
        fprintf(stderr, "Error! Please specify a valid reference index!\n"); cfg.usage(stdout, argv[0]); return 1;
    }
    fprintf(stdout, "Load the genome index files...");
    if (!load_ann(cfg.index, ix)) { fprintf(stderr, "\n\nError! Index files are corrupt!\n"); return 0; }
    // DART_GENE_COUNTS: a GTF that cannot be used ends the run here, before a context exists and before any output is begun; no failed run leaves a table, a stale one included.
    GtfAnnotation gtf;
    if (cfg.gene_gtf) {
        remove(cfg.genes_path.c_str());
        const std::string gerr = gtf_parse(cfg.gene_gtf, ix.names, cfg.gene_feature, gtf);
        if (!gerr.empty()) { fprintf(stderr, "\nError! DART_GENE_COUNTS=%s: %s\n", cfg.gene_gtf, gerr.c_str()); return 1; }
        if (gtf.skipped_seq || gtf.skipped_strand)
            fprintf(stderr, "DART_GENE_COUNTS: skipped %zu '%s' lines on sequences the index lacks and %zu with a strand other than + or -\n", gtf.skipped_seq, cfg.gene_feature, gtf.skipped_strand);
    }
    // DART_RNA_METRICS: the same for its GTF
    GtfTranscripts rna;
    if (cfg.rna_gtf) {
        remove(cfg.rna_path.c_str());
        const std::string rerr = gtf_parse_transcripts(cfg.rna_gtf, ix.names, rna);
        if (!rerr.empty()) { fprintf(stderr, "\nError! DART_RNA_METRICS=%s: %s\n", cfg.rna_gtf, rerr.c_str()); return 1; }
        if (rna.skipped_seq || rna.skipped_strand)
            fprintf(stderr, "DART_RNA_METRICS: skipped %zu lines on sequences the index lacks and %zu with a strand other than + or -\n", rna.skipped_seq, rna.skipped_strand);
    }
    // DART_TX_QUANT: and for its GTF; no failed run leaves a table, a stale one included
    GtfTranscripts txq;
    if (cfg.tx_gtf) {
        remove(cfg.tx_path.c_str());
        const std::string terr = gtf_parse_transcripts(cfg.tx_gtf, ix.names, txq);
        if (!terr.empty()) { fprintf(stderr, "\nError! DART_TX_QUANT=%s: %s\n", cfg.tx_gtf, terr.c_str()); return 1; }
        if (txq.skipped_seq || txq.skipped_strand)
            fprintf(stderr, "DART_TX_QUANT: skipped %zu lines on sequences the index lacks and %zu with a strand other than + or -\n", txq.skipped_seq, txq.skipped_strand);
    }
    if (cfg.cuts()) remove(cfg.trim_path.c_str());      // (no failed run leaves a table, a stale one included)
    if ((rc = make_contexts(job, ix, gtf, rna, txq, n_gpu)) != RUN) return rc;
    job.start_up_s = now_s() - t_proc0;
    fprintf(stdout, "\nLoad the reference sequences...\n");
    if ((rc = open_output(job, ix, out)) != RUN) return rc;
    job.t0 = time(NULL);
    if (cfg.silent) fprintf(stdout, "Start read mapping...\n");
    if ((rc = run_library(job, out, 0, first)) != RUN) return rc;
    for (size_t lib = 1; lib < cfg.f1.size(); lib++) {
        LibPlan next;
        next.look(cfg, lib);
        if ((rc = run_library(job, out, lib, next)) != RUN) return rc;
    }
    if (!cfg.silent) fprintf(stdout, "\rAll the %lld %s reads have been processed in %lld seconds.\n", job.total.total, job.pair_end ? "paired-end" : "single-end", (long long)(time(NULL) - job.t0));
    if (cfg.sort_bam && (rc = finish_sorted_bam(job, out)) != RUN) return rc;
    if (cfg.bam) { if (!out.bam.close()) { abandon_outputs(cfg, out, CLOSE_FAILED); fprintf(stderr, "Error while writing %s\n", cfg.out); return 1; } }
    else fclose(out.sam);
    if (cfg.coverage && (rc = write_coverage(job, out)) != RUN) return rc;
    if (cfg.pileup && (rc = write_pileup(job, out)) != RUN) return rc;
    if (cfg.qc && (rc = write_qc(job, ix, out)) != RUN) return rc;
    if (cfg.rna_gtf && (rc = write_rna_metrics(job, out)) != RUN) return rc;
    SjTable sj;
    if (cfg.device_sj && (rc = finish_junctions(job, sj)) != RUN) return rc;
    unsigned long long gene_counted = 0;
    if (cfg.gene_gtf && (rc = write_gene_table(job, gtf, gene_counted)) != RUN) return rc;
    uint64_t tx_summary[16] = {0}; float tx_ms[3] = {0.f, 0.f, 0.f};
    if (cfg.tx_gtf && (rc = write_tx_table(job, txq, tx_summary, tx_ms)) != RUN) return rc;
    if (cfg.cuts() && (rc = write_trim_stats(job)) != RUN) return rc;
    for (auto x : job.clones) dg_destroy(x);
    for (auto x : job.roots) dg_destroy(x);
    if (job.total.total > 0) print_summary(job, ix, sj);
    if (cfg.timing && cfg.tx_gtf) {
        fprintf(stderr, "[dart timing] tx:");
        for (int k = 0; k < 16; k++) fprintf(stderr, " %s=%llu", dg_tx_word_name(k), (unsigned long long)tx_summary[k]);
        fprintf(stderr, " acc_ms=%.3f compat_ms=%.3f classes_ms=%.3f em_ms=%.3f\n", job.tx_acc_ns.load() * 1e-6, (double)tx_ms[0], (double)tx_ms[1], (double)tx_ms[2]);
    }
    if (cfg.timing && cfg.cuts())
        fprintf(stderr, "[dart trim] reads_in=%llu reads_kept=%llu bases_in=%llu bases_kept=%llu kernels_ms=%.3f\n", job.trim_stats[0].load(), job.trim_stats[1].load(), job.trim_stats[2].load(),
                job.trim_stats[3].load(), job.trim_kernel_us.load() * 1e-3);
    if (cfg.timing && cfg.gene_gtf)
        fprintf(stderr, "[dart genes] table=device units=%llu counted=%llu genes=%zu acc_ms=%.3f min_mapq=%u\n", (unsigned long long)job.gene_units.load(), gene_counted, gtf.genes.size(), job.gene_acc_ns.load() * 1e-6, cfg.gene_min_mapq);
    if (cfg.timing) {
        if (cfg.device_sj) fprintf(stderr, "[dart sj] table=device tuples=%llu entries=%zu accumulate_ms=%.3f finish_ms=%.3f\n", (unsigned long long)job.sj_tuples.load(), sj.entries, job.sj_acc_ns.load() * 1e-6, (double)sj.finish_ms);
        else fprintf(stderr, "[dart sj] table=host tuples=%llu entries=%zu map_s=%.6f\n", (unsigned long long)job.sj_tuples.load(), job.sjmap.size(), job.sj_map_ns.load() * 1e-9);
    }
    return 0;
}
