// dart_amd/csrc/host/fast_fastq.h -- the host side of `dart` for plain (uncompressed) FASTQ input, built for throughput:
// the reference reads, maps and prints under two global locks (GetData.cpp:134-179 under LibraryLock, Mapping.cpp:644-664 under
// OutputLock); with the mapping at hundreds of millions of reads per second those two serial sections are everything.
//
//   index pass     the input files are memory-mapped; T threads count the newlines of their share (pass A), then walk the lines
//                  of their share with the exact line number known (pass B): every fourth line starts a record.  No heuristics
//                  about '@': a record is four lines, as GetNextEntry (GetData.cpp:77-132) reads them.
//   assembly       per batch, T threads copy the bases into a page-locked arena (mate 2 reverse-complemented as GetData.cpp:157-166
//                  does) -- headers and qualities are never copied, the formatter reads them from the mapping
//   mapping        dg_map_batch on the batch's arena, one thread per context
//   format + write T threads format contiguous read ranges into their own buffers, the ranges' sizes give their file offsets,
//                  and the same threads pwrite() them: SAM bytes in input order without a serial writer
// The record semantics (header trimming, "an entry without bases ends the stream", qualities cut to the read length, the
// 4000-read / 1 000 000-base chunking that decides which reads of an odd-sized tail are mapped unpaired) are those of the
// reference's reader and of the streaming path in dart_main.cpp; tests/test_gpu_cli.py runs both paths against the oracle's
// command line.
#pragma once
#include <functional>
#include <atomic>
#include <cerrno>
#include <fcntl.h>
#include <sys/mman.h>
#include "libdeflate_dl.h"
#include <unistd.h>
#include "dart_config.h"

// (libdeflate_dl.h: the system's libdeflate when it is there; it has no streaming interface, so a .gz file's output must fit a buffer: open_gz below)
struct MappedFile {
    const char *p = nullptr; size_t n = 0; int fd = -1;
    size_t cap = 0;                                   // > 0: p is an anonymous mapping of cap bytes holding an inflated file
    // A .gz file, inflated whole into memory (every member, as gzread concatenates them).  false = not possible here (no libdeflate, larger than
    // max_out, not a clean gzip file): the caller takes the streaming reader, which has gzread's behaviour for whatever this is.
    // What this process may still take: MemAvailable, and what the cgroup (v2, then v1) leaves -- a container's limit is not in /proc/meminfo.  0 = unknown.
    static size_t memory_left() {
        size_t avail = 0;
        if (FILE *f = fopen("/proc/meminfo", "r")) {
            char line[256];
            while (fgets(line, sizeof line, f)) { unsigned long long kb; if (sscanf(line, "MemAvailable: %llu kB", &kb) == 1) { avail = (size_t)kb << 10; break; } }
            fclose(f);
        }
        if (!avail) { const long pg = sysconf(_SC_AVPHYS_PAGES), sz = sysconf(_SC_PAGESIZE); if (pg > 0 && sz > 0) avail = (size_t)pg * (size_t)sz; }
        auto read_u64 = [](const char *path, unsigned long long &v) { FILE *f = fopen(path, "r"); if (!f) return false; const bool ok = fscanf(f, "%llu", &v) == 1; fclose(f); return ok; };
        unsigned long long lim = 0, cur = 0;
        if ((read_u64("/sys/fs/cgroup/memory.max", lim) && read_u64("/sys/fs/cgroup/memory.current", cur)) ||
            (read_u64("/sys/fs/cgroup/memory/memory.limit_in_bytes", lim) && read_u64("/sys/fs/cgroup/memory/memory.usage_in_bytes", cur))) {
            const size_t room = lim > cur ? (size_t)(lim - cur) : 0;
            if (lim < (1ull << 60) && (!avail || room < avail)) avail = room;
        }
        return avail;
    }
    // A .gz file, inflated whole into memory (every member, as gzread concatenates them).  false = not possible here (no libdeflate, larger than
    // max_out or than a third of the memory this process may still take -- both mates are inflated at once and the batch buffers come on top; the
    // streaming reader runs such a job in constant memory --, not a clean gzip file): the caller takes the streaming reader, which has gzread's
    // behaviour for whatever this is.  The mapping grows in place (mremap) and the inflate goes on with the member that did not fit: the last
    // member's ISIZE is only a first guess (multi-member and bgzip files), and starting over doubled the work each time.
    bool open_gz(const char *fn, size_t max_out) {
        const LibDeflate &ld = lib_deflate();
        if (!ld.ok()) return false;          // (DART_GZ_STREAM=1, always the streaming reader, is choose_pipelines' business: such a job never comes here)
        MappedFile z;
        if (!z.open(fn) || z.n < 18 || (unsigned char)z.p[0] != 0x1f || (unsigned char)z.p[1] != 0x8b) return false;
        { const size_t left = memory_left(); if (left && left / 3 < max_out) max_out = left / 3; }
        uint32_t isize; memcpy(&isize, z.p + z.n - 4, 4);                       // the last member's size mod 2^32: the first guess
        size_t want = std::max<size_t>((size_t)isize + 64, z.n * 4);
        if (want > max_out) return false;
        void *d = ld.alloc();
        if (!d) return false;
        void *m = mmap(nullptr, want, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) { ld.release(d); return false; }
        size_t in_at = 0, out_at = 0; int rc = 0;
        while (in_at < z.n) {
            if (z.n - in_at < 18 || (unsigned char)z.p[in_at] != 0x1f || (unsigned char)z.p[in_at + 1] != 0x8b) { rc = 1; break; }    // bytes behind the last member: gzread's business
            size_t used = 0, made = 0;
            rc = ld.gunzip(d, z.p + in_at, z.n - in_at, (char *)m + out_at, want - out_at, &used, &made);
            if (rc == 3) {                                                      // LIBDEFLATE_INSUFFICIENT_SPACE: this member again, into a larger mapping (what the earlier members gave stays)
                const size_t bigger = want * 2;
                if (bigger > max_out) break;
                void *m2 = mremap(m, want, bigger, MREMAP_MAYMOVE);
                if (m2 == MAP_FAILED) break;
                m = m2; want = bigger; rc = 0;
                continue;
            }
            if (rc) break;
            in_at += used; out_at += made;
        }
        ld.release(d);
        if (rc != 0 || in_at < z.n) { munmap(m, want); return false; }
        p = (const char *)m; n = out_at; cap = want;
        return true;
    }
    bool open(const char *fn) {
        fd = ::open(fn, O_RDONLY);
        if (fd < 0) return false;
        struct stat st; if (fstat(fd, &st) != 0) return false;
        n = (size_t)st.st_size;
        if (n == 0) { p = ""; return true; }
        void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) return false;
        madvise(m, n, MADV_SEQUENTIAL);
        p = (const char *)m;
        return true;
    }
    void close_now() { if (p && (cap || n)) munmap((void *)p, cap ? cap : n); if (fd >= 0) ::close(fd); p = nullptr; n = cap = 0; fd = -1; }
    ~MappedFile() { close_now(); }
};

// one FASTQ record: byte offset of its header line and the lengths of its four lines INCLUDING the newline (0 = the line does
// not exist: end of file)
struct FqRec { uint64_t off; uint32_t l0, l1, l2, l3; };

template <class F>
static void parallel_for(int nt, F f)
{
    if (nt <= 1) { f(0); return; }
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back([&f, t]() { f(t); });
    f(0);
    for (auto &x : th) x.join();
}

// the records of a mapped FASTQ file, in file order; *has_empty: some record has no bases (such an entry ends a chunk of the
// reference's reader, GetData.cpp:141,154: the caller then replays the chunking)
static void index_fastq(const MappedFile &mf, int nt, std::vector<FqRec> &recs, bool *has_empty, size_t min_share = (size_t)1 << 20)
{
    recs.clear(); *has_empty = false;
    const char *p = mf.p; const size_t n = mf.n;
    if (n == 0) return;
    nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)nt, n / min_share + 1));
    std::vector<size_t> cut(nt + 1), nl(nt + 1, 0);
    for (int k = 0; k <= nt; k++) cut[k] = n / nt * k;
    cut[nt] = n;
    parallel_for(nt, [&](int k) {                       // pass A: newlines per share
        size_t c = 0;
        for (const char *q = p + cut[k], *e = p + cut[k + 1]; q < e;) { const char *f = (const char *)memchr(q, '\n', e - q); if (!f) break; c++; q = f + 1; }
        nl[k + 1] = c;
    });
    for (int k = 0; k < nt; k++) nl[k + 1] += nl[k];    // newlines before each share
    std::vector<std::vector<FqRec>> part(nt);
    auto line_len = [&](size_t at) -> uint32_t {        // length of the line that starts at `at`, newline included; 0 past the end
        if (at >= n) return 0;
        const char *f = (const char *)memchr(p + at, '\n', n - at);
        return (uint32_t)(f ? (size_t)(f - (p + at)) + 1 : n - at);
    };
    parallel_for(nt, [&](int k) {                       // pass B: the records whose header line starts in this share
        const size_t c0 = cut[k], c1 = cut[k + 1];
        // a line starts at 0 and behind every newline; its number = the newlines before it.  First start in [c0, c1):
        size_t pos, line;
        if (c0 == 0) { pos = 0; line = 0; }
        else if (p[c0 - 1] == '\n') { pos = c0; line = nl[k]; }
        else { const char *f = (const char *)memchr(p + c0, '\n', n - c0); if (!f) return; pos = (size_t)(f - p) + 1; line = nl[k] + 1; }
        part[k].reserve((c1 - c0) / 200 + 16);
        while (pos < c1 && pos < n) {
            if (line & 3) { const uint32_t l = line_len(pos); pos += l; line++; if (l == 0) break; continue; }
            FqRec r; r.off = pos;
            r.l0 = line_len(pos); r.l1 = line_len(pos + r.l0); r.l2 = line_len(pos + r.l0 + r.l1); r.l3 = line_len(pos + r.l0 + r.l1 + r.l2);
            part[k].push_back(r);
            pos += (size_t)r.l0 + r.l1 + r.l2 + r.l3; line += 4;
            if (r.l3 == 0) break;                       // the file ended inside this record
        }
    });
    size_t total = 0;
    for (auto &v : part) total += v.size();
    recs.reserve(total);
    for (auto &v : part)
        for (const FqRec &r : v) {
            if ((int)r.l1 - 1 <= 0) *has_empty = true;           // rlen = line length - 1 (GetData.cpp:103)
            recs.push_back(r);
        }
}

// One read as the formatter sees it.  The STORED read (what ReadItem_t holds, GetData.cpp:140-166) is s[0..sl) and q[0..ql) as they
// are in the file, or -- rc: mate 2 of a pair -- the reverse complement (non-ACGT -> N) of s and the reversed q.
struct RView { const char *h; const char *s; const char *q; uint32_t hl, sl, ql; bool rc; };

static inline char comp_base_f(char c)   // tools.cpp:3-17
{
    switch (c) { case 'A': case 'a': return 'T'; case 'C': case 'c': return 'G'; case 'G': case 'g': return 'C'; case 'T': case 't': return 'A'; default: return 'N'; }
}

#define PUT_LIT(out, lit) (out).put(lit, sizeof(lit) - 1)

// complement tables: COMP1 = comp_base_f, COMP2 = comp_base_f applied twice (canonical upper-case base, or N)
struct CompTables { unsigned char c1[256], c2[256]; CompTables() { for (int i = 0; i < 256; i++) { c1[i] = (unsigned char)comp_base_f((char)i); c2[i] = (unsigned char)comp_base_f(comp_base_f((char)i)); } } };
static const CompTables g_comp;

// ---- byte-string kernels of the formatter: reversed copy and reverse-complement copy, 32 bytes at a time where the CPU has AVX2 ----
#include <immintrin.h>
__attribute__((target("avx2"))) static void rev_copy_avx2(char *d, const char *s, size_t l)
{
    const __m256i idx = _mm256_setr_epi8(15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0);
    size_t i = 0;
    for (; i + 32 <= l; i += 32) {
        __m256i v = _mm256_loadu_si256((const __m256i *)(s + l - 32 - i));
        v = _mm256_permute2x128_si256(_mm256_shuffle_epi8(v, idx), _mm256_shuffle_epi8(v, idx), 1);
        _mm256_storeu_si256((__m256i *)(d + i), v);
    }
    for (; i < l; i++) d[i] = s[l - 1 - i];
}
// comp_base_f on 32 bytes: A/a -> T, C/c -> G, G/g -> C, T/t -> A, anything else -> N
__attribute__((target("avx2"))) static inline __m256i comp32_avx2(__m256i v)
{
    const __m256i lo = _mm256_or_si256(v, _mm256_set1_epi8(0x20));
    __m256i r = _mm256_set1_epi8('N');
    r = _mm256_blendv_epi8(r, _mm256_set1_epi8('T'), _mm256_cmpeq_epi8(lo, _mm256_set1_epi8('a')));
    r = _mm256_blendv_epi8(r, _mm256_set1_epi8('G'), _mm256_cmpeq_epi8(lo, _mm256_set1_epi8('c')));
    r = _mm256_blendv_epi8(r, _mm256_set1_epi8('C'), _mm256_cmpeq_epi8(lo, _mm256_set1_epi8('g')));
    r = _mm256_blendv_epi8(r, _mm256_set1_epi8('A'), _mm256_cmpeq_epi8(lo, _mm256_set1_epi8('t')));
    return r;
}
__attribute__((target("avx2"))) static void revcomp_copy_avx2(char *d, const char *s, size_t l)
{
    const __m256i idx = _mm256_setr_epi8(15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0);
    size_t i = 0;
    for (; i + 32 <= l; i += 32) {
        __m256i v = comp32_avx2(_mm256_loadu_si256((const __m256i *)(s + l - 32 - i)));
        v = _mm256_shuffle_epi8(v, idx);
        _mm256_storeu_si256((__m256i *)(d + i), _mm256_permute2x128_si256(v, v, 1));
    }
    for (; i < l; i++) d[i] = (char)g_comp.c1[(unsigned char)s[l - 1 - i]];
}
__attribute__((target("avx2"))) static void comp2_copy_avx2(char *d, const char *s, size_t l)     // comp_base_f twice: the canonical base, or N
{
    size_t i = 0;
    for (; i + 32 <= l; i += 32) _mm256_storeu_si256((__m256i *)(d + i), comp32_avx2(comp32_avx2(_mm256_loadu_si256((const __m256i *)(s + i)))));
    for (; i < l; i++) d[i] = (char)g_comp.c2[(unsigned char)s[i]];
}
static const bool g_avx2 = __builtin_cpu_supports("avx2");
static const char g_digits2[201] = "00010203040506070809101112131415161718192021222324252627282930313233343536373839404142434445464748495051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";

// (one per formatter thread, side by side in a vector: each on cache lines of its own -- `n` is written with every field, and neighbours that
//  shared a line made thirteen threads format slower than one: 890 ns per read and thread against 50, profiles/r03/g_formatter_false_sharing.txt)
struct alignas(128) TextBuf {
    char *b = nullptr; size_t n = 0, cap = 0;
    ~TextBuf() { free(b); }
    inline void need(size_t more) { if (n + more > cap) { cap = std::max(cap * 2, n + more + (1 << 16)); b = (char *)realloc(b, cap); } }
    inline void put(const char *s, size_t l) { memcpy(b + n, s, l); n += l; }
    inline void ch(char c) { b[n++] = c; }
    inline void put_rev(const char *s, size_t l) {                          // s reversed
        char *d = b + n;
        if (g_avx2) rev_copy_avx2(d, s, l); else for (size_t i = 0; i < l; i++) d[i] = s[l - 1 - i];
        n += l;
    }
    inline void put_comp2(const char *s, size_t l) {                        // comp(comp(s))
        char *d = b + n;
        if (g_avx2) comp2_copy_avx2(d, s, l); else for (size_t i = 0; i < l; i++) d[i] = (char)g_comp.c2[(unsigned char)s[i]];
        n += l;
    }
    inline void put_revcomp(const char *s, size_t l) {                      // reverse complement (non-ACGT -> N)
        char *d = b + n;
        if (g_avx2) revcomp_copy_avx2(d, s, l); else for (size_t i = 0; i < l; i++) d[i] = (char)g_comp.c1[(unsigned char)s[l - 1 - i]];
        n += l;
    }
    inline void num(long long v) {                                          // decimal, two digits per step
        char t[24]; int k = 24;
        unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
        while (u >= 100) { const unsigned r = (unsigned)(u % 100); u /= 100; k -= 2; t[k] = g_digits2[2 * r]; t[k + 1] = g_digits2[2 * r + 1]; }
        if (u >= 10) { k -= 2; t[k] = g_digits2[2 * u]; t[k + 1] = g_digits2[2 * u + 1]; } else t[--k] = (char)('0' + u);
        if (v < 0) b[n++] = '-';
        memcpy(b + n, t + k, (size_t)(24 - k)); n += (size_t)(24 - k);
    }
};

struct alignas(128) Counters { long long total = 0, unique = 0, unmapped = 0, paired = 0; };

// OutputPairedAlignments / OutputSingledAlignments (Mapping.cpp:208-369) for reads [lo,hi) of a batch.
// names/name_len: chromosome names; n_pair_mode: reads below this index are mates of pairs (2i, 2i+1).
static void format_views(const RView *V, int lo, int hi, int n_pair_mode, const dg_read_out *ro, const dg_report_out *po, const uint32_t *cig,
                         const std::vector<std::string> &names, bool unique_only, bool multi, bool fastq, TextBuf &out, Counters &ct)
{
    static const char *XS_A[3] = { "", " XS:A:+", " XS:A:-" };
    static const size_t XS_L[3] = { 0, 7, 7 };
    for (int k = lo; k < hi; k++) {
        const bool is_pair = k < n_pair_mode, mate2 = is_pair && (k & 1);
        const RView &e = V[k];
        // the reference prints the stored quality as a C string: it ends at a NUL byte, if there is one
        uint32_t ql = e.ql;
        if (ql && memchr(e.q, 0, ql)) { uint32_t z = 0; while (z < ql && (e.rc ? e.q[ql - 1 - z] : e.q[z]) != 0) z++; ql = z; }
        const dg_read_out &r = ro[k];
        const dg_report_out *rp = po + r.rep_off;
        auto put_stored_seq = [&]() { if (e.rc) out.put_revcomp(e.s, e.sl); else out.put(e.s, e.sl); };
        auto put_stored_qual = [&]() { if (e.rc) out.put_rev(e.q + (e.ql - ql), ql); else out.put(e.q, ql); };
        if (r.score == 0) {
            ct.unmapped++;
            out.need(e.hl + e.sl + ql + 96);
            out.put(e.h, e.hl); out.ch('\t'); out.num(rp[0].flag); PUT_LIT(out, "\t*\t0\t0\t*\t*\t0\t0\t"); put_stored_seq(); out.ch('\t');
            if (fastq) put_stored_qual(); else out.ch('*');
            PUT_LIT(out, "\tAS:i:0\tXS:i:0\n");
            continue;
        }
        if (!(!unique_only || r.mapq > 3)) continue;
        if (r.mapq == 50) ct.unique++;
        const dg_read_out *m = is_pair ? &ro[k ^ 1] : nullptr;
        const dg_report_out *mp = m ? po + m->rep_off : nullptr;
        for (int j = r.best; j < r.n_rep; j++) {
            const dg_report_out &pr = rp[j];
            const bool show = is_pair ? pr.aln_score > 0 : pr.aln_score == r.score;
            if (show) {
                int xs;
                if (pr.sj_type == -1) xs = 0; else if (pr.sj_type == 0 || pr.sj_type == 2) xs = mate2 ? 2 : 1; else xs = mate2 ? 1 : 2;
                const bool use_alt = mate2 ? pr.bdir == 1 : pr.bdir == 0;      // print the reverse complement of the stored read
                const std::string &cn = names[pr.chr];
                int pj;
                out.need(e.hl + cn.size() + e.sl + ql + 16 * (size_t)pr.n_cigar + 192);
                out.put(e.h, e.hl);
                out.ch('\t'); out.num(pr.flag); out.ch('\t'); out.put(cn.data(), cn.size()); out.ch('\t'); out.num((long long)pr.pos); out.ch('\t'); out.num(r.mapq); out.ch('\t');
                for (uint32_t c = 0; c < pr.n_cigar; c++) { const uint32_t op = cig[pr.cigar_off + c]; out.num(op >> 4); out.ch("MIDNS"[op & 15]); }
                if (is_pair && (pj = pr.paired_idx) != -1 && mp[pj].aln_score > 0) {
                    const dg_report_out &a = mate2 ? mp[pj] : pr, &b = mate2 ? pr : mp[pj];
                    const int l1 = mate2 ? (int)V[k ^ 1].sl : (int)e.sl, l2 = mate2 ? (int)e.sl : (int)V[k ^ 1].sl;
                    int dist = (int)(b.pos - a.pos + (a.bdir ? l2 : 0 - l1));
                    if (mate2) dist = 0 - dist; else if (j == r.best) ct.paired += 2;
                    PUT_LIT(out, "\t=\t"); out.num((long long)mp[pj].pos); out.ch('\t'); out.num(dist); out.ch('\t');
                } else PUT_LIT(out, "\t*\t0\t0\t");
                if (!use_alt) put_stored_seq();
                else if (e.rc) out.put_comp2(e.s, e.sl);                          // revcomp of the stored revcomp
                else out.put_revcomp(e.s, e.sl);
                out.ch('\t');
                if (!fastq) out.ch('*');
                else if (!use_alt) put_stored_qual();
                else if (e.rc) out.put(e.q + (e.ql - ql), ql);                  // the stored qualities reversed = the file's (the last ql of them)
                else out.put_rev(e.q, ql);
                PUT_LIT(out, "\tNM:i:"); out.num(r.mis_num); PUT_LIT(out, "\tAS:i:"); out.num(r.score); PUT_LIT(out, "\tXS:i:"); out.num(r.sub_score);
                out.put(XS_A[xs], XS_L[xs]); out.ch('\n');
                if (!is_pair && !multi) break;
            }
            if (is_pair && !multi) break;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the pipeline
// ---------------------------------------------------------------------------------------------
static int hdr_beg(const char *s, int len) { for (int i = 1; i < len; i++) if (s[i] != '>' && s[i] != '@') return i; return len - 1; }
static int hdr_end(const char *s, int len) { for (int i = 1; i < len; i++) if (s[i] == ' ' || s[i] == '/' || s[i] == '\t') return i; return len - 1; }

static inline void rev_copy(char *d, const char *s, size_t l) { if (g_avx2) rev_copy_avx2(d, s, l); else for (size_t i = 0; i < l; i++) d[i] = s[l - 1 - i]; }

// the program's one clock (monotonic)
static inline unsigned long long now_ns() { return (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static inline double now_s() { return (double)now_ns() * 1e-9; }

struct FastSlot {                       // one batch travelling through the stages
    size_t first = 0; int n = 0, odd = 0; size_t seqno = 0;
    std::vector<uint32_t> hoff, qoff; char *names_quals = nullptr; size_t nq_cap = 0;      // device formatter: the batch's names and stored qualities, flat
    char *text = nullptr; size_t text_cap = 0, text_n = 0; uint64_t dev_ct[3] = {0, 0, 0}, bam_rr[2] = {0, 0}; //  its text (or BGZF blocks) and counters; BAM: records written, lines refused
    std::vector<RView> view; std::vector<uint32_t> soff; std::vector<uint16_t> rl;
    char *seq = nullptr; size_t seq_cap = 0, n_cap = 0;            // page-locked
    dg_read_out *ro = nullptr; dg_report_out *po = nullptr; uint32_t *cig = nullptr; dg_sj_out *sj = nullptr; size_t caps[3] = {0, 0, 0}, used[3] = {0, 0, 0};
    const char *fq1 = nullptr, *fq2 = nullptr; size_t fq_n1 = 0, fq_n2 = 0; bool fq_device = false;      // device parser: the batch's byte range of each mapped file
    int gz_chunk = -1;                  // DART_DEVICE_GZ: the ranges are whole BGZF blocks of the compressed files, chunk gz_chunk of the library's plan
    int rc = 0; std::string err;
};

struct FastStats { double t_index = 0, t_asm = 0, t_map = 0, t_fmt = 0, t_write = 0, t_alloc = 0, t_gather = 0, t_dev_call = 0, t_dev_kernels = 0, t_download = 0; size_t n_batches = 0;
                   bool gz_device = false; double t_gz_check = 0, t_gz_tail = 0;      // the library's .gz files were inflated on the device: the check pass / waiting for and downloading the tails
                   bool fq_device = false; double t_fq_call = 0, t_fq_kernels = 0; };      // the library's batches were parsed on the device: dg_batch_upload_fastq, sum over workers / its kernels

// Batch arenas: ordinary memory by default -- page-locking costs ~1 s per GB, more than a short job saves; DART_PINNED=1 page-locks them
// (then the copies to and from the GPU are plain DMA transfers: worth it for long runs with several contexts in flight)
// The batch slots and their arenas; with DART_PINNED=1 they are page-locked in the background while the index loads.  (The switch counts when the pool is
// started, which is when the first library looks like the parallel pipeline's: a pool that a later library is the first to use has ordinary memory.)
struct SlotPool {
    std::vector<FastSlot> slots; std::thread th; bool pinned = false;
    void *alloc(size_t bytes) const { return pinned ? dg_host_alloc(bytes) : malloc(bytes ? bytes : 1); }
    void release(void *p) const { if (!p) return; if (pinned) dg_host_free(p); else free(p); }
    void reserve(FastSlot &s, size_t n, size_t bases, const size_t need[3]) const {
        if (bases + 64 > s.seq_cap) { release(s.seq); s.seq_cap = bases + bases / 8 + 4096; s.seq = (char *)alloc(s.seq_cap); }
        const size_t want[3] = { std::max(need[0], n * 2 + 1024), std::max(need[1], n * 6 + 4096), std::max(need[2], n + 1024) };
        if (!s.ro || s.n_cap < n || s.caps[0] < want[0] || s.caps[1] < want[1] || s.caps[2] < want[2]) {
            release(s.ro); release(s.po); release(s.cig); release(s.sj);
            s.n_cap = n + 16;
            s.ro = (dg_read_out *)alloc(s.n_cap * sizeof(dg_read_out)); s.po = (dg_report_out *)alloc(want[0] * sizeof(dg_report_out));
            s.cig = (uint32_t *)alloc(want[1] * 4); s.sj = (dg_sj_out *)alloc(want[2] * sizeof(dg_sj_out));
            s.caps[0] = want[0]; s.caps[1] = want[1]; s.caps[2] = want[2];
        }
    }
    // text: the slot's room for the device formatter's output
    void reserve_text(FastSlot &s, size_t nb) const { if (nb > s.text_cap) { release(s.text); s.text_cap = nb + nb / 8 + 4096; s.text = (char *)alloc(s.text_cap); } }
    void start(size_t n_slots, size_t batch_reads, size_t bytes_per_read, bool page_locked) {
        pinned = page_locked;
        slots.resize(n_slots);
        if (pinned) th = std::thread([this, batch_reads, bytes_per_read]() { const size_t z[3] = {0, 0, 0}; for (auto &s : slots) reserve(s, batch_reads, batch_reads * bytes_per_read, z); });
    }
    void wait() { if (th.joinable()) th.join(); }
    ~SlotPool() { wait(); for (auto &s : slots) { release(s.seq); release(s.ro); release(s.po); release(s.cig); release(s.sj); release(s.names_quals); release(s.text); } }
};

// One run of the program: what was asked (Config), the device contexts, and everything that lives across its libraries.  main owns it and hands it to both
// pipelines -- the parallel one below and the streaming one in dart_main.cpp -- and to the stages behind them.  What the switches mean to a batch:
//   cfg.device_sam     the SAM text of a batch is formatted on the GPU (dg_batch_format_sam) right behind its mapping, on the same context, and downloaded into
//                      the slot; format_views is not run
//   cfg.device_fastq   a batch goes to the GPU as the bytes of its records, straight from the mapped files (dg_batch_upload_fastq): no arena, no base copy on the
//                      host; with device_sam as well the text is formatted from the names and qualities that upload left in HBM (dg_batch_format_sam_resident)
//                      and nothing is gathered.  The index pass still decides the batches.  A library with a record without bases keeps the host's assembly
//   cfg.trim           every mapping thread sets the DART_TRIM_* switches on its context (dg_set_trim) for the library, and the upload cuts adapters, poly tails and
//                      low-quality ends and drops what became too short: the batch's read count is from then on what the upload returned, not what the index
//                      pass planned, and the statistics of every upload are summed into trim_stats.  Needs device_fastq and a device formatter (Config refuses the
//                      job otherwise); a library that falls back to the host's assembly is refused here
//   cfg.device_bam     the batch's BAM records are written and compressed on the GPU (dg_batch_format_bam, or its resident form with device_fastq) behind its
//                      mapping; the slot holds whole BGZF blocks and the ordered writer hands them to bam_sink (BamWriter::add_bgzf_blocks) instead of writing
//                      text to sam_fd.  cfg.bgzf_dynamic: the blocks are coded with dynamic Huffman codes per strip (DG_BAM_DYNAMIC): a smaller file of the same records
//   cfg.sort_bam       a batch's records are left uncompressed (DG_BAM_RAW) and appended to its context's store in HBM (dg_batch_accumulate_bam) under the batch's
//                      index counted across libraries; nothing is downloaded, the ordered writer only sums the counters.  The sorted-BAM stage merges the
//                      stores, sorts and writes the file at the end of the job
//   cfg.device_sj      every mapping thread counts its batch's junction tuples in its context's table on the GPU (sj_accumulate) right behind the mapping; the
//                      tuples are not downloaded and the ordered writer's map loop does not run.  The junction stage merges the tables and prints junctions.tab
//                      from the device's text at the end of the job
//   cfg.gene_gtf       every mapping thread counts its batch's units per gene in its context's table on the GPU (gene_accumulate) right behind the mapping, where
//                      sj_accumulate sits: mates are still neighbours there.  The gene stage merges the tables and prints <out>.genes.tab at the end of the job
//   cfg.tx_gtf         likewise its units into its context's class table (tx_accumulate); the expression stage merges the tables, runs the EM and prints
//                      <out>.transcripts.tab at the end of the job
struct Job {
    const Config &cfg;
    std::vector<dg_ctx *> ctx, roots, clones;             // ctx: all contexts, device by device, each root followed by its clones
    std::vector<std::string> names;                       // chromosome names
    bool pair_end;                                        // -p, or a library of two files has been seen
    Counters total;
    std::map<std::pair<int64_t, int64_t>, int> sjmap;     // the host's junction table (without cfg.device_sj)
    time_t t0 = 0;                                        // mapping began (the progress lines count from it)
    double start_up_s = 0;                                // process start to contexts ready: the start-up field of the `[dart timing]` lines
    SlotPool pool;                                       // batch slots of the parallel pipeline
    std::function<bool(const char *blocks, size_t n, long long records, long long refused)> bam_sink;
    int sam_fd = -1; uint64_t sam_off = 0;                // the parallel pipeline's place in the SAM file: descriptor and offset (advanced), set around each library
    size_t sort_ordinal_base = 0;                         // cfg.sort_bam: batches of the libraries before the current one
    // accounting for the `[dart timing]`, `[dart sj]` and `[dart genes]` lines: time in dg_batch_accumulate_bam; junction tuples seen, time in the accumulate
    // calls, time in the writer's map loop; units counted per gene, time in the accumulate calls
    std::atomic<unsigned long long> sort_acc_ns{0}, sj_tuples{0}, sj_acc_ns{0}, sj_map_ns{0}, gene_units{0}, gene_acc_ns{0}, tx_units{0}, tx_acc_ns{0};
    std::atomic<unsigned long long> trim_stats[16] = {}, trim_kernel_us{0};      // cfg.trim: dg_batch_trim_stats summed over batches and libraries; the trimming kernels' device time
    explicit Job(const Config &c) : cfg(c), pair_end(c.pair_end) {}
};

// A batch is in the output: its reads into the total, its junction tuples into the host's table (UpdateLocal/GlobalSJMap, Mapping.cpp:532-577; not with
// cfg.device_sj, where they never left the device), the progress line.  Both pipelines' ordered writers call it.
static void batch_written(Job &job, long long n_reads, const dg_sj_out *sj, size_t n_sj)
{
    job.total.total += n_reads;
    if (!job.cfg.device_sj) {
        const unsigned long long tj = now_ns();
        for (size_t k = 0; k < n_sj; k++) job.sjmap[std::make_pair(sj[k].g1, sj[k].g2)]++;
        job.sj_map_ns += now_ns() - tj; job.sj_tuples += n_sj;
    }
    if (!job.cfg.silent) { fprintf(stdout, "\r%lld %s tags have been processed in %lld seconds...", job.total.total, job.pair_end ? "paired-end" : "singled-end", (long long)(time(NULL) - job.t0)); fflush(stdout); }
}

// the tuples of the batch that ctx has just mapped into its table
static inline int sj_accumulate(Job &job, dg_ctx *ctx)
{
    const unsigned long long t = now_ns();
    size_t n = 0;
    const int rc = dg_batch_accumulate_sj(ctx, &n);
    job.sj_acc_ns += now_ns() - t; job.sj_tuples += n;
    return rc;
}
// likewise its units per gene
static inline int gene_accumulate(Job &job, dg_ctx *ctx, int n_pair_mode)
{
    const unsigned long long t = now_ns();
    size_t n = 0;
    const int rc = dg_batch_accumulate_genes(ctx, n_pair_mode, job.cfg.gene_min_mapq, &n);
    job.gene_acc_ns += now_ns() - t; job.gene_units += n;
    return rc;
}

// and its units into its class table (DART_TX_QUANT)
static inline int tx_accumulate(Job &job, dg_ctx *ctx, int n_pair_mode)
{
    const unsigned long long t = now_ns();
    size_t n = 0;
    const int rc = dg_batch_accumulate_tx(ctx, n_pair_mode, Config::tx_min_mapq, job.cfg.tx_strand, &n);
    job.tx_acc_ns += now_ns() - t; job.tx_units += n;
    return rc;
}

// The mapped read files of a library and the positions of their records.  The host program starts this for its first library before it
// loads the genome index and calls dg_init, so the two overlap (0.2 s per 16 M reads of the 1.6 s a job of that size takes).
// Would the reference's gz reader (gzGetNextEntry, GetData.cpp:181-210: gzgets into 1024 bytes, strlen) see these records as its plain reader
// (GetNextEntry, :77-132: getline) does?  Yes when every record has its four lines, none of them reaches 1024 bytes or holds a NUL, every header
// line begins with '@' and names something, and no entry is without bases.  Anything else goes through the streaming reader, which restates gzgets.
static bool gz_reader_sees_the_same(const MappedFile &mf, const std::vector<FqRec> &recs, int nt)
{
    if (mf.n && memchr(mf.p, 0, mf.n)) return false;
    std::atomic<bool> same(true);
    parallel_for(std::max(1, nt), [&](int k) {
        const size_t a = recs.size() * (size_t)k / (size_t)std::max(1, nt), b = recs.size() * (size_t)(k + 1) / (size_t)std::max(1, nt);
        for (size_t i = a; i < b && same.load(std::memory_order_relaxed); i++) {
            const FqRec &r = recs[i];
            bool good = r.l0 >= 2 && r.l1 >= 2 && r.l2 >= 1 && r.l3 >= 1 && r.l0 < 1024 && r.l1 < 1024 && r.l2 < 1024 && r.l3 < 1024 && mf.p[r.off] == '@';
            if (good) {                                     // IdentifyHeaderBegPos / EndPos (:55-75): the name must not be empty (:194)
                const char *h = mf.p + r.off; const int len = (int)r.l0;
                int p1 = len - 1, p2 = len - 1;
                for (int q = 0; q < len; q++) if (h[q] != '>' && h[q] != '@') { p1 = q; break; }
                for (int q = 1; q < len; q++) if (h[q] == ' ' || h[q] == '/' || h[q] == '\t') { p2 = q; break; }
                good = p2 - p1 > 0;
            }
            if (!good) same.store(false, std::memory_order_relaxed);
        }
    });
    return same.load();
}

struct FastqIndex {
    MappedFile m1, m2; std::vector<FqRec> r1, r2; bool e1 = false, e2 = false, ok = false, two = false; double t_index = 0;
    std::string f1, f2; std::thread th;
    // gz: the files are .gz and are inflated whole first (MappedFile::open_gz); ok then also says that the plain pipeline reads them as the gz reader would
    void run(const char *a, const char *b, int T, bool gz = false, size_t max_out = 0) {
        const double t = now_s();
        f1 = a; f2 = b ? b : ""; two = b != nullptr;
        if (gz) {
            bool ok2 = true;
            if (b) { std::thread t2([&]() { ok2 = m2.open_gz(b, max_out); }); ok = m1.open_gz(a, max_out); t2.join(); ok = ok && ok2; }
            else ok = m1.open_gz(a, max_out);
        } else ok = m1.open(a) && (!b || m2.open(b));
        if (ok) {
            if (b) { std::thread t2([&]() { index_fastq(m2, std::max(1, T / 2), r2, &e2); }); index_fastq(m1, std::max(1, T - T / 2), r1, &e1); t2.join(); }
            else index_fastq(m1, T, r1, &e1);
        }
        if (ok && gz) ok = !e1 && !e2 && gz_reader_sees_the_same(m1, r1, T) && (!b || gz_reader_sees_the_same(m2, r2, T));
        if (!ok && gz) { m1.close_now(); m2.close_now(); r1.clear(); r2.clear(); r1.shrink_to_fit(); r2.shrink_to_fit(); }
        t_index = now_s() - t;
    }
    void start(const char *a, const char *b, int T, bool gz = false, size_t max_out = 0) { f1 = a; f2 = b ? b : ""; th = std::thread([this, a, b, T, gz, max_out]() { run(a, b, T, gz, max_out); }); }
    void wait() { if (th.joinable()) th.join(); }
    ~FastqIndex() { wait(); }
};

// DART_DEVICE_GZ=1: a library of BGZF-compressed FASTQ files goes to the GPU as it lies on the disk (dg_batch_upload_fastq_bgzf): the files are mapped,
// cut into chunks of whole blocks (by the blocks' ISIZE, to about a batch of reads), and every chunk is inflated and parsed in HBM.  Blocks do not end where
// records end: what lies behind a chunk's last whole record (its tail) is downloaded and goes in front of the next chunk, so the uploads are ordered.
// The plan is made by a first pass over all chunks with DG_FQ_CHECK_ONLY: it finds a corrupt block, and a record the reference's gz reader would read in its
// own way, before a byte of output exists -- such a library takes the host's path -- and it leaves every chunk's number of reads.
struct GzDevPlan {
    struct Member { size_t off; uint32_t bsize, isize; };
    struct Chunk { size_t a1, b1, a2, b2; int n_reads; bool last; };
    MappedFile m1, m2; bool two = false;
    std::vector<Chunk> chunks; size_t total_reads = 0; double t_check = 0;
    // the mapping pass: whose turn it is to upload, and the tails the turn before left
    std::mutex mu; std::condition_variable cv; size_t turn = 0; std::vector<char> tail1, tail2;

    // the members of a mapped file; false: not BGZF all the way (the library's own walk will say the same)
    static bool members(const MappedFile &mf, std::vector<Member> &out) {
        const unsigned char *p = (const unsigned char *)mf.p;
        for (size_t at = 0; at < mf.n;) {
            if (mf.n - at < 12 || p[at] != 0x1f || p[at + 1] != 0x8b || p[at + 2] != 8 || p[at + 3] != 4) return false;
            const size_t xlen = (size_t)p[at + 10] | (size_t)p[at + 11] << 8;
            if (mf.n - at - 12 < xlen) return false;
            size_t bsize = 0;
            for (size_t x = at + 12, xe = at + 12 + xlen; x + 4 <= xe;) {
                const size_t slen = (size_t)p[x + 2] | (size_t)p[x + 3] << 8;
                if (xe - x - 4 < slen) break;
                if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2) { bsize = ((size_t)p[x + 4] | (size_t)p[x + 5] << 8) + 1; break; }
                x += 4 + slen;
            }
            if (!bsize || bsize > mf.n - at || bsize < 12 + xlen + 8) return false;
            uint32_t isize; memcpy(&isize, p + at + bsize - 4, 4);
            if (isize > 65536) return false;
            out.push_back(Member{at, (uint32_t)bsize, isize});
            at += bsize;
        }
        return true;
    }
    // one chunk through the library; the tails replace the heads
    static int upload(dg_ctx *c, const GzDevPlan &P, const Chunk &k, std::vector<char> &h1, std::vector<char> &h2, bool pair_end, int max_reads, uint32_t flags, int *n, uint64_t *unlike) {
        dg_fastq_bgzf in;
        in.head1 = h1.data(); in.n_head1 = h1.size(); in.blocks1 = P.m1.p + k.a1; in.n_blocks1 = k.b1 - k.a1;
        in.head2 = P.two ? h2.data() : nullptr; in.n_head2 = P.two ? h2.size() : 0; in.blocks2 = P.two ? P.m2.p + k.a2 : nullptr; in.n_blocks2 = P.two ? k.b2 - k.a2 : 0;
        in.rc_odd_reads = pair_end ? 1 : 0; in.max_reads = max_reads; in.last = k.last ? 1 : 0;
        size_t tail[2] = {0, 0};
        int rc = dg_batch_upload_fastq_bgzf(c, &in, flags, n, tail, unlike);
        if (rc) return rc;
        std::vector<char> t1(tail[0] + 1), t2(tail[1] + 1);
        rc = dg_batch_download_fastq_tail(c, t1.data(), tail[0], t2.data(), tail[1]);
        if (rc) return rc;
        t1.resize(tail[0]); t2.resize(tail[1]); h1.swap(t1); h2.swap(t2);
        return 0;
    }
    // false: the library is not one for this path (the caller takes the host's, silently)
    bool make(const char *f1, const char *f2, bool pair_end, size_t batch_reads, dg_ctx *c) {
        const double t = now_s();
        two = f2 != nullptr;
        if (pair_end && !two) return false;                   // (interlaced pairs: a chunk would have to end on an even record)
        if (!m1.open(f1) || (two && !m2.open(f2))) return false;
        std::vector<Member> M1, M2;
        if (!members(m1, M1) || (two && !members(m2, M2)) || M1.empty() || (two && M2.empty())) return false;
        const size_t target = std::max<size_t>(1, two ? batch_reads / 2 : batch_reads);      // records of each text per chunk
        double bpr1 = 125, bpr2 = 125;                        // bytes per record: a first guess, then what the last chunk had
        std::vector<char> h1, h2;
        for (size_t i1 = 0, i2 = 0; i1 < M1.size() || i2 < M2.size();) {
            size_t j1 = i1, j2 = i2, sum1 = 0, sum2 = 0;
            while (j1 < M1.size() && (double)sum1 < (double)target * bpr1) sum1 += M1[j1++].isize;
            while (j2 < M2.size() && (double)sum2 < (double)target * bpr2) sum2 += M2[j2++].isize;
            if (h1.size() + sum1 >= 0xFFFFFF00ull || h2.size() + sum2 >= 0xFFFFFF00ull) return false;
            Chunk k;
            k.a1 = i1 < M1.size() ? M1[i1].off : m1.n; k.b1 = j1 < M1.size() ? M1[j1].off : m1.n;
            k.a2 = i2 < M2.size() ? M2[i2].off : m2.n; k.b2 = j2 < M2.size() ? M2[j2].off : m2.n;
            k.last = j1 == M1.size() && j2 == M2.size(); k.n_reads = 0;
            const size_t in1 = h1.size() + sum1, in2 = h2.size() + sum2;
            uint64_t unlike = 0;
            const size_t room = (in1 + in2) / 4 + 2;
            if (upload(c, *this, k, h1, h2, pair_end, (int)std::min<size_t>(room, 0x7FFFFFFF), DG_FQ_CHECK_ONLY, &k.n_reads, &unlike) != 0 || unlike) return false;
            if (pair_end && (k.n_reads & 1)) return false;    // (an unpaired tail is the host's business)
            const size_t rec = two ? (size_t)(k.n_reads + 1) / 2 : (size_t)k.n_reads;
            if (rec) { bpr1 = std::max(16.0, (double)(in1 - h1.size()) / (double)rec); if (two && k.n_reads > 1) bpr2 = std::max(16.0, (double)(in2 - h2.size()) / (double)(k.n_reads / 2)); }
            chunks.push_back(k); total_reads += (size_t)k.n_reads;
            i1 = j1; i2 = j2;
        }
        t_check = now_s() - t;
        return !chunks.empty();
    }
};

// Maps one library of plain FASTQ files.  f2 == nullptr: one file (single-end, or interlaced pairs when pair_end).
// gzp: the library is BGZF-compressed and gzp holds its plan (DART_DEVICE_GZ): the batches are the plan's chunks, inflated and parsed on the device.
// pre: the caller's index of this library, if it made one beside dg_init (or inflated the .gz files whole).
// Returns 0, or the failing dg status (message in err).  SAM text goes to job.sam_fd at job.sam_off (advanced).
static int run_fast_library(Job &job, const char *f1, const char *f2, FastqIndex *pre, GzDevPlan *gzp, FastStats &st, std::string &err)
{
    const Config &c = job.cfg;
    const bool pair_end = job.pair_end;
    size_t batch_reads = c.batch_reads;
    const int T = std::max(1, c.threads);
    // T is the budget of ALL stages (the GPU boxes grant a CPU quota, not cores: more runnable threads than the quota means the whole process is
    // throttled): the formatter takes what the writer (TWR threads), the assembler and the mapping threads leave.  DART_FMT_THREADS / DART_WRITE_THREADS override.
    // (ONE writer: pwrites to one file serialise on its inode lock, and two threads taking turns at it are slower than one that keeps it --
    //  write 0.78 s against 1.4-1.6 s per 16 M reads on tmpfs, profiles/r03/g_formatter_false_sharing.txt)
    const int TWR = c.write_threads;
    const int TF = c.fmt_threads ? c.fmt_threads : std::max(1, T - TWR - 1);
    const bool use_mmap = c.write_mmap;
    FastqIndex own;                                   // (unless the caller has indexed this library already, beside dg_init)
    if (gzp) pre = &own;                              // (no record index: the host never sees the text)
    else {
        if (pre) pre->wait();
        if (!pre || pre->f1 != f1 || pre->f2 != (f2 ? f2 : "")) { pre = &own; own.run(f1, f2, T); }
        if (!pre->ok) { err = "cannot map the read files"; return DG_ERR_ARG; }
    }
    MappedFile &m1 = pre->m1, &m2 = pre->m2;
    std::vector<FqRec> &r1 = pre->r1, &r2 = pre->r2;
    const bool e1 = pre->e1, e2 = pre->e2;
    st.t_index += pre->t_index;
    // The reads in input order, as GetNextChunk (GetData.cpp:134-179) hands them out: from separate files r1[i], r2[i] alternate (the
    // stream ends with the shorter file, one read of file 1 more if it is the longer); from one file its records in order.
    // An entry without bases ends the reader's current chunk (it is consumed), a chunk without reads ends the stream, and a chunk with
    // an odd number of reads is mapped unpaired (Mapping.cpp:598) and ends the stream here (as in the streaming path of dart_main.cpp).
    // Without such entries the order is implicit; with them the chunking is replayed once to list the reads explicitly.
    std::vector<uint64_t> order;                       // (record index << 1) | file; used only when an entry without bases exists
    const bool explicit_order = e1 || e2;
    size_t n_total, odd_from;
    auto len_of = [&](const std::vector<FqRec> &v, size_t i) -> long long { return (long long)v[i].l1 - 1; };
    if (!explicit_order) {
        n_total = f2 ? (r1.size() > r2.size() ? 2 * r2.size() + 1 : 2 * r1.size()) : r1.size();
        odd_from = n_total;
        if (pair_end && (n_total & 1)) {               // only the last chunk can be odd: find where it starts
            size_t k = 0, start = 0; int count = 0; long long base = 0;
            auto rl_at = [&](size_t q) { return f2 ? len_of((q & 1) ? r2 : r1, q >> 1) : len_of(r1, q); };
            while (k < n_total) {
                base += rl_at(k); count++; k++;
                if (k >= n_total) break;
                base += rl_at(k); count++; k++;
                if (count == 4000 || base > 1000000) { start = k; count = 0; base = 0; }
            }
            odd_from = start;
        }
    } else {
        size_t p1 = 0, p2 = 0;                         // next record of file 1 / file 2
        odd_from = (size_t)-1;
        while (true) {
            const size_t chunk_start = order.size();
            int count = 0; long long base = 0;
            while (true) {
                if (p1 >= r1.size()) break;
                if (len_of(r1, p1) <= 0) { p1++; break; }
                order.push_back(((uint64_t)p1 << 1) | 0u); base += len_of(r1, p1); count++; p1++;
                std::vector<FqRec> &v2 = f2 ? r2 : r1; size_t &q = f2 ? p2 : p1;
                if (q >= v2.size()) break;
                if (len_of(v2, q) <= 0) { q++; break; }
                order.push_back(((uint64_t)q << 1) | (f2 ? 1u : 0u)); base += len_of(v2, q); count++; q++;
                if (count == 4000 || base > 1000000) break;
            }
            if (count == 0) break;
            if (count & 1) { if (pair_end) odd_from = chunk_start; break; }
        }
        n_total = order.size();
        if (odd_from == (size_t)-1) odd_from = n_total;
    }
    auto rec_of = [&](size_t k, const MappedFile *&mf) -> const FqRec & {
        if (explicit_order) { const uint64_t e = order[k]; mf = (e & 1) ? &m2 : &m1; return (e & 1) ? r2[e >> 1] : r1[e >> 1]; }
        if (f2) { mf = (k & 1) ? &m2 : &m1; return (k & 1) ? r2[k >> 1] : r1[k >> 1]; }
        mf = &m1; return r1[k];
    };
    // read k as the formatter sees it: name, bases and qualities where they lie in the mapping, nothing copied
    auto view_of = [&](size_t k) {
        const MappedFile *mf; const FqRec &r = rec_of(k, mf);
        const char *l0 = mf->p + r.off, *l1 = l0 + r.l0, *l3 = l1 + r.l1 + r.l2;
        const int p1 = hdr_beg(l0, (int)r.l0), p2 = hdr_end(l0, (int)r.l0);
        RView v;
        v.h = l0 + p1; v.hl = p2 > p1 ? (uint32_t)(p2 - p1) : 0u;
        v.s = l1; v.sl = r.l1 - 1;
        v.q = l3; v.ql = std::min<uint32_t>(v.sl, r.l3);                 // qualities cut to the read length (GetData.cpp:118-121)
        v.rc = pair_end && (k & 1);                                      // mate 2 is stored reverse-complemented (also in an unpaired tail)
        return v;
    };
    if (gzp) { n_total = gzp->total_reads; odd_from = n_total; st.gz_device = true; st.t_gz_check += gzp->t_check; }
    if (batch_reads & 1) batch_reads++;
    const bool fq_device = gzp || (c.device_fastq && !explicit_order);      // (an entry without bases ends a chunk: the replayed order is not a byte range)
    st.fq_device = fq_device;
    if (c.cuts() && !fq_device) { err = "DART_TRIM_* / DART_UMI: this library falls back to the host's assembly (a record without bases), where nothing is trimmed"; return DG_ERR_ARG; }
    // the bytes of records [a, b) of a mapped file
    auto byte_range = [](const MappedFile &mf, const std::vector<FqRec> &v, size_t a, size_t b, const char *&p, size_t &n) {
        const size_t lo = a < v.size() ? (size_t)v[a].off : mf.n, hi = b < v.size() ? (size_t)v[b].off : mf.n;
        p = mf.p + lo; n = hi - lo;
    };
    // slots + queues
    job.pool.wait();
    if (job.pool.slots.size() < job.ctx.size() + 2) job.pool.slots.resize(job.ctx.size() + 2);
    std::vector<FastSlot> &slots = job.pool.slots;
    std::mutex mu; std::condition_variable cv;
    std::deque<FastSlot *> free_q, map_q; std::map<size_t, FastSlot *> fmt_q;
    for (auto &s : slots) free_q.push_back(&s);
    bool asm_done = false, failed = false; size_t mappers_left = job.ctx.size();
    int fail_rc = 0;

    std::thread assembler([&]() {
        size_t next = 0, seqno = 0;
        for (size_t ci = 0; gzp && ci < gzp->chunks.size(); ci++) {      // DART_DEVICE_GZ: a batch is a chunk of the plan
            FastSlot *s;
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return !free_q.empty() || failed; }); if (failed) break; s = free_q.front(); free_q.pop_front(); }
            const double ta = now_s();
            const int n = gzp->chunks[ci].n_reads;
            s->first = next; s->n = n; s->odd = 0; s->seqno = seqno++; s->rc = 0; s->fq_device = true; s->gz_chunk = (int)ci;
            { const double tl = now_s(); const size_t z[3] = {0, 0, 0}; job.pool.reserve(*s, (size_t)n, 0, z); st.t_alloc += now_s() - tl; }
            st.t_asm += now_s() - ta;
            next += (size_t)n;
            { std::lock_guard<std::mutex> lk(mu); map_q.push_back(s); }
            cv.notify_all();
        }
        while (!gzp && next < n_total) {
            FastSlot *s;
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return !free_q.empty() || failed; }); if (failed) break; s = free_q.front(); free_q.pop_front(); }
            const double ta = now_s();
            // a batch ends at the start of the unpaired tail, which is a batch of its own
            size_t end = std::min(n_total, next + batch_reads);
            int odd = 0;
            if (next < odd_from && end > odd_from) end = odd_from;
            if (next >= odd_from) { end = n_total; odd = (int)(end - next); }
            const int n = (int)(end - next);
            s->first = next; s->n = n; s->odd = odd; s->seqno = seqno++; s->rc = 0; s->fq_device = fq_device; s->gz_chunk = -1;
            if (fq_device) {
                // the batch is a byte range of each file (next is even: batches and the start of an unpaired tail are); the host keeps views for its
                // formatter only -- names, bases and qualities where they lie in the mapping, nothing copied
                s->fq2 = nullptr; s->fq_n2 = 0;
                if (f2) { byte_range(m1, r1, next / 2, (end + 1) / 2, s->fq1, s->fq_n1); byte_range(m2, r2, next / 2, end / 2, s->fq2, s->fq_n2); }
                else byte_range(m1, r1, next, end, s->fq1, s->fq_n1);
                if (s->fq_n1 >= 0xFFFFFF00ull || s->fq_n2 >= 0xFFFFFF00ull) { s->rc = DG_ERR_ARG; s->err = "a batch's FASTQ text exceeds 32-bit offsets: lower DART_BATCH"; }
                else {
                    { const double tl = now_s(); const size_t z[3] = {0, 0, 0}; job.pool.reserve(*s, (size_t)n, 0, z); st.t_alloc += now_s() - tl; }
                    if (!c.device_sam && !c.device_bam) {
                        s->view.resize(n);
                        const int TA = std::max(1, T / 8);
                        parallel_for(TA, [&](int tid) {
                            const int lo = (int)((long long)n * tid / TA), hi = (int)((long long)n * (tid + 1) / TA);
                            for (int k = lo; k < hi; k++) s->view[k] = view_of(next + k);
                        });
                    }
                }
                st.t_asm += now_s() - ta;
                next = end;
                { std::lock_guard<std::mutex> lk(mu); map_q.push_back(s); }
                cv.notify_all();
                continue;
            }
            s->view.resize(n); s->soff.resize((size_t)n + 1); s->rl.resize(n);
            size_t bases = 0;
            bool too_long = false;
            for (int k = 0; k < n; k++) {               // offsets: sequential (one add per read)
                const MappedFile *mf; const FqRec &r = rec_of(next + k, mf);
                const uint32_t rlen = r.l1 - 1;
                s->soff[k] = (uint32_t)bases; bases += rlen;
                if (rlen > DG_MAX_RLEN) too_long = true;
                s->rl[k] = (uint16_t)rlen;
            }
            s->soff[n] = (uint32_t)bases;
            if (too_long || bases > 0xFFFFFF00ull) { s->rc = DG_ERR_ARG; s->err = "read longer than DG_MAX_RLEN"; }
            else {
                { const double tl = now_s(); const size_t z[3] = {0, 0, 0}; job.pool.reserve(*s, (size_t)n, bases, z); st.t_alloc += now_s() - tl; }
                const int TA = std::max(1, T / 8);              // (copying bases is a tenth of the formatter's work; T is the budget of ALL stages)
                parallel_for(TA, [&](int tid) {
                    const int lo = (int)((long long)n * tid / TA), hi = (int)((long long)n * (tid + 1) / TA);
                    for (int k = lo; k < hi; k++) {
                        const RView &v = s->view[k] = view_of(next + k);
                        char *dst = s->seq + s->soff[k];
                        if (v.rc) { for (uint32_t i = 0; i < v.sl; i++) dst[i] = comp_base_f(v.s[v.sl - 1 - i]); }
                        else memcpy(dst, v.s, v.sl);
                    }
                });
            }
            st.t_asm += now_s() - ta;
            next = end;
            { std::lock_guard<std::mutex> lk(mu); map_q.push_back(s); }
            cv.notify_all();
        }
        { std::lock_guard<std::mutex> lk(mu); asm_done = true; }
        cv.notify_all();
    });

    std::vector<std::thread> mappers;
    for (size_t w = 0; w < job.ctx.size(); w++) mappers.emplace_back([&, w]() {
        if (c.umi) { dg_umi u = c.umi_par; u.flags = pair_end ? DG_UMI_PAIRS : 0u; if (dg_set_umi(job.ctx[w], &u)) { std::lock_guard<std::mutex> lk(mu); failed = true; fail_rc = DG_ERR_ARG; err = dg_last_error(job.ctx[w]); } }
        if (c.trim) { dg_trim t = c.trim_par; t.flags = pair_end ? DG_TRIM_PAIRS : 0u; if (dg_set_trim(job.ctx[w], &t)) { std::lock_guard<std::mutex> lk(mu); failed = true; fail_rc = DG_ERR_ARG; err = dg_last_error(job.ctx[w]); } }
        while (true) {
            FastSlot *s;
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return !map_q.empty() || asm_done || failed; }); if (failed || map_q.empty()) break; s = map_q.front(); map_q.pop_front(); }
            const double tm = now_s();
            double t_fq = 0, t_gz_wait = 0; float fq_ms = 0.f;
            if (!s->rc && s->fq_device) {
                // upload the text (the device cuts it into the batch) -> run -> download
                int n = s->n;
                dg_params p = c.p; p.paired = (pair_end && !s->odd) ? 1 : 0;
                dg_set_params(job.ctx[w], &p);
                dg_fastq_text ft; ft.text1 = s->fq1; ft.n1 = s->fq_n1; ft.text2 = s->fq2; ft.n2 = s->fq_n2; ft.rc_odd_reads = pair_end ? 1 : 0; ft.max_reads = n;
                int got = 0;
                double tu = now_s();
                int rc;
                if (s->gz_chunk >= 0) {
                    // the uploads take turns: this chunk's heads are the tails of the one before
                    std::unique_lock<std::mutex> lk(gzp->mu);
                    gzp->cv.wait(lk, [&]() { return gzp->turn == (size_t)s->gz_chunk; });
                    t_gz_wait = now_s() - tu; tu = now_s();
                    uint64_t unlike = 0;
                    rc = GzDevPlan::upload(job.ctx[w], *gzp, gzp->chunks[s->gz_chunk], gzp->tail1, gzp->tail2, pair_end, n, 0u, &got, &unlike);
                    gzp->turn++;
                    lk.unlock(); gzp->cv.notify_all();
                } else rc = dg_batch_upload_fastq(job.ctx[w], &ft, &got);
                t_fq = now_s() - tu;
                (void)dg_batch_fastq_device_ms(job.ctx[w], &fq_ms);
                if (!rc && c.cuts()) {             // the batch is what the upload kept: every count behind it is the returned one
                    uint64_t ts[16]; float tms = 0.f;
                    (void)dg_batch_trim_stats(job.ctx[w], ts, &tms);
                    for (int k = 0; k < 16; k++) job.trim_stats[k] += ts[k];
                    job.trim_kernel_us += (unsigned long long)(tms * 1e3f);
                    s->n = n = got;
                }
                if (!rc && got != n) { s->rc = DG_ERR_INTERNAL; s->err = "the device parser found " + std::to_string(got) + " reads in a batch of " + std::to_string(n); }
                else if (rc) { s->rc = rc; s->err = dg_last_error(job.ctx[w]); }
                else {
                    rc = dg_batch_run(job.ctx[w], s->used);
                    if (!rc && (s->used[0] > s->caps[0] || s->used[1] > s->caps[1] || s->used[2] > s->caps[2])) {
                        const size_t need[3] = { s->used[0] + s->used[0] / 8 + 1024, s->used[1] + s->used[1] / 8 + 1024, s->used[2] + s->used[2] / 8 + 1024 };
                        job.pool.reserve(*s, (size_t)n, 0, need);
                    }
                    if (!rc && c.device_sj) rc = sj_accumulate(job, job.ctx[w]);
                    if (!rc && c.gene_gtf) rc = gene_accumulate(job, job.ctx[w], (pair_end && !s->odd) ? n : 0);
                    if (!rc && c.tx_gtf) rc = tx_accumulate(job, job.ctx[w], (pair_end && !s->odd) ? n : 0);
                    if (!rc) rc = dg_batch_download(job.ctx[w], s->ro, s->po, s->cig, c.device_sj ? nullptr : s->sj, s->caps);
                    s->rc = rc; if (rc) s->err = dg_last_error(job.ctx[w]);
                }
            } else
            if (!s->rc) {
                const int n = s->n;
                for (int attempt = 0; attempt < 2; attempt++) {
                    if (attempt) { const size_t need[3] = { s->used[0] * 2 + 1024, s->used[1] * 2 + 1024, s->used[2] * 2 + 1024 }; job.pool.reserve(*s, (size_t)n, 0, need); }
                    dg_params p = c.p; p.paired = (pair_end && !s->odd) ? 1 : 0;
                    dg_set_params(job.ctx[w], &p);
                    int rc = dg_map_batch(job.ctx[w], n, s->soff.data(), s->rl.data(), s->seq, s->ro, s->po, s->cig, c.device_sj ? nullptr : s->sj, s->caps, s->used);
                    if (rc == DG_ERR_CAPACITY && attempt == 0) continue;      // `used` holds the need
                    if (!rc && c.device_sj) rc = sj_accumulate(job, job.ctx[w]);       // (a batch that ran short of capacity is mapped again as a new batch and was not counted)
                    if (!rc && c.gene_gtf) rc = gene_accumulate(job, job.ctx[w], (pair_end && !s->odd) ? n : 0);
                    if (!rc && c.tx_gtf) rc = tx_accumulate(job, job.ctx[w], (pair_end && !s->odd) ? n : 0);
                    s->rc = rc; if (rc) s->err = dg_last_error(job.ctx[w]);
                    break;
                }
            }
            double t_gather = 0, t_call = 0, t_dl = 0; float dev_ms = 0.f;
            const bool dev_out = c.device_sam || c.device_bam;
            // the device's formatter for this job: SAM text, or with DART_DEVICE_BAM the BGZF blocks of the BAM records (in == nullptr: the resident form)
            auto dev_format = [&](const dg_sam_text *in, int npm, size_t *nb) -> int {
                const uint32_t fl = c.unique ? DG_SAM_UNIQUE_ONLY : 0u;
                if (!c.device_bam) return in ? dg_batch_format_sam(job.ctx[w], in, fl, nb, s->dev_ct, &dev_ms) : dg_batch_format_sam_resident(job.ctx[w], npm, fl, nb, s->dev_ct, &dev_ms);
                uint64_t ct[5] = {0, 0, 0, 0, 0}; size_t raw = 0;
                const uint32_t bfl = fl | (c.sort_bam ? DG_BAM_RAW : c.bgzf_dynamic ? DG_BAM_DYNAMIC : 0u);
                int rc = in ? dg_batch_format_bam(job.ctx[w], in, bfl, nb, &raw, ct, &dev_ms) : dg_batch_format_bam_resident(job.ctx[w], npm, bfl, nb, &raw, ct, &dev_ms);
                for (int i = 0; i < 3; i++) s->dev_ct[i] = ct[i];
                s->bam_rr[0] = ct[3]; s->bam_rr[1] = ct[4];
                if (!rc && c.sort_bam) {
                    const unsigned long long t = now_ns();
                    rc = dg_batch_accumulate_bam(job.ctx[w], (uint32_t)(job.sort_ordinal_base + s->seqno), nullptr, nullptr);
                    job.sort_acc_ns += now_ns() - t;
                    *nb = 0;                                  // the records stay in HBM: the slot carries the counters alone
                }
                return rc;
            };
            auto dev_download = [&]() -> int { return c.sort_bam ? 0 : c.device_bam ? dg_batch_download_bam(job.ctx[w], s->text, s->text_cap) : dg_batch_download_sam(job.ctx[w], s->text, s->text_cap); };
            // format on the device, then the text (or the blocks) into the slot
            auto dev_text = [&](const dg_sam_text *in, int npm) {
                size_t nb = 0;
                const double tc = now_s();
                int rc = dev_format(in, npm, &nb);
                t_call = now_s() - tc;
                if (!rc) {
                    const double td = now_s();
                    job.pool.reserve_text(*s, nb);
                    rc = dev_download();
                    s->text_n = nb;
                    t_dl = now_s() - td;
                }
                if (rc) { s->rc = rc; s->err = dg_last_error(job.ctx[w]); }
            };
            if (!s->rc && dev_out && s->fq_device) dev_text(nullptr, (pair_end && !s->odd) ? s->n : 0);      // names and qualities are in HBM already, in stored order: nothing to gather
            else
            if (!s->rc && dev_out) {
                // the batch's names and qualities, flat, mate 2's qualities in stored order (reversed); then the text from the device
                const double tg = now_s();
                const int n = s->n;
                s->hoff.resize((size_t)n + 1); s->qoff.resize((size_t)n + 1);
                uint32_t ho = 0, qo = 0; bool fits = true;
                for (int k = 0; k < n; k++) { s->hoff[k] = ho; s->qoff[k] = qo; const RView &v = s->view[k]; if ((uint64_t)ho + v.hl + qo + v.ql > 0xFFFFFF00ull) { fits = false; break; } ho += v.hl; qo += v.ql; }
                s->hoff[n] = ho; s->qoff[n] = qo;
                if (!fits) { s->rc = DG_ERR_ARG; s->err = "names and qualities of a batch exceed 32-bit offsets"; }
                else {
                    if ((size_t)ho + qo + 64 > s->nq_cap) { job.pool.release(s->names_quals); s->nq_cap = ((size_t)ho + qo) * 9 / 8 + 4096; s->names_quals = (char *)job.pool.alloc(s->nq_cap); }
                    char *hb = s->names_quals, *qb = s->names_quals + ho;
                    const int TG = std::max(1, T / 8);
                    parallel_for(TG, [&](int tid) {
                        const int lo = (int)((long long)n * tid / TG), hi = (int)((long long)n * (tid + 1) / TG);
                        for (int k = lo; k < hi; k++) {
                            const RView &v = s->view[k];
                            memcpy(hb + s->hoff[k], v.h, v.hl);
                            if (v.rc) rev_copy(qb + s->qoff[k], v.q, v.ql); else memcpy(qb + s->qoff[k], v.q, v.ql);
                        }
                    });
                    t_gather = now_s() - tg;
                    dg_sam_text in; in.hdr_off = s->hoff.data(); in.hdr = hb; in.qual_off = s->qoff.data(); in.qual = qb; in.n_pair_mode = (pair_end && !s->odd) ? n : 0;
                    dev_text(&in, in.n_pair_mode);
                }
            }
            { std::lock_guard<std::mutex> lk(mu); st.t_map += now_s() - tm - t_gather - t_call - t_dl - t_fq - t_gz_wait; st.t_gz_tail += t_gz_wait; st.t_fq_call += t_fq; st.t_fq_kernels += fq_ms * 1e-3; st.t_gather += t_gather; st.t_dev_call += t_call; st.t_dev_kernels += dev_ms * 1e-3; st.t_download += t_dl; st.n_batches++; if (s->rc) { failed = true; fail_rc = s->rc; err = s->err; } fmt_q[s->seqno] = s; }
            cv.notify_all();
        }
        if (c.umi) (void)dg_set_umi(job.ctx[w], nullptr);
        if (c.trim) (void)dg_set_trim(job.ctx[w], nullptr);      // (the next library's check pass, and its pairing, start from an untrimmed context)
        { std::lock_guard<std::mutex> lk(mu); mappers_left--; }
        cv.notify_all();
    });

    // format (this thread drives; T threads do the work) and write (its own thread, T threads again), batches in order; two sets of
    // text buffers, so batch b+1 is formatted while batch b is written
    struct TextSet { std::vector<TextBuf> bufs; std::vector<Counters> cts; FastSlot *slot = nullptr; bool full = false;
                     std::vector<std::pair<const char *, size_t>> pieces; };      // the text in file order: the formatter threads' buffers, or the slot's device text
    TextSet sets[2];
    for (auto &ts : sets) { ts.bufs.resize(TF); ts.cts.resize(TF); }
    bool fmt_done = false;
    std::thread writer([&]() {
        int cur = 0;
        while (true) {
            TextSet &ts = sets[cur];
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return ts.full || fmt_done || failed; }); if (!ts.full) break; }
            const double tw = now_s();
            FastSlot *s = ts.slot;
            std::vector<size_t> offs(TF + 1, 0);
            for (int k = 0; k < TF; k++) offs[k + 1] = offs[k] + ts.pieces[k].second;
            const uint64_t base = job.sam_off;
            char *win = nullptr; size_t win_len = 0; const uint64_t a0 = base & ~(uint64_t)4095;
            if (use_mmap && !c.device_bam && offs[TF] && ftruncate(job.sam_fd, (off_t)(base + offs[TF])) == 0) {      // copy into a shared mapping of the file's new part
                win_len = (size_t)(base + offs[TF] - a0);
                void *m = mmap(nullptr, win_len, PROT_READ | PROT_WRITE, MAP_SHARED, job.sam_fd, (off_t)a0);
                win = m == MAP_FAILED ? nullptr : (char *)m;
            }
            const int TW = win ? std::max(1, TF / 4) : TWR;     // writes to one file serialise in the kernel: more threads only burn the CPU share
            std::atomic<int> write_errno{0};                 // a full disk must not end as a holed SAM file and exit code 0
            if (c.device_bam) { if (!job.bam_sink || !job.bam_sink(ts.pieces[0].first, ts.pieces[0].second, (long long)s->bam_rr[0], (long long)s->bam_rr[1])) write_errno = errno ? errno : EIO; }
            else if (use_mmap && offs[TF] && !win) write_errno = errno ? errno : EIO;
            else parallel_for(TW, [&](int wt) {
                for (int tid = wt; tid < TF; tid += TW) {
                    const char *piece = ts.pieces[tid].first; const size_t piece_n = ts.pieces[tid].second;
                    if (win) { memcpy(win + (base - a0) + offs[tid], piece, piece_n); continue; }
                    size_t done = 0;
                    while (done < piece_n) {
                        const ssize_t w = pwrite(job.sam_fd, piece + done, piece_n - done, (off_t)(base + offs[tid] + done));
                        if (w < 0 && errno == EINTR) continue;
                        if (w <= 0) { write_errno = w < 0 ? errno : ENOSPC; break; }
                        done += (size_t)w;
                    }
                }
            });
            if (win) munmap(win, win_len);
            if (write_errno) {
                { std::lock_guard<std::mutex> lk(mu); failed = true; fail_rc = DG_ERR_INTERNAL; err = std::string("writing the output failed: ") + strerror(write_errno); ts.full = false; }
                cv.notify_all();
                break;
            }
            if (!c.device_bam) job.sam_off = base + offs[TF];
            for (int k = 0; k < TF; k++) { job.total.unique += ts.cts[k].unique; job.total.unmapped += ts.cts[k].unmapped; job.total.paired += ts.cts[k].paired; }
            batch_written(job, s->n, s->sj, s->used[2]);
            st.t_write += now_s() - tw;
            { std::lock_guard<std::mutex> lk(mu); ts.full = false; free_q.push_back(s); }
            cv.notify_all();
            cur ^= 1;
        }
    });
    size_t next_out = 0;
    int fill = 0;
    while (true) {
        FastSlot *s = nullptr;
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return fmt_q.count(next_out) || failed || (mappers_left == 0 && fmt_q.empty()); });
          if (failed) break;
          if (fmt_q.count(next_out)) { s = fmt_q[next_out]; fmt_q.erase(next_out); } else break; }
        TextSet &ts = sets[fill];
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return !ts.full || failed; }); if (failed) break; }
        const double tf = now_s();
        const int n = s->n, n_pair_mode = (pair_end && !s->odd) ? n : 0;
        ts.pieces.assign(TF, std::make_pair((const char *)nullptr, (size_t)0));
        if (c.device_sam || c.device_bam) {                   // formatted on the device behind the mapping: the text (or the BGZF blocks) is in the slot
            for (int tid = 0; tid < TF; tid++) ts.cts[tid] = Counters();
            ts.pieces[0] = std::make_pair((const char *)s->text, s->text_n);
            ts.cts[0].unmapped = (long long)s->dev_ct[0]; ts.cts[0].unique = (long long)s->dev_ct[1]; ts.cts[0].paired = (long long)s->dev_ct[2];
        } else {
            parallel_for(TF, [&](int tid) {
                int lo = (int)((long long)n * tid / TF) & ~1, hi = tid == TF - 1 ? n : ((int)((long long)n * (tid + 1) / TF) & ~1);
                ts.bufs[tid].n = 0; ts.cts[tid] = Counters();
                format_views(s->view.data(), lo, hi, n_pair_mode, s->ro, s->po, s->cig, job.names, c.unique, c.multi, true, ts.bufs[tid], ts.cts[tid]);
                ts.pieces[tid] = std::make_pair((const char *)ts.bufs[tid].b, ts.bufs[tid].n);
            });
            st.t_fmt += now_s() - tf;
        }
        { std::lock_guard<std::mutex> lk(mu); ts.slot = s; ts.full = true; }
        cv.notify_all();
        next_out++; fill ^= 1;
    }
    { std::lock_guard<std::mutex> lk(mu); fmt_done = true; }
    cv.notify_all();
    writer.join();
    if (failed) cv.notify_all();
    assembler.join();
    for (auto &m : mappers) m.join();
    return failed ? (fail_rc ? fail_rc : DG_ERR_INTERNAL) : 0;
}
