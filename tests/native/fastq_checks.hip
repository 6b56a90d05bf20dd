// CPU suite: the __host__ __device__ functions of dart_amd/csrc/dg_fastq.h -- the record rules of the device's FASTQ parser -- run on the host the way the
// kernels use them: newlines found 16 bytes at a time (k_fq_count / k_fq_lines), a read's place among the records (k_fq_len), its lengths, and its stored
// bytes one by one (k_fq_write).  No HIP call.
// argv[1]: i64 two, rc_odd_reads, n1, n2, then text1 and text2 (each padded to 8 bytes); argv[2]: out = i64 n_reads (-1: the record counts do not fit),
// i64 rlen[n], u32 name length[n], u32 quality length[n], then per read its stored bases, name and stored quality.
#include "../../dart_amd/csrc/dg_fastq.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

struct Text { std::vector<char> t; uint64_t n = 0; std::vector<uint32_t> line_start; uint64_t n_nl = 0, n_lines = 0; };

// line starts as the kernels find them: the mask of every 16 bytes, a line start behind each newline; a last line without '\n' counts
static void find_lines(Text &x)
{
    x.line_start.assign(1, 0u);
    for (uint64_t pos = 0; pos < x.n; pos += 16) {
        uint32_t w[4];
        memcpy(w, x.t.data() + pos, 16);                        // (the buffer is padded: only the first n - pos bytes count)
        uint32_t m = fq_nl_mask16(w[0], w[1], w[2], w[3], x.n - pos);
        for (; m; m &= m - 1) x.line_start.push_back((uint32_t)(pos + (uint32_t)__builtin_ctz(m) + 1u));
    }
    x.n_nl = x.line_start.size() - 1;
    x.n_lines = x.n_nl + ((x.n && x.t[x.n - 1] != '\n') ? 1 : 0);
}
static uint32_t line_len(const Text &x, uint64_t i, uint32_t &start)
{
    if (i >= x.n_lines) { start = 0; return 0; }
    start = x.line_start[i];
    return (uint32_t)((i < x.n_nl ? x.line_start[i + 1] : x.n) - start);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[4];
    if (fread(h, 8, 4, f) != 4) return 2;
    Text x[2];
    for (int i = 0; i < 2; i++) {
        x[i].n = (uint64_t)h[2 + i];
        x[i].t.assign(((x[i].n + 7) & ~7ull) + 32, (char)0x0A);      // the bytes behind the text are newlines: the mask must not see them
        if (x[i].n && fread(x[i].t.data(), 1, (x[i].n + 7) & ~7ull, f) != ((x[i].n + 7) & ~7ull)) return 2;
        for (uint64_t k = x[i].n; k < x[i].t.size(); k++) x[i].t[k] = (char)0x0A;
        find_lines(x[i]);
    }
    fclose(f);
    const bool two = h[0] != 0; const int rc_odd = (int)h[1];
    const int64_t n = fq_read_count(two, (x[0].n_lines + 3) / 4, two ? (x[1].n_lines + 3) / 4 : 0);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(&n, 8, 1, o);
    if (n < 0) { fclose(o); printf("record counts do not fit\n"); return 0; }
    std::vector<int64_t> rl(n); std::vector<uint32_t> hl(n), ql(n); std::vector<char> body;
    for (int64_t k = 0; k < n; k++) {
        int file; uint32_t rec;
        fq_read_place((uint32_t)k, two, file, rec);
        const Text &t = x[file];
        uint32_t s0, s1, s2, s3;
        const uint32_t l0 = line_len(t, 4ull * rec, s0), l1 = line_len(t, 4ull * rec + 1, s1), l2 = line_len(t, 4ull * rec + 2, s2), l3 = line_len(t, 4ull * rec + 3, s3);
        const FqRecord r = fq_record(t.t.data(), s0, l0, l1, l2, l3);
        if (l1 && r.seq_at != s1) { fprintf(stderr, "read %lld: line 1 is not behind line 0\n", (long long)k); return 1; }
        if (l3 && r.qual_at != s3) { fprintf(stderr, "read %lld: line 3 is not behind line 2\n", (long long)k); return 1; }
        rl[k] = r.rlen; hl[k] = r.hl; ql[k] = r.ql;
        const bool rc = fq_stored_rc((uint32_t)k, rc_odd);
        if (r.rlen > 0) for (uint32_t i = 0; i < (uint32_t)r.rlen; i++) body.push_back(fq_stored_base(t.t.data() + r.seq_at, (uint32_t)r.rlen, i, rc));
        for (uint32_t i = 0; i < r.hl; i++) body.push_back(t.t[r.name_at + i]);
        for (uint32_t i = 0; i < r.ql; i++) body.push_back(fq_stored_qual(t.t.data() + r.qual_at, r.ql, i, rc));
    }
    fwrite(rl.data(), 8, n, o); fwrite(hl.data(), 4, n, o); fwrite(ql.data(), 4, n, o); fwrite(body.data(), 1, body.size(), o);
    fclose(o);
    printf("reads %lld\n", (long long)n);
    return 0;
}
