// CPU suite: the __host__ __device__ functions of dart_amd/csrc/dg_samfmt.h -- the per-read arithmetic of the device's SAM formatter -- run on the
// host, read by read, the way k_sam_len (lengths, counters) and k_sam_write (the text; its staged fields through the same bounded sink) use them.
// argv[1]: a batch written by tests/sam_device_inputs.py::write_batch; argv[2]: out = u64 len[n], u64 counters[3], u64 text bytes, the text.
#include "../../dart_amd/csrc/dg_samfmt.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static std::vector<char> blob;
static size_t at = 0;
template <typename T> static const T *take(size_t n) { const T *p = (const T *)(blob.data() + at); at += (n * sizeof(T) + 7) & ~(size_t)7; if (at > blob.size()) { fprintf(stderr, "input too short\n"); exit(2); } return p; }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END); blob.resize((size_t)ftell(f) + 8); fseek(f, 0, SEEK_SET);
    if (fread(blob.data(), 1, blob.size() - 8, f) != blob.size() - 8) return 2;
    fclose(f);
    const int32_t *h = take<int32_t>(8);
    const int n = h[0], n_rep = h[1], n_cig = h[2], n_chr = h[3], has_qual = h[7];
    SamBatch b;
    b.n_reads = n; b.n_pair_mode = h[4]; b.unique_only = h[5]; b.multi = h[6]; b.qlen = nullptr;
    b.ro = take<dg_read_out>(n); b.po = take<dg_report_out>(n_rep); b.cig = take<uint32_t>(n_cig);
    b.seq_off = take<uint32_t>(n + 1); b.rlen = take<uint16_t>(n); b.seq = take<unsigned char>(b.seq_off[n]);
    b.hdr_off = take<uint32_t>(n + 1); b.hdr = take<char>(b.hdr_off[n]);
    b.qual_off = take<uint32_t>(n + 1); b.qual = take<char>(b.qual_off[n]);
    if (!has_qual) b.qual = nullptr;
    b.chr_off = take<uint32_t>(n_chr + 1); b.chr = take<char>(b.chr_off[n_chr]);

    std::vector<uint64_t> len(n);
    uint64_t ct64[3] = {0, 0, 0}, total = 0;
    std::vector<uint32_t> ql(n);
    for (int k = 0; k < n; k++) { uint32_t ct[3] = {0, 0, 0}; len[k] = sam_read_len(b, k, ct, &ql[k]); total += len[k]; for (int i = 0; i < 3; i++) ct64[i] += ct[i]; }
    std::vector<char> text(total + 1);
    uint64_t pos = 0; int bad = 0;
    SamBatch b2 = b; b2.qlen = ql.data();                  // the writer takes the quality lengths pass 1 left, as k_sam_write does
    for (int k = 0; k < n; k++) {
        const uint64_t w = sam_read_text(b2, k, text.data() + pos);
        if (w != len[k]) { fprintf(stderr, "read %d: wrote %llu bytes, pass 1 said %llu\n", k, (unsigned long long)w, (unsigned long long)len[k]); bad++; }
        // the fields of every line once more through the kernel's bounded staging sink: the same bytes, or a count that says "does not fit"
        const SamRead e = sam_read_begin(b2, k);
        uint64_t lp = pos;
        for (int j = sam_line_first(b2, e); j != SAM_LINE_NONE; j = sam_line_after(b2, e, j)) {
            char stage[SAM_MID_STAGE], tail[SAM_TAIL_STAGE];
            SamSink m{stage, 0, SAM_MID_STAGE}, t{tail, 0, SAM_TAIL_STAGE};
            sam_line_mid(b2, e, j, m); sam_line_tail(e, j, t);
            const uint64_t ll = sam_line_len(b2, e, j);
            if (m.n <= SAM_MID_STAGE && memcmp(stage, text.data() + lp + e.hl, m.n)) { fprintf(stderr, "read %d line %d: staged fields differ\n", k, j); bad++; }
            if (t.n > SAM_TAIL_STAGE || memcmp(tail, text.data() + lp + ll - t.n, t.n)) { fprintf(stderr, "read %d line %d: staged tags differ\n", k, j); bad++; }
            lp += ll;
        }
        if (lp != pos + w) { fprintf(stderr, "read %d: line lengths do not add up\n", k); bad++; }
        pos += w;
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(len.data(), 8, n, o); fwrite(ct64, 8, 3, o); fwrite(&pos, 8, 1, o); fwrite(text.data(), 1, pos, o);
    fclose(o);
    printf("reads %d bytes %llu bad %d\n", n, (unsigned long long)pos, bad);
    return bad ? 1 : 0;
}
