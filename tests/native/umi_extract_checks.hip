// tests/native/umi_extract_checks.hip -- the host-callable rules of the inline UMI cut (dart_amd/csrc/dg_trim.h: trim_umi_slot, trim_umi_partnered, trim_umi_cut,
// trim_umi_ok, trim_umi_letter, trim_umi_suffix) run on the CPU over reads in batch order, as k_trim_cut, k_trim_len and k_trim_write apply them.
// usage: umi_extract_checks <input>
//   input   i64 n_reads, two, flags, len[0], len[1], skip[0], skip[1], sep; per read i64 file, L and its L bases
//   stdout  per read "<slot> <cut> <fails> <dropped> <partnered> <suffix>": the suffix (sep and letters) only for a read that is not dropped
#include "../../dart_amd/csrc/dg_trim.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "umi_extract_checks: %s failed (line %d)\n", #x, __LINE__); exit(2); } } while (0)

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: umi_extract_checks <input>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    long long head[8];
    CHECK(fread(head, 8, 8, f) == 8);
    const uint32_t n = (uint32_t)head[0];
    const bool two = head[1] != 0;
    TrimPar par; memset(&par, 0, sizeof par);
    par.umi_on = 1; par.umi_flags = (uint32_t)head[2]; par.umi_len[0] = (uint32_t)head[3]; par.umi_len[1] = (uint32_t)head[4]; par.umi_skip[0] = (uint32_t)head[5]; par.umi_skip[1] = (uint32_t)head[6];
    par.umi_sep = (uint32_t)head[7];
    std::vector<int> file(n); std::vector<std::vector<char>> read(n);      // (exact-size copies on the heap: a letter read behind a read's end is seen by the sanitizer build)
    for (uint32_t k = 0; k < n; k++) {
        long long h2[2]; CHECK(fread(h2, 8, 2, f) == 2);
        file[k] = (int)h2[0]; read[k].resize((size_t)h2[1]);
        if (h2[1]) CHECK(fread(read[k].data(), 1, (size_t)h2[1], f) == (size_t)h2[1]);
    }
    fclose(f);
    std::vector<int> slot(n); std::vector<uint32_t> cut(n); std::vector<bool> fail(n);
    for (uint32_t k = 0; k < n; k++) {                                // k_trim_cut
        slot[k] = trim_umi_slot(k, two, file[k], par.umi_flags); cut[k] = trim_umi_cut(par, slot[k]);
        fail[k] = !trim_umi_ok((uint32_t)read[k].size(), cut[k]);
    }
    for (uint32_t k = 0; k < n; k++) {                                // k_trim_len's verdict and name length, k_trim_write's suffix
        const bool partnered = trim_umi_partnered(k, two, par.umi_flags, n), drop = fail[k] || (partnered && fail[k ^ 1u]);
        std::string sfx;
        if (!drop) {
            sfx.push_back((char)par.umi_sep);
            for (uint32_t j = 0; j < (partnered ? 2u : 1u); j++) {
                const uint32_t kk = partnered ? (k & ~1u) + j : k, len = par.umi_len[slot[kk]];
                CHECK(len <= read[kk].size());
                for (uint32_t i = 0; i < len; i++) sfx.push_back(trim_umi_letter(read[kk][i]));
            }
            CHECK(sfx.size() == trim_umi_suffix(par, slot[k], partnered));
        }
        printf("%d %u %d %d %d %s\n", slot[k], cut[k], (int)fail[k], (int)drop, (int)partnered, sfx.c_str());
    }
    return 0;
}
