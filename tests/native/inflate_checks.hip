// CPU suite: the __host__ __device__ functions of dart_amd/csrc/dg_inflate.h run on the host, in the kernel's order.
//   inflate_checks <cases> <out>
// <cases>: any number of { u32 n, n bytes of BGZF members }.  Every case goes through inf_walk_members and then, member by member, through inf_member -- the
// whole of what one wave of k_bgzf_inflate runs, the lanes of a phase one after the other, once in ascending order and once in a scrambled one (the bytes
// must not depend on it).  A member's input and output lie in heap blocks of exactly in_len and isize bytes, so that a build with the sanitizers sees any byte
// read or written outside them.
// <out>: per case { i32 verdict, u32 member, u32 n, n bytes }: verdict 0 and the inflated bytes; -1: the walker refused member `member`; > 0: the INF_E_* rule
// member `member` broke (n = 0).
#include "../../dart_amd/csrc/dg_inflate.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static bool run_case(const unsigned char *p, size_t n, const uint32_t *crc_tab, InfLds *lds, int32_t &verdict, uint32_t &member, std::vector<unsigned char> &bytes)
{
    std::vector<InfBlock> tab;
    size_t n_out = 0, bad = 0;
    verdict = 0; member = 0; bytes.clear();
    if (inf_walk_members(p, n, 0, 0, tab, &n_out, &bad)) { verdict = -1; member = (uint32_t)bad; return true; }
    for (size_t k = 0; k < tab.size(); k++) {
        const InfBlock &b = tab[k];
        if (b.in_off + b.in_len > n) return false;
        unsigned char *in = (unsigned char *)malloc(b.in_len ? b.in_len : 1), *out[2];
        memcpy(in, p + b.in_off, b.in_len);
        uint32_t st[2];
        for (int pass = 0; pass < 2; pass++) {
            out[pass] = (unsigned char *)malloc(b.isize ? b.isize : 1);
            memset(out[pass], 0xA5, b.isize);
            memset(lds, 0x5A, sizeof *lds);                       // nothing may be read before it is written: garbage would change a verdict
            inf_host_lane_xor = pass ? 37u : 0u;
            st[pass] = inf_member(*lds, crc_tab, in, b.in_len, out[pass], b.isize, b.crc);
        }
        const bool same = st[0] == st[1] && (st[0] != INF_OK || memcmp(out[0], out[1], b.isize) == 0);
        if (same && st[0] == INF_OK) bytes.insert(bytes.end(), out[0], out[0] + b.isize);
        free(in); free(out[0]); free(out[1]);
        if (!same) return false;
        if (st[0] != INF_OK) { verdict = (int32_t)st[0]; member = (uint32_t)k; bytes.clear(); return true; }
    }
    return bytes.size() == n_out;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: inflate_checks <cases> <out>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t crc_tab[256];
    for (uint32_t i = 0; i < 256; i++) crc_tab[i] = bgzf_crc_entry(i);
    InfLds *lds = new InfLds;
    uint32_t n;
    int n_cases = 0;
    while (fread(&n, 4, 1, f) == 1) {
        std::vector<unsigned char> in(n ? n : 1), bytes;
        if (n && fread(in.data(), 1, n, f) != n) return 3;
        unsigned char *exact = (unsigned char *)malloc(n ? n : 1);   // (the walker too must stay inside the case's bytes)
        memcpy(exact, in.data(), n);
        int32_t verdict; uint32_t member;
        const bool ok = run_case(exact, n, crc_tab, lds, verdict, member, bytes);
        free(exact);
        if (!ok) { fprintf(stderr, "case %d: the lane order changed the result, or the sizes do not add up\n", n_cases); return 4; }
        const uint32_t nb = (uint32_t)bytes.size();
        fwrite(&verdict, 4, 1, o); fwrite(&member, 4, 1, o); fwrite(&nb, 4, 1, o);
        if (nb) fwrite(bytes.data(), 1, nb, o);
        n_cases++;
    }
    delete lds;
    fclose(f); fclose(o);
    printf("cases %d\n", n_cases);
    return 0;
}
