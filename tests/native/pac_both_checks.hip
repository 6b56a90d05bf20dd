// Host run of every host-callable reader of the 2-bit text (dg_common.h, dg_pair.h, dg_report.h) in its two forms: pac holding both strands (DIndex::pac_both = 1,
// what every kernel is launched with) against pac holding the forward half only (pac_both = 0, the form the other host checks keep running).  Random texts of
// L = 5, 6, 7, 8, 37, 64, 1000, 4099 symbols (every L % 4); the second half is built here from its definition T[t] = 3 - T[2L-1-t], symbol by symbol, and the
// library's per-byte rule (d_pac_both_byte, what k_pac_both runs) must give the same bytes, in place.  Then for every g in [-70, 2L + 70) and every window
// length: d_refchar, d_ref8, d_ref_codes (n = 1 .. 28), ReadAscii / ReadWords ::mismatches8 (e = 1 .. 8) and the 64-symbol window d_text64 must agree between
// the forms, d_text64 also with d_refchar symbol by symbol.  Compiled with hipcc, run without a GPU (no HIP API call).  Test infrastructure.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <cstdlib>
#include <vector>
#include "../../include/dartgpu.h"
#include "../../dart_amd/csrc/dg_common.h"
#include "../../dart_amd/csrc/dg_pair.h"
#include "../../dart_amd/csrc/dg_report.h"

static uint64_t rng_s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return rng_s; }

// where a window [g, g + len) lies in the text [0, 2L)
struct Where { long straddle_L, at_begin, at_end, first_half, second_half, outside; };
static void count(Where &w, int64_t g, int len, int64_t L)
{
    if (g + len <= 0 || g >= 2 * L) w.outside++;
    else if (g < 0) w.at_begin++;
    else if (g + len > 2 * L) w.at_end++;
    else if (g < L && g + len > L) w.straddle_L++;
    else if (g + len <= L) w.first_half++;
    else w.second_half++;
}

int main()
{
    const int64_t Ls[] = {5, 6, 7, 8, 37, 64, 1000, 4099};
    long bad = 0, n_cmp = 0, n_codes_ok_both = 0, n_codes_ok_new = 0, n_bytes = 0;
    Where w8 = {0, 0, 0, 0, 0, 0}, w64 = w8, wn = w8;
    auto fail = [&](const char *what, int64_t L, int64_t g, int len) { if (bad++ < 20) printf("MISMATCH %s L=%lld g=%lld len=%d\n", what, (long long)L, (long long)g, len); };
    for (const int64_t L : Ls) {
        const size_t nbytes = (size_t)((2 * L + 3) / 4), cap = nbytes + 4096;
        std::vector<uint8_t> sym((size_t)(2 * L));                       // the text by its definition
        for (int64_t t = 0; t < L; t++) sym[(size_t)t] = (uint8_t)(rnd() & 3);
        for (int64_t t = L; t < 2 * L; t++) sym[(size_t)t] = (uint8_t)(3 - sym[(size_t)(2 * L - 1 - t)]);
        std::vector<uint32_t> fwd_w(cap / 4 + 2, 0), both_w(cap / 4 + 2, 0), def_w(cap / 4 + 2, 0);
        uint8_t *fwd = (uint8_t *)fwd_w.data(), *both = (uint8_t *)both_w.data(), *def = (uint8_t *)def_w.data();
        for (int64_t t = 0; t < L; t++) fwd[t >> 2] |= (uint8_t)(sym[(size_t)t] << ((~t & 3) << 1));
        for (int64_t t = 0; t < 2 * L; t++) def[t >> 2] |= (uint8_t)(sym[(size_t)t] << ((~t & 3) << 1));
        memcpy(both, fwd, cap);
        for (int64_t b = L / 4; b < (int64_t)nbytes; b++) { both[b] = d_pac_both_byte(both, L, b); n_bytes++; }      // in place, as the kernel does
        if (memcmp(both, def, cap) != 0) fail("d_pac_both_byte", L, 0, 0);

        DIndex F; memset(&F, 0, sizeof F); F.pac = fwd; F.l_pac = L;
        DIndex B; memset(&B, 0, sizeof B); B.pac = both; B.l_pac = L; B.pac_both = 1;
        for (int64_t g = -70; g < 2 * L + 70; g++) {
            // ---- one symbol
            const char cf = d_refchar(F, g), cb = d_refchar(B, g);
            const char want = g >= 0 && g < 2 * L ? "ACGT"[sym[(size_t)g]] : 0;
            n_cmp++;
            if (cf != want || cb != want) fail("d_refchar", L, g, 1);
            // ---- eight characters
            count(w8, g, 8, L); n_cmp++;
            if (d_ref8(F, g) != d_ref8(B, g)) fail("d_ref8", L, g, 8);
            // ---- n <= 28 codes
            for (int n = 1; n <= 28; n++) {
                bool okf = false, okb = false;
                const uint64_t xf = d_ref_codes(F, g, n, &okf), xb = d_ref_codes(B, g, n, &okb);
                count(wn, g, n, L); n_cmp++;
                if (okf && !okb) fail("d_ref_codes: ok only without the second half", L, g, n);
                if (okf && okb) { n_codes_ok_both++; if ((xf >> (64 - 2 * n)) != (xb >> (64 - 2 * n))) fail("d_ref_codes", L, g, n); }
                if (okb) {
                    if (!okf) n_codes_ok_new++;
                    for (int j = 0; j < n; j++) if (d_refchar(F, g + j) != "ACGT"[d_codes_field(xb, j, 1)]) { fail("d_ref_codes against d_refchar", L, g, n); break; }
                }
            }
            // ---- mismatch counts of a read window against the text, as characters and as 2-bit + mask words
            {
                unsigned char rd[48];
                const int i0 = (int)((g + 70) % 32);
                for (int k = 0; k < 48; k++) rd[k] = (unsigned char)"ACGT"[rnd() & 3];
                for (int k = 0; k < 8; k++) { const char c = d_refchar(F, g + k); if (c && rnd() % 6) rd[i0 + k] = (unsigned char)c; }
                if (rnd() % 4 == 0) rd[i0 + (int)(rnd() % 8)] = 'N';
                uint32_t words[6] = {0, 0, 0, 0, 0, 0};                   // W2 = 3: 48 bases
                for (int k = 0; k < 48; k++) {
                    const uint8_t c = d_nt4(rd[k]);
                    if (c > 3) words[3 + (k >> 4)] |= 3u << (30 - 2 * (k & 15)); else words[k >> 4] |= (uint32_t)c << (30 - 2 * (k & 15));
                }
                ReadWords rw; rw.w = words; rw.W2 = 3;
                unsigned char ra_b[48];
                memcpy(ra_b, rd, 48);
                if (rnd() % 5 == 0) ra_b[i0 + (int)(rnd() % 8)] = '-';      // (characters only: a packed read never holds one)
                if (rnd() % 5 == 0) ra_b[i0 + (int)(rnd() % 8)] |= 0x20;
                ReadAscii ra; ra.p = ra_b;
                for (int e = 1; e <= 8; e++) {
                    bool d1 = false, d2 = false, d3 = false, d4 = false;
                    n_cmp += 2;
                    if (rw.mismatches8(F, i0, e, g, d1) != rw.mismatches8(B, i0, e, g, d2) || d1 != d2) fail("ReadWords::mismatches8", L, g, e);
                    if (ra.mismatches8(F, i0, e, g, d3) != ra.mismatches8(B, i0, e, g, d4) || d3 != d4) fail("ReadAscii::mismatches8", L, g, e);
                }
            }
            // ---- 64 symbols
            {
                const Text64 xf = d_text64(F, g), xb = d_text64(B, g);
                count(w64, g, 64, L); n_cmp++;
                if (xf.nv != xb.nv || xf.T0 != xb.T0 || xf.T1 != xb.T1 || xf.T2 != xb.T2 || xf.T3 != xb.T3) fail("d_text64", L, g, 64);
                const int64_t left = g >= 0 ? 2 * L - g : 0;
                if (xb.nv != (left >= 64 ? 64 : left > 0 ? (int)left : 0)) fail("d_text64 nv", L, g, 64);
                const uint32_t T[4] = {xb.T0, xb.T1, xb.T2, xb.T3};
                for (int j = 0; j < 64; j++) {
                    const uint32_t c = (T[j >> 4] >> (30 - 2 * (j & 15))) & 3u;
                    const char ch = d_refchar(F, g + j);
                    if (j < xb.nv ? "ACGT"[c] != ch : c != 0u) { fail("d_text64 against d_refchar", L, g, 64); break; }
                }
            }
        }
    }
    printf("second-half bytes built: %ld; comparisons: %ld; d_ref_codes fetched in both forms %ld, only with the second half %ld\n", n_bytes, n_cmp, n_codes_ok_both, n_codes_ok_new);
    const Where *ws[3] = {&w8, &wn, &w64};
    const char *names[3] = {"windows8", "windows1to28", "windows64"};
    for (int k = 0; k < 3; k++)
        printf("%s: straddle_L %ld at_begin %ld at_end %ld first_half %ld second_half %ld outside %ld\n", names[k], ws[k]->straddle_L, ws[k]->at_begin, ws[k]->at_end,
               ws[k]->first_half, ws[k]->second_half, ws[k]->outside);
    printf("bad=%ld\n", bad);
    return bad ? 1 : 0;
}
