// CPU suite: the __host__ __device__ functions of dart_amd/csrc/dg_trim.h -- the rules of the device's trimming stage -- run on the host the way the kernels use
// them: the read packed 64 bases at a time from three bit planes (k_trim_cut's ballots), the quality and poly walks in rounds of 64 steps with a carry and the
// rounds' lane sets, the adapter at every start position through the unaligned extracts of the packed planes (the planes are TR_WORDS long, as in LDS: a
// sanitizer build speaks when an extract at a read's last word leaves them), the mate's verdict, the stored window.  No HIP call.
// argv[1]: i64 two, rc_odd_reads, n1, n2; u32 flags, qual3, qual5, qual_base, min_overlap, max_err_permille, poly_mask, poly_min, min_len, alen0, alen1, 0;
// adapter 0 and 1 (64 bytes each); text1 and text2 (each padded to 8 bytes).  argv[2]: out = i64 n_in (-1: the record counts do not fit), i64 n_kept,
// u64 stats[16], a TrimRead per input read, then per kept read u32 read, name and quality length, then per kept read its stored bases, name and quality.
#include "../../dart_amd/csrc/dg_trim.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

struct Text { std::vector<char> t; uint64_t n = 0; std::vector<uint32_t> line_start; uint64_t n_nl = 0, n_lines = 0; };

static void find_lines(Text &x)
{
    x.line_start.assign(1, 0u);
    for (uint64_t pos = 0; pos < x.n; pos += 16) {
        uint32_t w[4];
        memcpy(w, x.t.data() + pos, 16);
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

#define NONE (-0x40000000)
// a round of a walk as the wave sees it: the running sums of 64 lanes (a lane past the end adds nothing), the lanes that exist
struct Round { int incl[64]; uint64_t valid; };

// k_trim_cut's trim_dev_qual_walk
static int qual_walk(const char *q, uint32_t L, bool from_end, uint32_t cutoff, uint32_t qual_base)
{
    int best = 0, best_t = -1, carry = 0;
    for (uint32_t t0 = 0; t0 < L; t0 += 64) {
        Round r; r.valid = 0;
        uint64_t neg = 0;
        int run = carry;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t t = t0 + lane;
            if (t < L) { r.valid |= 1ull << lane; run += trim_qual_term(cutoff, q[from_end ? L - 1u - t : t], qual_base); if (run < 0) neg |= 1ull << lane; }
            r.incl[lane] = run;
        }
        const uint64_t live = trim_live_lanes(r.valid, neg);
        int mx = NONE;
        for (uint32_t lane = 0; lane < 64; lane++) if (((live >> lane) & 1ull) && r.incl[lane] > mx) mx = r.incl[lane];
        if (mx > best) {
            uint64_t hits = 0;
            for (uint32_t lane = 0; lane < 64; lane++) if (((live >> lane) & 1ull) && r.incl[lane] == mx) hits |= 1ull << lane;
            best = mx; best_t = (int)(t0 + trim_first_lane(hits));
        }
        if (neg) break;
        carry = r.incl[63];
    }
    return best_t;
}

// k_trim_cut's trim_dev_poly_walk
static void poly_walk(const char *s, uint32_t a, uint32_t b, uint32_t c, int &best, int &best_t)
{
    const uint32_t n = b - a;
    int carry = 0;
    best = NONE; best_t = -1;
    for (uint32_t t0 = 0; t0 < n; t0 += 64) {
        Round r; r.valid = 0;
        int run = carry;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t t = t0 + lane;
            if (t < n) { r.valid |= 1ull << lane; run += trim_poly_term(s[b - 1u - t], c); }
            r.incl[lane] = run;
        }
        int mx = NONE;
        for (uint32_t lane = 0; lane < 64; lane++) if (((r.valid >> lane) & 1ull) && r.incl[lane] > mx) mx = r.incl[lane];
        if (mx >= best) {
            uint64_t hits = 0;
            for (uint32_t lane = 0; lane < 64; lane++) if (((r.valid >> lane) & 1ull) && r.incl[lane] == mx) hits |= 1ull << lane;
            best = mx; best_t = (int)(t0 + trim_last_lane(hits));
        }
        carry = r.incl[63];
        if (t0 + 64 < n && trim_poly_hopeless(carry, n - (t0 + 64), best)) break;
    }
}

// k_trim_cut for one read
static TrimRead cut(const char *line1, const char *line3, uint32_t L, uint32_t ql, const TrimPar &par, int ad)
{
    uint64_t *code = (uint64_t *)malloc(TR_WORDS * 8), *mask = (uint64_t *)malloc(TR_WORDS * 8);      // (heap blocks of the planes' exact size: the sanitizer's red zones lie right behind them)
    memset(code, 0xA5, TR_WORDS * 8); memset(mask, 0xA5, TR_WORDS * 8);                                  // what the rounds do not write means nothing
    for (uint32_t i0 = 0; i0 < L; i0 += 64) {
        uint64_t lo = 0, hi = 0, bad = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t c = i0 + lane < L ? trim_code(line1[i0 + lane]) : 4u;
            lo |= (uint64_t)(c & 1u) << lane; hi |= (uint64_t)((c >> 1) & 1u) << lane; bad |= (uint64_t)((c >> 2) & 1u) << lane;
        }
        trim_pack64(lo, hi, bad, code + (i0 >> 5), mask + (i0 >> 5));
    }
    uint32_t a = 0, b = L, cut5 = 0, cut3 = 0, flags = 0;
    if (par.qual3 | par.qual5) {
        if (ql == L) {
            const int t3 = par.qual3 ? qual_walk(line3, L, true, par.qual3, par.qual_base) : -1;
            const int t5 = par.qual5 ? qual_walk(line3, L, false, par.qual5, par.qual_base) : -1;
            trim_qual_window(L, t3, t5, a, b, cut5, cut3);
        } else flags |= TR_F_QSKIP;
    }
    uint32_t ad_cut = 0;
    const uint32_t alen = par.alen[ad];
    if (alen && b - a >= par.min_overlap) {
        const uint32_t last = b - par.min_overlap;
        bool found = false;
        for (uint32_t p0 = a; p0 <= last && !found; p0 += 64) {
            uint64_t hits = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t p = p0 + lane;
                if (p > last) continue;
                const uint32_t n = b - p < alen ? b - p : alen;
                if (trim_adapter_ok(trim_mismatches(code, mask, p, par.acode[ad][0], par.acode[ad][1], n), n, par.max_err_permille)) hits |= 1ull << lane;
            }
            if (hits) { const uint32_t p_hit = p0 + trim_first_lane(hits); ad_cut = b - p_hit; b = p_hit; flags |= TR_F_ADAPTER | (ad ? TR_F_ADAPTER1 : 0); found = true; }
        }
    }
    uint32_t poly_cut = 0;
    if (par.poly_mask && b > a) {
        uint32_t nb = b;
        for (uint32_t c = 0; c < 4; c++) {
            if (!((par.poly_mask >> c) & 1u)) continue;
            int best, best_t;
            poly_walk(line1, a, b, c, best, best_t);
            if (best > 0 && (uint32_t)best_t + 1u >= par.poly_min) { const uint32_t at = b - 1u - (uint32_t)best_t; nb = at < nb ? at : nb; }
        }
        if (nb < b) { poly_cut = b - nb; b = nb; flags |= TR_F_POLY; }
    }
    free(code); free(mask);
    TrimRead r = {(uint16_t)a, (uint16_t)b, (uint16_t)cut5, (uint16_t)cut3, (uint16_t)ad_cut, (uint16_t)poly_cut, (uint16_t)flags, 0};
    return r;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[4]; uint32_t pw[12]; char adapter[2][64];
    if (fread(h, 8, 4, f) != 4 || fread(pw, 4, 12, f) != 12 || fread(adapter, 1, 128, f) != 128) return 2;
    TrimPar par; memset(&par, 0, sizeof par);
    par.flags = pw[0]; par.qual3 = pw[1]; par.qual5 = pw[2]; par.qual_base = pw[3]; par.min_overlap = pw[4]; par.max_err_permille = pw[5]; par.poly_mask = pw[6]; par.poly_min = pw[7];
    par.min_len = pw[8]; par.alen[0] = pw[9]; par.alen[1] = pw[10];
    for (int i = 0; i < 2; i++) for (uint32_t j = 0; j < par.alen[i] && j < 64; j++) par.acode[i][j >> 5] |= (uint64_t)trim_code(adapter[i][j]) << (2u * (j & 31u));
    Text x[2];
    for (int i = 0; i < 2; i++) {
        x[i].n = (uint64_t)h[2 + i];
        x[i].t.assign(((x[i].n + 7) & ~7ull) + 32, (char)0x0A);
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
    if (n < 0) { const int64_t z = 0; fwrite(&z, 8, 1, o); fclose(o); printf("record counts do not fit\n"); return 0; }
    // k_trim_cut
    std::vector<TrimRead> win(n);
    std::vector<FqRecord> recs(n);
    for (int64_t k = 0; k < n; k++) {
        int file; uint32_t rec;
        fq_read_place((uint32_t)k, two, file, rec);
        const Text &t = x[file];
        uint32_t s0, s1, s2, s3;
        const uint32_t l0 = line_len(t, 4ull * rec, s0), l1 = line_len(t, 4ull * rec + 1, s1), l2 = line_len(t, 4ull * rec + 2, s2), l3 = line_len(t, 4ull * rec + 3, s3);
        recs[k] = fq_record(t.t.data(), s0, l0, l1, l2, l3);
        if (recs[k].rlen <= 0 || recs[k].rlen > DG_MAX_RLEN) { fprintf(stderr, "read %lld: the plain upload refuses it\n", (long long)k); return 1; }
        win[k] = cut(t.t.data() + s1, t.t.data() + s3, (uint32_t)recs[k].rlen, recs[k].ql, par, trim_adapter_of((uint32_t)k, two, file, par.flags));
    }
    // k_trim_len and k_trim_write
    uint64_t st[16]; memset(st, 0, sizeof st);
    std::vector<uint32_t> lens; std::vector<char> body;
    int64_t n_kept = 0;
    for (int64_t k = 0; k < n; k++) {
        int file; uint32_t rec;
        fq_read_place((uint32_t)k, two, file, rec);
        const Text &t = x[file];
        const TrimRead w = win[k];
        const bool own = trim_long_enough(w.a, w.b, par.min_len);
        bool mate = true;
        if ((par.flags & DG_TRIM_PAIRS) && (k ^ 1) < n) mate = trim_long_enough(win[k ^ 1].a, win[k ^ 1].b, par.min_len);
        const bool keep = own && mate;
        const uint32_t rl = (uint32_t)w.b - w.a, ql = trim_stored_ql(w.a, w.b, recs[k].ql);
        st[0]++; st[1] += keep; st[2] += (uint64_t)recs[k].rlen; st[3] += keep ? rl : 0; st[4] += w.cut5; st[5] += w.cut3;
        st[6] += (w.flags & TR_F_ADAPTER) && !(w.flags & TR_F_ADAPTER1); st[7] += (w.flags & TR_F_ADAPTER) && (w.flags & TR_F_ADAPTER1); st[8] += w.ad_cut;
        st[9] += (w.flags & TR_F_POLY) != 0; st[10] += w.poly_cut; st[11] += !own; st[12] += own && !mate; st[13] += (w.flags & TR_F_QSKIP) != 0;
        if (!keep) continue;
        win[k].flags |= TR_F_KEEP; n_kept++;
        lens.push_back(rl); lens.push_back(recs[k].hl); lens.push_back(ql);
        const bool rc = fq_stored_rc((uint32_t)k, rc_odd);
        for (uint32_t i = 0; i < rl; i++) body.push_back(fq_stored_base(t.t.data() + recs[k].seq_at + w.a, rl, i, rc));
        for (uint32_t i = 0; i < recs[k].hl; i++) body.push_back(t.t[recs[k].name_at + i]);
        for (uint32_t i = 0; i < ql; i++) body.push_back(fq_stored_qual(t.t.data() + recs[k].qual_at + w.a, ql, i, rc));
    }
    fwrite(&n_kept, 8, 1, o); fwrite(st, 8, 16, o); fwrite(win.data(), 16, n, o); fwrite(lens.data(), 4, lens.size(), o); fwrite(body.data(), 1, body.size(), o);
    fclose(o);
    printf("reads %lld kept %lld\n", (long long)n, (long long)n_kept);
    return 0;
}
