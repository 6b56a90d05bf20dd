// tests/native/rnametrics_checks.hip -- the host-callable code of the device's RNA-seq metrics (dart_amd/csrc/dg_rnametrics.h) run on the CPU, lane by lane as the
// kernels apply it: the flattening, a record's filter, blocks and segment walk (k_rm_class), the coverage track's two events per block, their sort (here
// std::stable_sort over the same keys) and the 32-bit scan in workgroup tiles (k_cv_depth, k_tiles_top), the upper-bound depth look-up and the 100 samples of a
// transcript as the 64 lanes of a wave take them (k_rm_body), and the text.
// usage: rnametrics_checks <input> <output.txt> <output.metrics>
//   input       i64 n_chr, exclude_flags, min_mapq, min_cov, n_raw, n_tx, n_exons, n_exons as the annotation claims it; n_tx x dg_rna_tx; n_exons x dg_rna_exon; the records
//   output.txt  per segment "seg <chr> <start> <class> <strands>", "elig <n>", per record "rec <i> <counted> <blocks> <top> <bits> <row>", "bad <i>" for the first
//               record out of range (then no words follow), "words" and the 330
//   exit status 3, the text on stderr: the annotation was refused
#include "../../dart_amd/csrc/dg_rnametrics.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "rnametrics_checks: %s failed (line %d)\n", #x, __LINE__); return 2; } } while (0)

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: rnametrics_checks <input> <output.txt> <output.metrics>\n"); return 1; }
    const bool format_only = !strcmp(argv[1], "--format");      // rnametrics_checks --format <330 u64 words> <output.metrics>: the text alone
    FILE *f = fopen(argv[format_only ? 2 : 1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<unsigned char> in;
    { unsigned char buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + k); fclose(f); }
    if (format_only) {
        CHECK(in.size() == rm_words() * 8);
        std::vector<uint64_t> words(rm_words()); memcpy(words.data(), in.data(), in.size());
        std::string text;
        rm_format(words.data(), text);
        FILE *o = fopen(argv[3], "wb");
        CHECK(o && fwrite(text.data(), 1, text.size(), o) == text.size());
        fclose(o);
        return 0;
    }
    CHECK(in.size() >= 64);
    long long head[8]; memcpy(head, in.data(), 64);
    const int n_chr = (int)head[0]; const CvFilter flt{0u, (uint32_t)head[1], (uint32_t)head[2]};
    const uint64_t min_cov = (uint64_t)head[3], n_raw = (uint64_t)head[4], n_tx = (uint64_t)head[5], n_ex = (uint64_t)head[6], n_ex_claimed = (uint64_t)head[7];
    static_assert(sizeof(dg_rna_tx) == 32 && sizeof(dg_rna_exon) == 8, "the annotation's layout");
    CHECK(in.size() == 64 + n_tx * 32 + n_ex * 8 + n_raw);
    // (exact-size copies on the heap: a read that leaves an array leaves its allocation, which the sanitizer build sees)
    std::vector<dg_rna_tx> txs((size_t)n_tx); if (n_tx) memcpy(txs.data(), in.data() + 64, (size_t)n_tx * 32);
    std::vector<dg_rna_exon> exs((size_t)n_ex); if (n_ex) memcpy(exs.data(), in.data() + 64 + n_tx * 32, (size_t)n_ex * 8);
    std::vector<unsigned char> raw(in.begin() + 64 + (long)(n_tx * 32 + n_ex * 8), in.end());
    dg_rna_annot an; an.n_tx = (uint32_t)n_tx; an.pad = 0; an.n_exons = (size_t)n_ex_claimed; an.tx = txs.data(); an.exons = exs.data();
    RmFlat fl; char why[400];
    if (!rm_flatten(n_chr, &an, fl, why, sizeof why)) { fprintf(stderr, "%s\n", why); return 3; }
    FILE *txt = fopen(argv[2], "w"), *met = fopen(argv[3], "wb");
    CHECK(txt && met);
    CHECK(fl.chr_first.size() == (size_t)n_chr + 1 && fl.seg_cs.size() == fl.seg_start.size() && fl.chr_first[(size_t)n_chr] == fl.seg_start.size());
    for (int c = 0; c < n_chr; c++)
        for (uint32_t i = fl.chr_first[(size_t)c]; i < fl.chr_first[(size_t)c + 1]; i++) {
            CHECK(i == fl.chr_first[(size_t)c] || fl.seg_start[i] > fl.seg_start[i - 1]);
            fprintf(txt, "seg %d %u %u %u\n", c, fl.seg_start[i], fl.seg_cs[i] & 7u, fl.seg_cs[i] >> 8);
        }
    fprintf(txt, "elig %zu\n", fl.tx.size());
    const RmTable t{fl.chr_first.data(), fl.seg_start.data(), fl.seg_cs.data(), n_chr};
    std::vector<uint64_t> at;
    for (uint64_t p = 0; p < n_raw;) { CHECK(p + 4 <= n_raw); at.push_back(p); p += 4ull + bs_le32(raw.data() + p); CHECK(p <= n_raw); }
    const size_t n = at.size();
    std::vector<unsigned long long> w(rm_words(), 0ull);
    // k_rm_class and k_cv_count
    std::vector<uint64_t> first(n + 1, 0);
    uint64_t bad = CV_NONE, kmin = CV_NONE, kmax = 0;
    for (size_t i = 0; i < n; i++) {
        const RmRec r = rm_record(raw.data() + at[i], n_raw - at[i], t, flt);
        const CvRec cr = cv_record(raw.data() + at[i], n_raw - at[i], n_chr, flt);
        CHECK(cr.counted == r.counted);
        uint32_t nb = 0;
        if (r.counted) {
            CvTally ty; ty.aligned = 0; ty.lo = CV_NONE; ty.hi = 0; ty.bad = false;
            nb = cv_blocks(raw.data() + at[i], cr, ty);
            CHECK(nb == r.blocks && ty.bad == r.bad);
            if (r.bad) { if (bad == CV_NONE) bad = i; }
            else {
                unsigned long long sum = 0;
                for (int k = 0; k < RM_CLASSES; k++) { w[rm_off_ba() + k] += r.acc.ba[k]; sum += r.acc.ba[k]; }
                CHECK(sum == ty.aligned && r.acc.top < RM_CLASSES && r.acc.bits < 4u && r.st < 4u);
                w[rm_off_rc() + r.acc.top]++; w[rm_off_st() + r.st]++; w[rm_off_sn() + RM_SN_COUNTED]++; w[rm_off_sn() + RM_SN_BLOCKS] += nb; w[rm_off_sn() + RM_SN_ALIGNED] += sum;
                if (nb) { kmin = std::min(kmin, cv_key(cr.refid, ty.lo)); kmax = std::max(kmax, cv_key(cr.refid, ty.hi)); }
            }
        }
        fprintf(txt, "rec %zu %d %u %u %u %u\n", i, (int)r.counted, nb, r.acc.top, r.acc.bits, r.st);
        first[i + 1] = first[i] + nb;
    }
    if (bad != CV_NONE) { fprintf(txt, "bad %llu\n", (unsigned long long)bad); fclose(txt); fclose(met); return 0; }
    w[rm_off_sn() + RM_SN_RECORDS] = n; w[rm_off_sn() + RM_SN_TX] = n_tx; w[rm_off_sn() + RM_SN_ELIGIBLE] = fl.tx.size(); w[rm_off_sn() + RM_SN_SEGMENTS] = fl.seg_start.size();
    // k_cv_emit, the sort, k_cv_depth in tiles of CV_THREADS with k_tiles_top's exclusive sums
    const uint64_t n_blocks = first[n], n_ev = 2 * n_blocks;
    std::vector<uint64_t> keys((size_t)n_ev, CV_NONE); std::vector<int64_t> vals((size_t)n_ev, 0);
    for (size_t i = 0; i < n; i++) {
        const CvRec r = cv_record(raw.data() + at[i], n_raw - at[i], n_chr, flt);
        if (!r.counted) continue;
        CvEmit e{keys.data(), vals.data(), first[i], n_blocks, r.refid};
        CHECK(cv_blocks(raw.data() + at[i], r, e) == first[i + 1] - first[i]);
    }
    std::vector<uint32_t> order((size_t)n_ev);
    for (uint64_t k = 0; k < n_ev; k++) order[k] = (uint32_t)k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    std::vector<uint64_t> skey((size_t)n_ev); std::vector<uint32_t> incl((size_t)n_ev), dep_base((size_t)((n_ev + CV_THREADS - 1) / CV_THREADS));
    uint32_t total = 0, in_tile = 0;
    for (uint64_t k = 0; k < n_ev; k++) {
        if (k % CV_THREADS == 0) { dep_base[(size_t)(k / CV_THREADS)] = total; in_tile = 0; }
        skey[k] = keys[order[k]]; in_tile += (uint32_t)vals[order[k]]; total += (uint32_t)vals[order[k]]; incl[k] = in_tile;
    }
    CHECK(total == 0u);
    // k_rm_body: a wave per eligible transcript, lane l takes samples l and l + 64
    for (size_t i = 0; i < fl.tx.size(); i++) {
        const RmTx x = fl.tx[i];
        CHECK(x.first + x.n_ex <= fl.ex.size() && x.len >= RM_MIN_LEN);
        const RmExon *e = fl.ex.data() + x.first;
        uint32_t d[RM_BINS]; unsigned long long S = 0;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            const bool two = lane + 64u < RM_BINS;
            const uint32_t g0 = rm_sample_pos(x, e, lane), g1 = rm_sample_pos(x, e, two ? lane + 64u : lane);
            for (uint32_t g : {g0, g1}) {
                bool inside = false;
                for (uint32_t k = 0; k < x.n_ex; k++) inside = inside || (e[k].start <= g && g < e[k].end);
                CHECK(inside);
            }
            uint32_t c0, c1;
            rm_upper2(skey.data(), (uint32_t)n_ev, cv_key(x.chr, g0), cv_key(x.chr, g1), c0, c1);
            // against the plain statement: the number of keys <= key
            CHECK(c0 == (uint32_t)(std::upper_bound(skey.begin(), skey.end(), cv_key(x.chr, g0)) - skey.begin()) && c1 == (uint32_t)(std::upper_bound(skey.begin(), skey.end(), cv_key(x.chr, g1)) - skey.begin()));
            d[lane] = rm_depth_at(incl.data(), dep_base.data(), c0); S += d[lane];
            { uint32_t run = 0; for (uint64_t k = 0; k < n_ev && skey[k] <= cv_key(x.chr, g0); k++) run += (uint32_t)vals[order[k]]; CHECK(d[lane] == run); }      // the plain statement: the deltas in front, summed
            if (two) { d[lane + 64u] = rm_depth_at(incl.data(), dep_base.data(), c1); S += d[lane + 64u]; }
        }
        if (!rm_contributes(S, min_cov)) continue;
        w[rm_off_sn() + RM_SN_CONTRIB]++;
        for (uint32_t b = 0; b < RM_BINS; b++) { w[rm_off_bc() + b] += d[b]; w[rm_off_bc() + RM_BINS + b] += d[b] ? 1u : 0u; w[rm_off_bc() + 2 * RM_BINS + b] += rm_norm(d[b], S); }
    }
    fprintf(txt, "words");
    for (unsigned long long v : w) fprintf(txt, " %llu", v);
    fprintf(txt, "\n");
    std::string text;
    rm_format((const uint64_t *)w.data(), text);
    CHECK(fwrite(text.data(), 1, text.size(), met) == text.size());
    fclose(txt); fclose(met);
    return 0;
}
