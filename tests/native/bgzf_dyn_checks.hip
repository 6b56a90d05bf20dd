// CPU suite: the __host__ __device__ functions of dart_amd/csrc/dg_bgzf_dyn.h run on the host.
//   deflate <file> <out>        the file as BGZF blocks through the lane functions of k_bgzf_deflate_dyn, in the kernel's order: a strip's lanes (or symbols)
//                               one after the other through each phase, in a scrambled order inside it, a barrier being the end of a loop.  The slot
//                               is filled with a pattern first: a byte behind the block that differs from what the kernel's own zeroing left fails the
//                               run.  The exact cost the choice was made with is compared with the bits the scan adds up.  Prints how often each fork ran:
//                               "dynamic D fixed F stored S repairs R nodist N0 onedist N1 blocks B"
//   lengths <limit> f0 f1 ...   the length builder (rank sort, tree, repair) on a histogram; prints "repaired R" and the lengths
#include "../../dart_amd/csrc/dg_bgzf_dyn.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static std::vector<char> blob;
static bool slurp(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END); blob.resize((size_t)ftell(f) + 8); fseek(f, 0, SEEK_SET);
    const bool ok = fread(blob.data(), 1, blob.size() - 8, f) == blob.size() - 8;
    fclose(f);
    return ok;
}
// the lanes (or symbols) 0 .. n - 1 in an order that differs from phase to phase
static std::vector<uint32_t> order(uint32_t n, uint32_t phase)
{
    std::vector<uint32_t> o(n);
    for (uint32_t i = 0; i < n; i++) o[i] = i;
    uint32_t x = 12345u + 977u * phase;
    for (uint32_t i = n; i > 1; i--) { x = x * 1664525u + 1013904223u; const uint32_t j = (x >> 8) % i; const uint32_t t = o[i - 1]; o[i - 1] = o[j]; o[j] = t; }
    return o;
}

static int deflate_file(const char *in, const char *out)
{
    if (!slurp(in)) return 2;
    const size_t n_total = blob.size() - 8;
    FILE *o = fopen(out, "wb");
    if (!o) return 2;
    BgzfDynLds *sd = new BgzfDynLds;
    BgzfLds &s = sd->b;
    BgzfDyn &d = sd->d;
    std::vector<uint32_t> slot_w(BGZF_SLOT / 4);
    unsigned char *slot = (unsigned char *)slot_w.data();
    unsigned long long n_dyn = 0, n_fixed = 0, n_stored = 0, n_rep = 0, n_d0 = 0, n_d1 = 0, n_blocks = 0;
    int bad = 0;
    for (size_t at = 0; at < n_total; at += BGZF_BLOCK) {
        const uint32_t n = (uint32_t)(n_total - at < BGZF_BLOCK ? n_total - at : BGZF_BLOCK);
        memset(sd, 0xa5, sizeof *sd);                              // what the kernel does not set it must not read
        memset(s.in, 0, sizeof s.in); memcpy(s.in, blob.data() + at, n); memset(s.tab, 0, sizeof s.tab);
        for (auto &w : slot_w) w = 0xdeadbeefu;
        const uint32_t zero_words = (18u + n + 8u + 3u) / 4u + 1u;
        for (uint32_t w = 0; w < zero_words; w++) slot_w[w] = 0;
        for (uint32_t i = 0; i < 256; i++) s.crc_tab[i] = bgzf_crc_entry(i);
        const uint32_t crc = bgzf_crc_bytes(s.crc_tab, (const unsigned char *)s.in, n);
        uint32_t bit_base = 0, phase = 0; bool coded = true;
        for (uint32_t s0 = 0; s0 < n && coded; s0 += BGZF_STRIP) {
            uint32_t nt[BGZF_THREADS], nb[BGZF_THREADS], mine[BGZF_THREADS], incl[BGZF_THREADS], sum = 0;
            auto seg = [&](uint32_t t, uint32_t &a, uint32_t &b) { a = s0 + t * BGZF_SEG; b = a + BGZF_SEG < n ? a + BGZF_SEG : n; };
            for (uint32_t t : order(BGZF_THREADS, phase++)) {
                uint32_t a, b; seg(t, a, b);
                nt[t] = bgzf_lane_tokens(s, t, a, b, nb[t]);
                if (nt[t] > BGZF_SEG) return 3;
            }
            for (uint32_t t = 0; t < BGZF_THREADS; t++) s.len[t] = bgzf_lane_meta(s, t, nt[t]);
            for (uint32_t i = 0; i < BGZF_NSYM; i++) { d.freq[i] = 0; d.len[i] = 0; }
            d.fixed_bits = 0; d.body_bits = 0;
            // (the merge reads the meta words and the lane's own tokens only, the histogram the lane's own tokens: one phase, as in the kernel)
            for (uint32_t t : order(BGZF_THREADS, phase++)) { bgzf_lane_merge(s, s.len, t, nt[t], nb[t]); bgzf_dyn_lane_hist(s, d, t, nt[t], nb[t]); }
            for (uint32_t i : order(BGZF_NSYM, phase++)) bgzf_dyn_lane_rank(d, i);
            bgzf_dyn_build(d, 1); bgzf_dyn_build(d, 0);
            for (uint32_t i : order(BGZF_NSYM, phase++)) bgzf_dyn_lane_code(d, i);
            bgzf_dyn_choose(d);
            const uint32_t cost = d.cost, head_bits = d.head_bits;
            coded = bgzf_dyn_still_coded(bit_base, cost, n);
            if (coded) {
                if (!d.dynamic) for (uint32_t i : order(BGZF_NSYM, phase++)) bgzf_dyn_lane_fixed(d, i);
                for (uint32_t t = 0; t < BGZF_THREADS; t++) { mine[t] = bgzf_dyn_lane_nbits(s, d, t, nt[t]); sum += mine[t]; incl[t] = sum; }
                if (head_bits + sum + (d.code[256] >> 16) != cost) { fprintf(stderr, "strip at %u: the cost was %u, the bits are %u\n", s0, cost, head_bits + sum + (d.code[256] >> 16)); bad++; }
                const uint32_t pos = 18u * 8u + bit_base + head_bits;
                if ((pos - head_bits + cost + 7u) / 8u > 18u + n) { fprintf(stderr, "strip at %u would write past the input's size\n", s0); return 3; }
                bgzf_dyn_put_eob(d, pos + sum, slot_w.data());
                for (uint32_t t : order(BGZF_THREADS, phase++)) if (nt[t]) bgzf_dyn_lane_emit(s, d, t, nt[t], pos + incl[t] - mine[t], slot_w.data());
                bgzf_dyn_put_head(d, 18u * 8u + bit_base, s0 + BGZF_STRIP >= n, slot_w.data());
                if (d.dynamic) n_dyn++; else n_fixed++;
                if (d.dynamic) { n_rep += d.repaired[0] + d.repaired[1] + d.cl_repaired; n_d0 += d.n_used[1] == 0; n_d1 += d.n_used[1] == 1; }
            }
            bit_base += cost;
            for (uint32_t t : order(BGZF_THREADS, phase++)) { uint32_t a, b; seg(t, a, b); bgzf_lane_insert(s, a, b, n); }
        }
        const uint32_t clen = coded ? (bit_base + 7u) / 8u : n + 5u;
        if (!coded) { n_stored++; bgzf_put_stored_head(slot + 18, n); memcpy(slot + 23, s.in, n); }
        const uint32_t bsize = 18u + clen + 8u;
        if (bsize > BGZF_SLOT) return 3;
        bgzf_put_header(slot, bsize);
        bgzf_put_trailer(slot + 18u + clen, crc, n);
        for (uint32_t i = bsize; i < BGZF_SLOT; i++) {
            const unsigned char want = i < 4u * zero_words ? 0 : (unsigned char)(0xdeadbeefu >> (8u * (i & 3u)));
            if (slot[i] != want) { fprintf(stderr, "block at %zu: byte %u behind the block (%u bytes) changed\n", at, i, bsize); bad++; break; }
        }
        fwrite(slot, 1, bsize, o);
        n_blocks++;
    }
    fclose(o);
    delete sd;
    printf("dynamic %llu fixed %llu stored %llu repairs %llu nodist %llu onedist %llu blocks %llu\n", n_dyn, n_fixed, n_stored, n_rep, n_d0, n_d1, n_blocks);
    return bad ? 1 : 0;
}

static int lengths(int argc, char **argv)
{
    const uint32_t limit = (uint32_t)strtoul(argv[2], nullptr, 10), n_sym = (uint32_t)(argc - 3);
    if (limit < 1 || limit > 15 || n_sym < 1 || n_sym > BGZF_HUFF_MAX_SYM) return 2;
    std::vector<uint32_t> freq(n_sym), key(n_sym, 0xa5a5a5a5u), work(n_sym, 0xa5a5a5a5u);
    std::vector<uint8_t> len(n_sym, 0);
    uint32_t cnt[16], next[16], used = 0;
    for (uint32_t i = 0; i < n_sym; i++) { freq[i] = (uint32_t)strtoul(argv[3 + i], nullptr, 10); if (freq[i] > BGZF_HUFF_FREQ_MAX) return 2; }
    for (uint32_t i : order(n_sym, 7)) used = bgzf_huff_rank(freq.data(), n_sym, i, key.data());
    if (used > (1u << limit)) return 2;
    const uint32_t rep = bgzf_huff_build(key.data(), used, limit, work.data(), len.data(), cnt, next);
    printf("repaired %u\n", rep);
    for (uint32_t i = 0; i < n_sym; i++) printf("%u%c", len[i], i + 1 < n_sym ? ' ' : '\n');
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "deflate")) return deflate_file(argv[2], argv[3]);
    if (argc >= 4 && !strcmp(argv[1], "lengths")) return lengths(argc, argv);
    return 2;
}
