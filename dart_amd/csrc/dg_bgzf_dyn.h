// dg_bgzf_dyn.h -- the BGZF coder of dg_bgzf.h with dynamic Huffman codes: every strip of a block (BGZF_STRIP input bytes) is a deflate block of its
// own, coded with the smaller of a Huffman code built from the strip's own tokens (BTYPE = 10) and the fixed code (BTYPE = 01); BFINAL on the last.
// The parse is dg_bgzf.h's (bgzf_lane_tokens / _meta / _merge / _insert), so a block's tokens are those of k_bgzf_deflate; the whole-block stored
// fallback and the n + 31 bound stay.  A strip, behind the merge pass:
//   histogram    LDS atomic adds: 286 literal / length counters (the end-of-block symbol once), 30 distance counters, the strip's bits in the fixed code
//   sort         every used symbol finds the rank of its (frequency, symbol) key among its alphabet's keys: all lanes, no order among them matters
//   lengths      one lane per alphabet (two waves): the in-place Moffat-Katajainen tree over the sorted frequencies, the lengths folded into counts per
//                length, the counts repaired to the 15-bit limit (Kraft sum back to 1), the lengths handed out again longest to rarest
//   codes        canonical: first code per length, a symbol's rank among the symbols of its length, bit-reversed; and freq * (length + extra bits)
//   header       one lane: HLIT / HDIST / HCLEN, the two length arrays run-length coded (symbols 16, 17, 18), the 7-bit-limited code of those
//                symbols, the header's bits; the dynamic cost is then exact, the fixed cost is the fixed bits + 3 + 7; dynamic only when smaller
//   stay-coded   the chosen cost against the input's size BEFORE anything of the strip is written; else the block goes out stored
//   emit         the chosen code lies in the LDS tables (a fixed strip fills them with the fixed code): scan of the lanes' bits, whole words by plain
//                stores, a lane's first and last word by OR; the next strip continues at the next bit, the stream is padded once, at its end
// Integers only, ties broken by the symbol's index: the host runs the same functions lane after lane (tests/native/bgzf_dyn_checks.hip) and gets the
// kernel's bytes.  LDS: BgzfLds (134,160 B) + BgzfDyn (7,408 B) = 141,568 B of the CU's 160 KB: still one workgroup per CU.
#ifndef DG_BGZF_DYN_H
#define DG_BGZF_DYN_H
#include "dg_bgzf.h"

#define BGZF_NLL 286u                       // literal / length symbols
#define BGZF_ND 30u                         // distance symbols
#define BGZF_NSYM (BGZF_NLL + BGZF_ND)      // both alphabets in one array: distance symbol k at BGZF_NLL + k
#define BGZF_NCL 19u                        // code-length symbols
#define BGZF_HUFF_KEY_BITS 9                // a sort key is freq << 9 | symbol
#define BGZF_HUFF_FREQ_MAX 0x7fffffu        // so a frequency has 23 bits (a strip's are at most 8193)
#define BGZF_HUFF_MAX_SYM 320u              // the most symbols dg_probe_huff_lengths takes

struct BgzfDyn {
    uint32_t freq[BGZF_NSYM];               // the strip's histogram
    uint32_t key[BGZF_NSYM];                // per alphabet: the used symbols' keys, ascending
    uint32_t work[BGZF_NSYM];               // per alphabet: the tree builder's array
    uint32_t code[BGZF_NSYM];               // the chosen code: bits (first bit in bit 0) | length << 16
    uint32_t hdr[BGZF_NSYM];                // the run-length coded lengths: code-length symbol | extra value << 5
    uint8_t len[BGZF_HUFF_MAX_SYM];         // the dynamic code's lengths
    uint32_t cnt[2][16], next[2][16];       // per alphabet: symbols per length, first code per length
    uint32_t n_used[2], repaired[2];
    uint32_t fixed_bits, body_bits;         // the strip's tokens in the fixed code; tokens + end of block in the dynamic code
    uint32_t cl_freq[BGZF_NCL], cl_key[BGZF_NCL], cl_work[BGZF_NCL], cl_code[BGZF_NCL], cl_cnt[16], cl_next[16];
    uint8_t cl_len[BGZF_NCL + 1];
    uint32_t n_hdr, hlit, hdist, hclen, hdr_bits, cl_repaired;
    uint32_t dynamic, head_bits, cost;      // the choice; the bits in front of the strip's tokens; head + tokens + end of block
};
struct BgzfDynLds { BgzfLds b; BgzfDyn d; };

BGZF_HD void bgzf_add(uint32_t *w, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(w, v);
#else
    *w += v;
#endif
}

// ---- bits into the zeroed slot: the first and the last word of a writer by OR, the words between -- all its own -- by plain stores ----
struct BgzfSink { uint32_t *slot_w; uint64_t acc; uint32_t w, nacc; bool first; };
BGZF_HD void bgzf_sink_open(BgzfSink &k, uint32_t *slot_w, uint32_t pos) { k.slot_w = slot_w; k.acc = 0; k.w = pos >> 5; k.nacc = pos & 31u; k.first = true; }
BGZF_HD void bgzf_sink_put(BgzfSink &k, uint32_t v, uint32_t nb)       // nb <= 32
{
    k.acc |= (uint64_t)v << k.nacc; k.nacc += nb;
    if (k.nacc >= 32u) {
        if (k.first) { bgzf_or(&k.slot_w[k.w], (uint32_t)k.acc); k.first = false; } else k.slot_w[k.w] = (uint32_t)k.acc;
        k.acc >>= 32; k.nacc -= 32u; k.w++;
    }
}
BGZF_HD void bgzf_sink_close(BgzfSink &k) { if (k.nacc) bgzf_or(&k.slot_w[k.w], (uint32_t)k.acc); }

// ---- code lengths ----
// symbol i's key to its rank among the used symbols' keys; returns the number of used symbols (every lane finds the same)
BGZF_HD uint32_t bgzf_huff_rank(const uint32_t *freq, uint32_t n_sym, uint32_t i, uint32_t *key)
{
    const uint32_t mine = (freq[i] << BGZF_HUFF_KEY_BITS) | i;
    uint32_t rank = 0, used = 0;
    for (uint32_t j = 0; j < n_sym; j++) {
        const uint32_t f = freq[j];
        if (!f) continue;
        used++;
        if (((f << BGZF_HUFF_KEY_BITS) | j) < mine) rank++;
    }
    if (freq[i]) key[rank] = mine;
    return used;
}
// The lengths of a Huffman code for the n used symbols in key[] (ascending), none above `limit`; A: n words of workspace; len[symbol] is written for the
// used symbols only; cnt[l] = symbols of length l, next[l] = the first canonical code of length l (l = 1..limit, 16 words each).  One used symbol gets
// length 1.  Returns 1 when lengths had to be cut to the limit.  Needs n <= 2^limit.
BGZF_HD uint32_t bgzf_huff_build(const uint32_t *key, uint32_t n_used, uint32_t limit, uint32_t *A, uint8_t *len, uint32_t *cnt, uint32_t *next)
{
    const int n = (int)n_used, lim = (int)limit;
    uint32_t over = 0;
    for (int l = 0; l < 16; l++) { cnt[l] = 0; next[l] = 0; }
    if (n == 0) return 0;
    if (n == 1) cnt[1] = 1;
    else {
        // Moffat and Katajainen, "In-place calculation of minimum-redundancy codes": A = the frequencies, then parent links, then depths
        for (int i = 0; i < n; i++) A[i] = key[i] >> BGZF_HUFF_KEY_BITS;
        A[0] += A[1];
        int root = 0, leaf = 2;
        for (int nx = 1; nx < n - 1; nx++) {
            if (leaf >= n || A[root] < A[leaf]) { A[nx] = A[root]; A[root++] = (uint32_t)nx; } else A[nx] = A[leaf++];
            if (leaf >= n || (root < nx && A[root] < A[leaf])) { A[nx] += A[root]; A[root++] = (uint32_t)nx; } else A[nx] += A[leaf++];
        }
        A[n - 2] = 0;
        for (int nx = n - 3; nx >= 0; nx--) A[nx] = A[A[nx]] + 1u;
        int avbl = 1, used = 0, dpth = 0, nx = n - 1;
        root = n - 2;
        while (avbl > 0) {
            while (root >= 0 && (int)A[root] == dpth) { used++; root--; }
            while (avbl > used) { A[nx--] = (uint32_t)dpth; avbl--; }
            avbl = 2 * used; dpth++; used = 0;
        }
        for (int i = 0; i < n; i++) { int l = (int)A[i]; if (l > lim) { l = lim; over = 1; } cnt[l]++; }
        if (over) {
            // the Kraft sum in units of 2^-limit is above 2^limit: every round gives up one code of the limit's length and splits the deepest shorter code
            uint32_t total = 0;
            for (int l = 1; l <= lim; l++) total += cnt[l] << (lim - l);
            while (total > (1u << lim)) {
                cnt[lim]--;
                for (int l = lim - 1; l > 0; l--) if (cnt[l]) { cnt[l]--; cnt[l + 1] += 2u; break; }
                total--;
            }
        }
    }
    int i = 0;
    for (int l = lim; l >= 1; l--) for (uint32_t c = 0; c < cnt[l]; c++) len[key[i++] & ((1u << BGZF_HUFF_KEY_BITS) - 1u)] = (uint8_t)l;
    uint32_t code = 0;
    for (int l = 1; l <= lim; l++) { code = (code + cnt[l - 1]) << 1; next[l] = code; }
    return over;
}
// inflaters want at least two codes in the distance code and a complete code-length code: a second (or a first and a second) symbol of length 1, the lowest
// unused ones; the first codes per length stay what they are (zero)
BGZF_HD void bgzf_huff_two(uint8_t *len, uint32_t n_used)
{
    if (n_used >= 2u) return;
    if (n_used == 0) { len[0] = 1; len[1] = 1; return; }
    len[len[0] ? 1 : 0] = 1;
}
// symbol i's canonical code, bit-reversed, | length << 16; 0 for an unused symbol
BGZF_HD uint32_t bgzf_huff_code(const uint8_t *len, const uint32_t *next, uint32_t i)
{
    const uint32_t l = len[i];
    if (!l) return 0;
    uint32_t c = next[l];
    for (uint32_t j = 0; j < i; j++) c += len[j] == l ? 1u : 0u;
    return bgzf_rev(c, (int)l) | (l << 16);
}

// ---- a lane's part of the phases of a strip ----
// extra bits behind symbol i of BgzfDyn's arrays
BGZF_HD uint32_t bgzf_dyn_extra(uint32_t i)
{
    if (i < 265u) return 0;
    if (i < 285u) return (i - 261u) >> 2;
    if (i < BGZF_NLL + 4u) return 0;
    return ((i - BGZF_NLL) >> 1) - 1u;
}
// histogram: the lane's nt tokens (after the merge), their nbits in the fixed code; lane 0 counts the end-of-block symbol
BGZF_HD void bgzf_dyn_lane_hist(const BgzfLds &s, BgzfDyn &d, uint32_t lane, uint32_t nt, uint32_t nbits)
{
    for (uint32_t i = 0; i < nt; i++) {
        const uint32_t tok = s.tok[i * BGZF_THREADS + lane];
        if (!(tok & 0x80000000u)) { bgzf_add(&d.freq[tok & 0xffu], 1u); continue; }
        uint32_t code, eb, ev;
        bgzf_len_code(((tok >> 15) & 0xffu) + 3u, code, eb, ev);
        bgzf_add(&d.freq[code], 1u);
        bgzf_dist_code((tok & 0x7fffu) + 1u, code, eb, ev);
        bgzf_add(&d.freq[BGZF_NLL + code], 1u);
    }
    if (nbits) bgzf_add(&d.fixed_bits, nbits);
    if (lane == 0) bgzf_add(&d.freq[256], 1u);
}
// sort: symbol i (0 .. BGZF_NSYM - 1) into its alphabet's key array
BGZF_HD void bgzf_dyn_lane_rank(BgzfDyn &d, uint32_t i)
{
    if (i < BGZF_NLL) { const uint32_t u = bgzf_huff_rank(d.freq, BGZF_NLL, i, d.key); if (i == 0) d.n_used[0] = u; }
    else { const uint32_t u = bgzf_huff_rank(d.freq + BGZF_NLL, BGZF_ND, i - BGZF_NLL, d.key + BGZF_NLL); if (i == BGZF_NLL) d.n_used[1] = u; }
}
// lengths: alphabet 0 = literal / length, 1 = distance (one lane each)
BGZF_HD void bgzf_dyn_build(BgzfDyn &d, uint32_t which)
{
    const uint32_t o = which ? BGZF_NLL : 0u;
    d.repaired[which] = bgzf_huff_build(d.key + o, d.n_used[which], 15u, d.work + o, d.len + o, d.cnt[which], d.next[which]);
    if (which) bgzf_huff_two(d.len + o, d.n_used[1]);
}
// codes: symbol i's entry of the table, and its share of the strip's bits
BGZF_HD void bgzf_dyn_lane_code(BgzfDyn &d, uint32_t i)
{
    const uint32_t which = i < BGZF_NLL ? 0u : 1u, o = which ? BGZF_NLL : 0u;
    const uint32_t e = bgzf_huff_code(d.len + o, d.next[which], i - o);
    d.code[i] = e;
    if (d.freq[i]) bgzf_add(&d.body_bits, d.freq[i] * ((e >> 16) + bgzf_dyn_extra(i)));
}
BGZF_HD uint32_t bgzf_cl_order(uint32_t k) { const unsigned char o[BGZF_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15}; return o[k]; }
BGZF_HD uint32_t bgzf_cl_extra(uint32_t sym) { return sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u; }
// header and choice (one lane): the run-length coded lengths, their code, the costs, the verdict
BGZF_HD void bgzf_dyn_choose(BgzfDyn &d)
{
    uint32_t hlit = BGZF_NLL, hdist = BGZF_ND;
    while (hlit > 257u && !d.len[hlit - 1u]) hlit--;
    while (hdist > 1u && !d.len[BGZF_NLL + hdist - 1u]) hdist--;
    const uint32_t total = hlit + hdist;
    for (uint32_t k = 0; k < BGZF_NCL; k++) { d.cl_freq[k] = 0; d.cl_len[k] = 0; }
    uint32_t nh = 0;
#define BGZF_DYN_L(k) ((uint32_t)d.len[(k) < hlit ? (k) : BGZF_NLL + (k) - hlit])
#define BGZF_DYN_EMIT(sym, extra) { d.hdr[nh++] = (uint32_t)(sym) | ((uint32_t)(extra) << 5); d.cl_freq[sym]++; }
    for (uint32_t k = 0; k < total;) {
        const uint32_t v = BGZF_DYN_L(k);
        uint32_t run = 1;
        while (k + run < total && BGZF_DYN_L(k + run) == v) run++;
        k += run;
        if (!v) {
            while (run >= 11u) { const uint32_t t = run < 138u ? run : 138u; BGZF_DYN_EMIT(18u, t - 11u); run -= t; }
            if (run >= 3u) { BGZF_DYN_EMIT(17u, run - 3u); run = 0; }
        } else {
            BGZF_DYN_EMIT(v, 0u); run--;
            while (run >= 3u) { const uint32_t t = run < 6u ? run : 6u; BGZF_DYN_EMIT(16u, t - 3u); run -= t; }
        }
        for (; run; run--) BGZF_DYN_EMIT(v, 0u);
    }
#undef BGZF_DYN_L
#undef BGZF_DYN_EMIT
    // the code of the code-length symbols: 19 keys sorted by insertion, at most 7 bits
    uint32_t nk = 0;
    for (uint32_t sym = 0; sym < BGZF_NCL; sym++) {
        if (!d.cl_freq[sym]) continue;
        const uint32_t key = (d.cl_freq[sym] << BGZF_HUFF_KEY_BITS) | sym;
        uint32_t at = nk++;
        for (; at > 0 && d.cl_key[at - 1u] > key; at--) d.cl_key[at] = d.cl_key[at - 1u];
        d.cl_key[at] = key;
    }
    d.cl_repaired = bgzf_huff_build(d.cl_key, nk, 7u, d.cl_work, d.cl_len, d.cl_cnt, d.cl_next);
    bgzf_huff_two(d.cl_len, nk);
    uint32_t hclen = BGZF_NCL, bits = 5u + 5u + 4u;
    while (hclen > 4u && !d.cl_len[bgzf_cl_order(hclen - 1u)]) hclen--;
    bits += 3u * hclen;
    for (uint32_t sym = 0; sym < BGZF_NCL; sym++) {
        d.cl_code[sym] = bgzf_huff_code(d.cl_len, d.cl_next, sym);
        bits += d.cl_freq[sym] * ((uint32_t)d.cl_len[sym] + bgzf_cl_extra(sym));
    }
    d.n_hdr = nh; d.hlit = hlit; d.hdist = hdist; d.hclen = hclen; d.hdr_bits = bits;
    const uint32_t dyn_cost = 3u + bits + d.body_bits, fixed_cost = 3u + d.fixed_bits + 7u;
    d.dynamic = dyn_cost < fixed_cost ? 1u : 0u;            // fixed on a tie
    d.head_bits = d.dynamic ? 3u + bits : 3u;
    d.cost = d.dynamic ? dyn_cost : fixed_cost;
}
// a fixed strip: entry i of the table from the fixed code
BGZF_HD void bgzf_dyn_lane_fixed(BgzfDyn &d, uint32_t i)
{
    if (i < BGZF_NLL) { uint32_t n; const uint32_t b = bgzf_litlen_bits(i, n); d.code[i] = b | (n << 16); }
    else d.code[i] = bgzf_rev(i - BGZF_NLL, 5) | (5u << 16);
}
// the strip's verdict: with the chosen cost behind the bit_base bits of the strips before, is the stream, padded to a byte, still smaller than the input?
BGZF_HD bool bgzf_dyn_still_coded(uint32_t bit_base, uint32_t cost, uint32_t n) { return (bit_base + cost + 7u) / 8u < n; }
// the bits of the lane's tokens in the table's code
BGZF_HD uint32_t bgzf_dyn_lane_nbits(const BgzfLds &s, const BgzfDyn &d, uint32_t lane, uint32_t nt)
{
    uint32_t n = 0;
    for (uint32_t i = 0; i < nt; i++) {
        const uint32_t tok = s.tok[i * BGZF_THREADS + lane];
        if (!(tok & 0x80000000u)) { n += d.code[tok & 0xffu] >> 16; continue; }
        uint32_t code, eb, ev;
        bgzf_len_code(((tok >> 15) & 0xffu) + 3u, code, eb, ev);
        n += (d.code[code] >> 16) + eb;
        bgzf_dist_code((tok & 0x7fffu) + 1u, code, eb, ev);
        n += (d.code[BGZF_NLL + code] >> 16) + eb;
    }
    return n;
}
// emit: the lane's tokens from bit `pos` of the slot on
BGZF_HD void bgzf_dyn_lane_emit(const BgzfLds &s, const BgzfDyn &d, uint32_t lane, uint32_t nt, uint32_t pos, uint32_t *slot_w)
{
    BgzfSink k;
    bgzf_sink_open(k, slot_w, pos);
    for (uint32_t i = 0; i < nt; i++) {
        const uint32_t tok = s.tok[i * BGZF_THREADS + lane];
        if (!(tok & 0x80000000u)) { const uint32_t e = d.code[tok & 0xffu]; bgzf_sink_put(k, e & 0xffffu, e >> 16); continue; }
        uint32_t code, eb, ev, e;
        bgzf_len_code(((tok >> 15) & 0xffu) + 3u, code, eb, ev);
        e = d.code[code];
        bgzf_sink_put(k, (e & 0xffffu) | (ev << (e >> 16)), (e >> 16) + eb);            // at most 15 + 5 bits
        bgzf_dist_code((tok & 0x7fffu) + 1u, code, eb, ev);
        e = d.code[BGZF_NLL + code];
        bgzf_sink_put(k, (e & 0xffffu) | (ev << (e >> 16)), (e >> 16) + eb);            // at most 15 + 13 bits
    }
    bgzf_sink_close(k);
}
// the strip's head from bit `pos` on (one lane): BFINAL, BTYPE, and for a dynamic strip the header bgzf_dyn_choose laid out
BGZF_HD void bgzf_dyn_put_head(const BgzfDyn &d, uint32_t pos, bool final, uint32_t *slot_w)
{
    BgzfSink k;
    bgzf_sink_open(k, slot_w, pos);
    bgzf_sink_put(k, (final ? 1u : 0u) | (d.dynamic ? 4u : 2u), 3u);
    if (d.dynamic) {
        bgzf_sink_put(k, d.hlit - 257u, 5u); bgzf_sink_put(k, d.hdist - 1u, 5u); bgzf_sink_put(k, d.hclen - 4u, 4u);
        for (uint32_t i = 0; i < d.hclen; i++) bgzf_sink_put(k, d.cl_len[bgzf_cl_order(i)], 3u);
        for (uint32_t i = 0; i < d.n_hdr; i++) {
            const uint32_t sym = d.hdr[i] & 31u, e = d.cl_code[sym];
            bgzf_sink_put(k, (e & 0xffffu) | ((d.hdr[i] >> 5) << (e >> 16)), (e >> 16) + bgzf_cl_extra(sym));      // at most 7 + 7 bits
        }
    }
    bgzf_sink_close(k);
}
// the end-of-block code at bit `pos` (one lane)
BGZF_HD void bgzf_dyn_put_eob(const BgzfDyn &d, uint32_t pos, uint32_t *slot_w)
{
    BgzfSink k;
    bgzf_sink_open(k, slot_w, pos);
    bgzf_sink_put(k, d.code[256] & 0xffffu, d.code[256] >> 16);
    bgzf_sink_close(k);
}

// where a block's time goes (dg_probe_bgzf_phases): lane 0's clock between the barriers, summed over the strips and the blocks
enum { BGZF_PH_PARSE, BGZF_PH_SORT, BGZF_PH_LENGTHS, BGZF_PH_CODES, BGZF_PH_HEADER, BGZF_PH_EMIT, BGZF_PH_INSERT, BGZF_PH_REST, BGZF_PHASES };
#define BGZF_DYN_MARK(ph) { if (phases && tid == 0) { const unsigned long long t_now = (unsigned long long)clock64(); atomicAdd(&phases[ph], t_now - t_mark); t_mark = t_now; } }

// k_bgzf_deflate's arguments, geometry (one workgroup of BGZF_THREADS lanes per block, a BGZF_SLOT-byte slot) and CRC; phases: NULL, or BGZF_PHASES sums of clocks
__global__ void __launch_bounds__(BGZF_THREADS)
k_bgzf_deflate_dyn(const unsigned char *__restrict__ in, unsigned long long n_total, unsigned char *__restrict__ slots, uint64_t *__restrict__ size_scan, uint32_t *__restrict__ size,
                   unsigned long long *__restrict__ phases)
{
    __shared__ BgzfDynLds sd;
    BgzfLds &s = sd.b;
    BgzfDyn &d = sd.d;
    const uint32_t tid = threadIdx.x;
    const unsigned long long at = (unsigned long long)blockIdx.x * BGZF_BLOCK;
    const uint32_t n = (uint32_t)(n_total - at < BGZF_BLOCK ? n_total - at : BGZF_BLOCK);
    unsigned char *slot = slots + (size_t)blockIdx.x * BGZF_SLOT;
    uint32_t *slot_w = (uint32_t *)slot;
    const uint32_t *src = (const uint32_t *)(in + at);
    unsigned long long t_mark = phases ? (unsigned long long)clock64() : 0ull;

    for (uint32_t w = tid; w < BGZF_IN_WORDS; w += BGZF_THREADS) {
        uint32_t v = 0;
        if (4u * w < n) { v = src[w]; if (4u * w + 4u > n) v &= 0xffffffffu >> (8u * (4u * w + 4u - n)); }
        s.in[w] = v;
    }
    const uint32_t zero_words = (18u + n + 8u + 3u) / 4u + 1u;                // < BGZF_SLOT / 4; the coded form ends before byte 18 + n
    for (uint32_t w = tid; w < zero_words; w += BGZF_THREADS) slot_w[w] = 0;
    for (uint32_t w = tid; w < (1u << BGZF_HASH_BITS); w += BGZF_THREADS) s.tab[w] = 0;
    s.crc_tab[tid] = bgzf_crc_entry(tid);
    __syncthreads();
    const unsigned char *inb = (const unsigned char *)s.in;

    {
        const uint32_t per = (n + BGZF_THREADS - 1) / BGZF_THREADS;
        const uint32_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
        s.scan[tid] = bgzf_crc_bytes(s.crc_tab, inb + lo, hi - lo);
        s.len[tid] = hi - lo;
        __syncthreads();
        for (uint32_t st = 1; st < BGZF_THREADS; st <<= 1) {
            if ((tid & (2u * st - 1u)) == 0) {
                s.scan[tid] = bgzf_crc_combine(s.scan[tid], s.scan[tid + st], s.len[tid + st]);
                s.len[tid] += s.len[tid + st];
            }
            __syncthreads();
        }
    }
    const uint32_t crc = s.scan[0];
    __syncthreads();
    BGZF_DYN_MARK(BGZF_PH_REST)

    uint32_t bit_base = 0;                                  // bits of the stream before the current strip
    bool coded = true;
    for (uint32_t s0 = 0; s0 < n && coded; s0 += BGZF_STRIP) {
        const uint32_t a = s0 + tid * BGZF_SEG;
        const uint32_t b = a + BGZF_SEG < n ? a + BGZF_SEG : n;
        uint32_t nbits = 0;
        uint32_t nt = bgzf_lane_tokens(s, tid, a, b, nbits);
        s.len[tid] = bgzf_lane_meta(s, tid, nt);
        for (uint32_t i = tid; i < BGZF_NSYM; i += BGZF_THREADS) { d.freq[i] = 0; d.len[i] = 0; }
        if (tid == 0) { d.fixed_bits = 0; d.body_bits = 0; }
        __syncthreads();
        bgzf_lane_merge(s, s.len, tid, nt, nbits);
        bgzf_dyn_lane_hist(s, d, tid, nt, nbits);
        __syncthreads();
        BGZF_DYN_MARK(BGZF_PH_PARSE)
        for (uint32_t i = tid; i < BGZF_NSYM; i += BGZF_THREADS) bgzf_dyn_lane_rank(d, i);
        __syncthreads();
        BGZF_DYN_MARK(BGZF_PH_SORT)
        if (tid == 0) bgzf_dyn_build(d, 0);
        if (tid == 64) bgzf_dyn_build(d, 1);
        __syncthreads();
        BGZF_DYN_MARK(BGZF_PH_LENGTHS)
        for (uint32_t i = tid; i < BGZF_NSYM; i += BGZF_THREADS) bgzf_dyn_lane_code(d, i);
        __syncthreads();
        BGZF_DYN_MARK(BGZF_PH_CODES)
        if (tid == 0) bgzf_dyn_choose(d);
        __syncthreads();
        BGZF_DYN_MARK(BGZF_PH_HEADER)
        const uint32_t cost = d.cost, head_bits = d.head_bits;
        // before anything of the strip is written: nothing is written once the coded form stops paying, and nothing past the slot
        coded = bgzf_dyn_still_coded(bit_base, cost, n);
        if (coded) {
            if (!d.dynamic) for (uint32_t i = tid; i < BGZF_NSYM; i += BGZF_THREADS) bgzf_dyn_lane_fixed(d, i);
            __syncthreads();
            const uint32_t mine = bgzf_dyn_lane_nbits(s, d, tid, nt);
            s.scan[tid] = mine;
            __syncthreads();
            for (uint32_t o = 1; o < BGZF_THREADS; o <<= 1) {
                const uint32_t t = tid >= o ? s.scan[tid - o] : 0u;
                __syncthreads();
                s.scan[tid] += t;
                __syncthreads();
            }
            const uint32_t pos = 18u * 8u + bit_base + head_bits;
            if (nt) bgzf_dyn_lane_emit(s, d, tid, nt, pos + s.scan[tid] - mine, slot_w);
            if (tid == 0) bgzf_dyn_put_head(d, 18u * 8u + bit_base, s0 + BGZF_STRIP >= n, slot_w);
            if (tid == BGZF_THREADS - 1) bgzf_dyn_put_eob(d, pos + s.scan[BGZF_THREADS - 1], slot_w);
        }
        BGZF_DYN_MARK(BGZF_PH_EMIT)                         // (lane 0 writes the header too: its own end, the other lanes' tail falls to the next phase)
        bit_base += cost;
        bgzf_lane_insert(s, a, b, n);
        __syncthreads();
        BGZF_DYN_MARK(BGZF_PH_INSERT)
    }
    const uint32_t clen = coded ? (bit_base + 7u) / 8u : n + 5u;
    __syncthreads();                                        // the coder's words are in the slot before the bytes around them
    if (!coded) {
        if (tid == 0) bgzf_put_stored_head(slot + 18, n);
        for (uint32_t i = tid; i < n; i += BGZF_THREADS) slot[23u + i] = inb[i];
    }
    if (tid == 0) {
        const uint32_t bsize = 18u + clen + 8u;
        bgzf_put_header(slot, bsize);
        bgzf_put_trailer(slot + 18u + clen, crc, n);
        size[blockIdx.x] = bsize; size_scan[blockIdx.x] = bsize;
    }
    BGZF_DYN_MARK(BGZF_PH_REST)
}
#undef BGZF_DYN_MARK

// dg_probe_huff_lengths: the length builder on a caller's histogram, one workgroup
__global__ void __launch_bounds__(BGZF_THREADS)
k_probe_huff(const uint32_t *__restrict__ freq, uint32_t n_sym, uint32_t limit, unsigned char *__restrict__ len_out)
{
    __shared__ uint32_t f[BGZF_HUFF_MAX_SYM], key[BGZF_HUFF_MAX_SYM], work[BGZF_HUFF_MAX_SYM], cnt[16], next[16], n_used;
    __shared__ uint8_t len[BGZF_HUFF_MAX_SYM];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < n_sym; i += BGZF_THREADS) { f[i] = freq[i]; len[i] = 0; }
    __syncthreads();
    for (uint32_t i = tid; i < n_sym; i += BGZF_THREADS) { const uint32_t u = bgzf_huff_rank(f, n_sym, i, key); if (i == 0) n_used = u; }
    __syncthreads();
    if (tid == 0) (void)bgzf_huff_build(key, n_used, limit, work, len, cnt, next);
    __syncthreads();
    for (uint32_t i = tid; i < n_sym; i += BGZF_THREADS) len_out[i] = len[i];
}
#endif
