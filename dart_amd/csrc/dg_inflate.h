// dg_inflate.h -- BGZF on the device, the other way: the blocked gzip stream `bgzip` and htslib write (and dg_bgzf.h, dg_bgzf_dyn.h) -> its bytes in HBM.
// Every member of such a file carries its own size (the 'BC' subfield), inflates to at most 64 KB and does not depend on its neighbours, so a file is
// thousands of independent jobs: the host hops over the headers (inf_walk_members: where each member's deflate stream lies, what its trailer promises),
//   k_bgzf_inflate  one wave per member, INF_WAVES waves per workgroup: RFC 1951 complete (stored, fixed and dynamic blocks, any number per member),
//                   then the member's length against ISIZE and its CRC32 against the trailer's; a status word per member, the first failing one
//                   (smallest index) in `verdict`.
// A deflate stream is one serial bit string: the wave keeps the bit buffer and the table walks uniform (every lane computes the same values; what is
// read back from LDS goes through readfirstlane) and uses its 64 lanes where there is width:
//   the input     a window of INF_WIN bytes in LDS, a word per lane, refilled when the bit buffer has drunk it; bytes behind in_len read as zero and
//                 every taking of bits is checked against in_len, so input that ends early is reported and never read past
//   the tables    code lengths -> per-length counts and the symbols in canonical order (lane 0, a few hundred steps), then a first-level table of
//                 INF_ROOT_L / INF_ROOT_D bits, lane = entry: each entry decodes its own index canonically.  A code longer than the root takes the
//                 canonical walk over the counts (rare: the overflow path needs no second-level tables)
//   the output    tokens are decoded INF_ROUND at a time into LDS; then the literals go out side by side (lane = token) and every match 64 bytes a
//                 step, a source byte behind the match's start taken modulo the distance (distance 1, length 258: 258 copies of one byte)
//   the CRC       lane = piece, combined pairwise (dg_bgzf.h's functions)
// What zlib's inflate refuses is refused here with the same verdict: the status names the first rule that failed (INF_E_*).  A malformed member never
// reads outside its in_len input bytes or writes outside its isize output bytes: every store is checked against isize before it is queued.
// LDS: sizeof(InfLds) = 5.4 KB per wave.  No inline assembly, no per-lane arrays.
// The whole member -- inf_member and what it calls -- is __host__ __device__: on the host the lane loops run one lane after the other
// (tests/native/inflate_checks.hip runs them against zlib, also under the sanitizers).
#ifndef DG_INFLATE_H
#define DG_INFLATE_H
#include "dg_bgzf.h"
#include <vector>

#define INF_HD __host__ __device__ __forceinline__
#define INF_WAVES 4              // members per workgroup
#define INF_ROUND 128u           // tokens decoded before the lanes write them out
#define INF_WIN 256u             // bytes of input in LDS: a word per lane
#define INF_ROOT_L 10u           // bits of the first-level table: literal / length
#define INF_ROOT_D 8u            // ... distance
#define INF_MAX_ISIZE 65536u

// the first rule a member broke (zlib's message where it has one)
enum { INF_OK = 0,
       INF_E_BTYPE = 1,          // "invalid block type"
       INF_E_STORED = 2,         // "invalid stored block lengths"
       INF_E_SYMBOLS = 3,        // "too many length or distance symbols"
       INF_E_CODELEN_SET = 4,    // "invalid code lengths set"
       INF_E_REPEAT = 5,         // "invalid bit length repeat"
       INF_E_NO_EOB = 6,         // "invalid code -- missing end-of-block"
       INF_E_LITLEN_SET = 7,     // "invalid literal/lengths set"
       INF_E_DIST_SET = 8,       // "invalid distances set"
       INF_E_LITLEN_CODE = 9,    // "invalid literal/length code"
       INF_E_DIST_CODE = 10,     // "invalid distance code"
       INF_E_FAR = 11,           // "invalid distance too far back"
       INF_E_INPUT = 12,         // the input ends before the final block does
       INF_E_ISIZE = 13,         // the stream's length is not the trailer's ISIZE
       INF_E_CRC = 14,           // the bytes' CRC32 is not the trailer's
       INF_E_N };
INF_HD const char *inf_rule(uint32_t st)
{
    switch (st) {
    case INF_OK: return "ok";
    case INF_E_BTYPE: return "invalid block type";
    case INF_E_STORED: return "invalid stored block lengths";
    case INF_E_SYMBOLS: return "too many length or distance symbols";
    case INF_E_CODELEN_SET: return "invalid code lengths set";
    case INF_E_REPEAT: return "invalid bit length repeat";
    case INF_E_NO_EOB: return "invalid code -- missing end-of-block";
    case INF_E_LITLEN_SET: return "invalid literal/lengths set";
    case INF_E_DIST_SET: return "invalid distances set";
    case INF_E_LITLEN_CODE: return "invalid literal/length code";
    case INF_E_DIST_CODE: return "invalid distance code";
    case INF_E_FAR: return "invalid distance too far back";
    case INF_E_INPUT: return "the input ends before the final block";
    case INF_E_ISIZE: return "the stream's length is not ISIZE";
    case INF_E_CRC: return "CRC32 mismatch";
    default: return "unknown";
    }
}

// one member: its deflate stream in the compressed bytes, its place in the output, what its trailer says
struct InfBlock { unsigned long long in_off, out_off; uint32_t in_len, isize, crc, pad; };

struct InfLds {                                  // one wave's
    uint32_t win[INF_WIN / 4];                   // input bytes [wbase, wbase + INF_WIN)
    uint32_t tok[INF_ROUND];                     // a round's tokens (dg_bgzf.h's form: a literal is its byte; bit 31: a match) ...
    uint16_t pos[INF_ROUND];                     // ... and where in the output each begins (< 65536)
    uint16_t fast_l[1u << INF_ROOT_L];           // low bits of the bit buffer -> code length << 9 | symbol; 0: no code this short
    uint16_t fast_d[1u << INF_ROOT_D];
    uint16_t sym_l[288], sym_d[32], sym_c[20];   // symbols in canonical order (by length, then by value)
    uint16_t cnt_l[16], cnt_d[16], cnt_c[16];    // codes per length
    uint16_t offs[16];
    uint8_t lens[320];                           // code lengths as the block's header gives them: literal / length, then distance
    uint32_t crc[64], clen[64];
};

// ---- the wave on the device, the lanes one after the other on the host ----
static uint32_t inf_host_lane_xor = 0;           // host only: the order of the lanes inside a phase; any value below 64 must give the same bytes
#if defined(__HIP_DEVICE_COMPILE__)
#define INF_LANES(l) for (uint32_t l = threadIdx.x & 63u, l##_once = 1u; l##_once; l##_once = 0u)
#define INF_LANE0 if ((threadIdx.x & 63u) == 0u)
// LDS operations of a wave complete in order: what a lane wrote is there for the others once the compiler keeps the order
#define INF_SYNC_LDS() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
// bytes in HBM a lane wrote, read by another lane of the wave
#define INF_SYNC_MEM() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)
INF_HD uint32_t inf_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
#else
#define INF_LANES(l) for (uint32_t l##_i = 0, l = inf_host_lane_xor; l##_i < 64u; l##_i++, l = l##_i ^ inf_host_lane_xor)
#define INF_LANE0
#define INF_SYNC_LDS() do { } while (0)
#define INF_SYNC_MEM() do { } while (0)
INF_HD uint32_t inf_uni(uint32_t v) { return v; }
#endif

// ---- the bit string ----
struct InfBits {
    const unsigned char *in; uint32_t in_len;
    uint64_t bb; uint32_t bn;                    // the buffer: bn bits, the next one in bit 0 (bits behind the input's end are zeros)
    uint32_t rp;                                 // the input byte the buffer is fed from next (a multiple of 4)
    uint32_t wbase;                              // the window's first byte
    uint32_t used, total;                        // bits taken, bits there are
};
// window <- bytes [base, base + INF_WIN) of the input, zeros behind in_len
INF_HD void inf_fill(InfLds &s, const InfBits &b, uint32_t base)
{
    INF_SYNC_LDS();
    INF_LANES(lane) {
        const uint32_t i0 = base + 4u * lane;
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4u; k++) if (i0 + k < b.in_len) w |= (uint32_t)b.in[i0 + k] << (8u * k);
        s.win[lane] = w;
    }
    INF_SYNC_LDS();
}
// afterwards the buffer holds at least 33 bits
INF_HD void inf_refill(InfLds &s, InfBits &b)
{
    if (b.bn <= 32u) {
        if (b.rp - b.wbase >= INF_WIN) { b.wbase = b.rp; inf_fill(s, b, b.wbase); }
        const uint32_t w = inf_uni(s.win[(b.rp - b.wbase) >> 2]);
        b.bb |= (uint64_t)w << b.bn; b.bn += 32u; b.rp += 4u;
    }
}
INF_HD void inf_seek(InfLds &s, InfBits &b, uint32_t bitpos)
{
    b.used = bitpos; b.rp = (bitpos >> 3) & ~3u; b.bb = 0; b.bn = 0;
    const uint32_t drop = bitpos - 8u * b.rp;
    inf_refill(s, b);
    b.bb >>= drop; b.bn -= drop;
}
INF_HD void inf_drop(InfBits &b, uint32_t n) { b.bb >>= n; b.bn -= n; b.used += n; }
// n <= 16 bits; false: the input ends first
INF_HD bool inf_take(InfLds &s, InfBits &b, uint32_t n, uint32_t &v)
{
    inf_refill(s, b);
    if (b.used + n > b.total) return false;
    v = (uint32_t)b.bb & ((1u << n) - 1u);
    inf_drop(b, n);
    return true;
}

// ---- Huffman codes ----
// The code of `bits` (first bit in bit 0) among codes of up to maxlen bits: its symbol and length, or 0xffff / 0 when the bits are no code.
// UNI: called with the same bits in every lane (what comes from LDS is made uniform)
template <bool UNI>
INF_HD uint32_t inf_canon(const uint16_t *cnt, const uint16_t *sym, uint32_t bits, uint32_t maxlen, uint32_t &len)
{
    int32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= maxlen; l++) {
        code |= (int32_t)(bits & 1u); bits >>= 1;
        const int32_t c = (int32_t)inf_uni(cnt[l]);            // (the same in every lane either way)
        if (code - c < first) { len = l; const uint32_t v = sym[index + (code - first)]; return UNI ? inf_uni(v) : v; }
        index += c; first += c; first <<= 1; code <<= 1;
    }
    len = 0;
    return 0xffffu;
}
// lens[0, n) -> cnt[1..15] and sym[]; returns 0: a complete code, -1: over-subscribed, 1: incomplete with one code of length 1 (zlib lets a literal /
// length or distance code be that), 2: incomplete otherwise, 3: no code at all
INF_HD int inf_code(InfLds &s, uint32_t from, uint32_t n, uint16_t *cnt, uint16_t *sym)
{
    INF_SYNC_LDS();
    INF_LANE0 {
        for (uint32_t l = 0; l < 16u; l++) cnt[l] = 0;
        for (uint32_t i = 0; i < n; i++) cnt[s.lens[from + i] & 15u]++;
        cnt[0] = 0;
        s.offs[1] = 0;
        for (uint32_t l = 1; l < 15u; l++) s.offs[l + 1] = (uint16_t)(s.offs[l] + cnt[l]);
        for (uint32_t i = 0; i < n; i++) { const uint32_t l = s.lens[from + i] & 15u; if (l) sym[s.offs[l]++] = (uint16_t)i; }
    }
    INF_SYNC_LDS();
    int32_t left = 1; uint32_t maxl = 0;
    for (uint32_t l = 1; l < 16u; l++) {
        const int32_t c = (int32_t)inf_uni(cnt[l]);
        left = 2 * left - c;
        if (left < 0) return -1;
        if (c) maxl = l;
    }
    if (maxl == 0) return 3;
    if (left > 0) return maxl == 1u ? 1 : 2;
    return 0;
}
// the first-level table: lane = entry
INF_HD void inf_fast(const uint16_t *cnt, const uint16_t *sym, uint16_t *fast, uint32_t root)
{
    INF_LANES(lane) for (uint32_t i = lane; i < (1u << root); i += 64u) {
        uint32_t len;
        const uint32_t sy = inf_canon<false>(cnt, sym, i, root, len);
        fast[i] = len ? (uint16_t)((len << 9) | sy) : (uint16_t)0;
    }
    INF_SYNC_LDS();
}
// the next symbol of the bit buffer (at least 15 bits of it are looked at); len = 0: the bits are no code
INF_HD uint32_t inf_sym(const uint16_t *fast, uint32_t root, const uint16_t *cnt, const uint16_t *sym, uint32_t bits, uint32_t &len)
{
    const uint32_t e = inf_uni(fast[bits & ((1u << root) - 1u)]);
    if (e) { len = e >> 9; return e & 511u; }
    return inf_canon<true>(cnt, sym, bits, 15u, len);
}
// RFC 1951 3.2.5: length symbol 257..285 -> base and extra bits; distance symbol 0..29 likewise
INF_HD void inf_len_base(uint32_t sy, uint32_t &base, uint32_t &eb)
{
    if (sy < 265u) { base = sy - 254u; eb = 0; return; }
    if (sy == 285u) { base = 258u; eb = 0; return; }
    const uint32_t k = sy - 261u;
    eb = k >> 2; base = 3u + ((4u + (k & 3u)) << eb);
}
INF_HD void inf_dist_base(uint32_t sy, uint32_t &base, uint32_t &eb)
{
    if (sy < 4u) { base = sy + 1u; eb = 0; return; }
    eb = (sy >> 1) - 1u; base = 1u + ((2u + (sy & 1u)) << eb);
}
// the order in which a dynamic block's header lists the lengths of the code-length code, five bits each
INF_HD uint32_t inf_clc_order(uint32_t i)
{
    // 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return i < 12u ? (uint32_t)(lo >> (5u * i)) & 31u : (uint32_t)(hi >> (5u * (i - 12u))) & 31u;
}

// both tables from s.lens[0, nlen) and s.lens[nlen, nlen + ndist): zlib's verdicts on the two sets
INF_HD uint32_t inf_tables(InfLds &s, uint32_t nlen, uint32_t ndist)
{
    int v = inf_code(s, 0, nlen, s.cnt_l, s.sym_l);
    if (v == -1 || v == 2 || v == 3) return INF_E_LITLEN_SET;
    v = inf_code(s, nlen, ndist, s.cnt_d, s.sym_d);
    if (v == -1 || v == 2) return INF_E_DIST_SET;                // (3: no distance code at all is a legal block of literals)
    inf_fast(s.cnt_l, s.sym_l, s.fast_l, INF_ROOT_L);
    inf_fast(s.cnt_d, s.sym_d, s.fast_d, INF_ROOT_D);
    return INF_OK;
}
INF_HD uint32_t inf_fixed_tables(InfLds &s)
{
    INF_SYNC_LDS();
    INF_LANES(lane) for (uint32_t i = lane; i < 320u; i += 64u) s.lens[i] = (uint8_t)(i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : i < 288u ? 8u : 5u);
    return inf_tables(s, 288u, 32u);                             // (symbols 286, 287 and distances 30, 31 have codes; meeting one is the error)
}
// the header of a dynamic block
INF_HD uint32_t inf_dynamic_tables(InfLds &s, InfBits &b)
{
    uint32_t v;
    if (!inf_take(s, b, 14u, v)) return INF_E_INPUT;
    const uint32_t nlen = (v & 31u) + 257u, ndist = ((v >> 5) & 31u) + 1u, ncode = (v >> 10) + 4u;
    if (nlen > 286u || ndist > 30u) return INF_E_SYMBOLS;
    INF_SYNC_LDS();
    INF_LANES(lane) if (lane < 19u) s.lens[lane] = 0;
    INF_SYNC_LDS();
    for (uint32_t i = 0; i < ncode; i++) {
        if (!inf_take(s, b, 3u, v)) return INF_E_INPUT;
        INF_LANE0 s.lens[inf_clc_order(i)] = (uint8_t)v;
    }
    if (inf_code(s, 0, 19u, s.cnt_c, s.sym_c) != 0) return INF_E_CODELEN_SET;
    uint32_t have = 0, prev = 0;
    while (have < nlen + ndist) {
        inf_refill(s, b);
        uint32_t len;
        const uint32_t sy = inf_canon<true>(s.cnt_c, s.sym_c, (uint32_t)b.bb, 7u, len);
        if (!len || b.used + len > b.total) return INF_E_INPUT;  // (the code is complete: bits that are no code do not exist)
        inf_drop(b, len);
        uint32_t rep = 1, val = sy;
        if (sy == 16u) { if (!have) return INF_E_REPEAT; if (!inf_take(s, b, 2u, v)) return INF_E_INPUT; rep = 3u + v; val = prev; }
        else if (sy == 17u) { if (!inf_take(s, b, 3u, v)) return INF_E_INPUT; rep = 3u + v; val = 0; }
        else if (sy == 18u) { if (!inf_take(s, b, 7u, v)) return INF_E_INPUT; rep = 11u + v; val = 0; }
        if (have + rep > nlen + ndist) return INF_E_REPEAT;
        INF_LANES(lane) for (uint32_t i = lane; i < rep; i += 64u) s.lens[have + i] = (uint8_t)val;
        have += rep; prev = val;
    }
    INF_SYNC_LDS();
    if (inf_uni(s.lens[256]) == 0) return INF_E_NO_EOB;
    return inf_tables(s, nlen, ndist);
}

// the tokens of a fixed or dynamic block from the tables in s: decoded a round at a time, written by the lanes; opos: the output's length so far
INF_HD uint32_t inf_tokens(InfLds &s, InfBits &b, unsigned char *out, uint32_t isize, uint32_t &opos)
{
    for (;;) {
        uint32_t nt = 0, p = opos;
        bool eob = false;
        while (nt < INF_ROUND) {
            inf_refill(s, b);
            uint32_t len, base, eb;
            uint32_t sy = inf_sym(s.fast_l, INF_ROOT_L, s.cnt_l, s.sym_l, (uint32_t)b.bb, len);
            if (!len) return b.used >= b.total ? INF_E_INPUT : INF_E_LITLEN_CODE;
            if (b.used + len > b.total) return INF_E_INPUT;
            inf_drop(b, len);
            uint32_t tok;
            uint32_t adv = 1u;
            if (sy < 256u) tok = sy;
            else if (sy == 256u) { eob = true; break; }
            else {
                if (sy > 285u) return INF_E_LITLEN_CODE;
                inf_len_base(sy, base, eb);
                if (b.used + eb > b.total) return INF_E_INPUT;
                const uint32_t mlen = base + ((uint32_t)b.bb & ((1u << eb) - 1u));
                inf_drop(b, eb);
                inf_refill(s, b);
                sy = inf_sym(s.fast_d, INF_ROOT_D, s.cnt_d, s.sym_d, (uint32_t)b.bb, len);
                if (!len) return b.used >= b.total ? INF_E_INPUT : INF_E_DIST_CODE;
                if (b.used + len > b.total) return INF_E_INPUT;
                inf_drop(b, len);
                if (sy > 29u) return INF_E_DIST_CODE;
                inf_dist_base(sy, base, eb);
                if (b.used + eb > b.total) return INF_E_INPUT;
                const uint32_t dist = base + ((uint32_t)b.bb & ((1u << eb) - 1u));
                inf_drop(b, eb);
                if (dist > p) return INF_E_FAR;
                tok = bgzf_tok_match(mlen, dist); adv = mlen;
            }
            if (p + adv > isize) return INF_E_ISIZE;               // nothing is ever stored behind the member's slot
            INF_LANE0 { s.tok[nt] = tok; s.pos[nt] = (uint16_t)p; }
            nt++; p += adv;
        }
        // the round's bytes: literals side by side, then the matches in their order (a match may copy what the round has just written)
        INF_SYNC_LDS();
        INF_LANES(lane) for (uint32_t t = lane; t < nt; t += 64u) { const uint32_t tok = s.tok[t]; if (!(tok >> 31)) out[s.pos[t]] = (unsigned char)tok; }
        for (uint32_t t = 0; t < nt; t++) {
            const uint32_t tok = inf_uni(s.tok[t]);
            if (!(tok >> 31)) continue;
            const uint32_t mlen = ((tok >> 15) & 0xffu) + 3u, dist = (tok & 0x7fffu) + 1u, at = inf_uni(s.pos[t]);
            INF_SYNC_MEM();
            INF_LANES(lane) for (uint32_t i = lane; i < mlen; i += 64u) out[at + i] = out[at - dist + (i < dist ? i : i % dist)];
        }
        opos = p;
        if (eob) return INF_OK;
    }
}

// One member: in_len bytes of deflate stream -> isize bytes at out; crc_tab: 256 entries of bgzf_crc_entry.  Returns INF_OK or the first rule broken.
INF_HD uint32_t inf_member(InfLds &s, const uint32_t *crc_tab, const unsigned char *in, uint32_t in_len, unsigned char *out, uint32_t isize, uint32_t crc)
{
    InfBits b;
    b.in = in; b.in_len = in_len; b.total = 8u * in_len; b.wbase = 0x80000000u;
    inf_seek(s, b, 0);
    uint32_t opos = 0;
    bool fixed_ready = false;
    for (;;) {
        uint32_t hdr;
        if (!inf_take(s, b, 3u, hdr)) return INF_E_INPUT;
        const uint32_t last = hdr & 1u, type = hdr >> 1;
        if (type == 3u) return INF_E_BTYPE;
        if (type == 0u) {
            uint32_t v, len, nlen;
            if (!inf_take(s, b, (8u - (b.used & 7u)) & 7u, v) || !inf_take(s, b, 16u, len) || !inf_take(s, b, 16u, nlen)) return INF_E_INPUT;
            if ((len ^ 0xffffu) != nlen) return INF_E_STORED;
            const uint32_t at = b.used >> 3;
            if (at + len > in_len) return INF_E_INPUT;
            if (opos + len > isize) return INF_E_ISIZE;
            INF_LANES(lane) for (uint32_t i = lane; i < len; i += 64u) out[opos + i] = in[at + i];
            opos += len;
            inf_seek(s, b, b.used + 8u * len);
        } else {
            uint32_t st = INF_OK;
            if (type == 1u) { if (!fixed_ready) st = inf_fixed_tables(s); fixed_ready = true; }
            else { fixed_ready = false; st = inf_dynamic_tables(s, b); }
            if (st) return st;
            st = inf_tokens(s, b, out, isize, opos);
            if (st) return st;
        }
        if (last) break;
    }
    if (opos != isize) return INF_E_ISIZE;
    // CRC32: every lane its piece, combined pairwise
    INF_SYNC_MEM();
    const uint32_t per = (isize + 63u) / 64u;
    INF_LANES(lane) {
        const uint32_t lo = lane * per < isize ? lane * per : isize, hi = lo + per < isize ? lo + per : isize;
        s.crc[lane] = bgzf_crc_bytes(crc_tab, out + lo, hi - lo); s.clen[lane] = hi - lo;
    }
    for (uint32_t st = 1; st < 64u; st <<= 1) {
        INF_SYNC_LDS();
        INF_LANES(lane) if ((lane & (2u * st - 1u)) == 0u) {
            s.crc[lane] = bgzf_crc_combine(s.crc[lane], s.crc[lane + st], s.clen[lane + st]);
            s.clen[lane] += s.clen[lane + st];
        }
    }
    INF_SYNC_LDS();
    return inf_uni(s.crc[0]) == crc ? INF_OK : INF_E_CRC;
}

// ------------------------------------------------------------------------------------------
// the kernel
// ------------------------------------------------------------------------------------------
// status[i]: member i's verdict; verdict: the smallest (index << 8 | status) of a failing member (the caller sets it to all ones)
__global__ void __launch_bounds__(64 * INF_WAVES)
k_bgzf_inflate(const unsigned char *__restrict__ in, const InfBlock *__restrict__ tab, uint32_t n_blocks, unsigned char *out, uint32_t *__restrict__ status,
               unsigned long long *__restrict__ verdict)
{
    __shared__ InfLds s[INF_WAVES];
    __shared__ uint32_t crc_tab[256];
    for (uint32_t i = threadIdx.x; i < 256u; i += 64u * INF_WAVES) crc_tab[i] = bgzf_crc_entry(i);
    __syncthreads();
    const uint32_t w = threadIdx.x >> 6, blk = blockIdx.x * INF_WAVES + w;
    if (blk >= n_blocks) return;
    const InfBlock b = tab[blk];
    const uint32_t st = inf_member(s[w], crc_tab, in + b.in_off, inf_uni(b.in_len), out + b.out_off, inf_uni(b.isize), inf_uni(b.crc));
    if ((threadIdx.x & 63u) == 0u) { status[blk] = st; if (st) atomicMin(verdict, ((unsigned long long)blk << 8) | st); }
}

// ------------------------------------------------------------------------------------------
// the host's part: hopping over the members (RFC 1952 with the SAM specification's 'BC' subfield)
// ------------------------------------------------------------------------------------------
// Members of p[0, n) -> tab (in_off counted from in_base, out_off from out_base on); *n_out: the sum of their ISIZEs.  Returns nullptr, or what is wrong with
// member *bad: nothing is appended for it.
static inline const char *inf_walk_members(const unsigned char *p, size_t n, unsigned long long in_base, unsigned long long out_base, std::vector<InfBlock> &tab, size_t *n_out, size_t *bad)
{
    size_t at = 0, total = 0, k = 0;
    while (at < n) {
        *bad = k;
        if (n - at < 12 || p[at] != 0x1f || p[at + 1] != 0x8b || p[at + 2] != 8) return "bytes that are no gzip member";
        if (p[at + 3] != 4) return "FLG is not FEXTRA alone";
        const size_t xlen = (size_t)p[at + 10] | (size_t)p[at + 11] << 8;
        if (n - at - 12 < xlen) return "the extra field runs past the input";
        size_t bsize = 0;
        for (size_t x = at + 12, xe = at + 12 + xlen; x + 4 <= xe;) {
            const size_t slen = (size_t)p[x + 2] | (size_t)p[x + 3] << 8;
            if (xe - x - 4 < slen) break;
            if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2) { bsize = ((size_t)p[x + 4] | (size_t)p[x + 5] << 8) + 1; break; }
            x += 4 + slen;
        }
        if (!bsize) return "no BC subfield";
        if (bsize > n - at) return "BSIZE points past the input";
        if (bsize < 12 + xlen + 8) return "BSIZE is smaller than the member's header and trailer";
        const unsigned char *t = p + at + bsize - 8;
        const uint32_t crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        const uint32_t isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        if (isize > INF_MAX_ISIZE) return "ISIZE is above 65536";
        InfBlock b;
        b.in_off = in_base + at + 12 + xlen; b.in_len = (uint32_t)(bsize - 12 - xlen - 8); b.out_off = out_base + total; b.isize = isize; b.crc = crc; b.pad = 0;
        tab.push_back(b);
        total += isize; at += bsize; k++;
    }
    *n_out = total;
    return nullptr;
}
#endif
