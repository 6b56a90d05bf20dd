// dg_bgzf.h -- BGZF on the device: a byte array in HBM -> the blocked gzip stream a BAM file is made of (SAM specification 4.1).
// The array is cut into blocks of BGZF_BLOCK (0xff00) input bytes; one workgroup compresses one block into a 64 KB slot of its own:
//   k_bgzf_deflate  the 18-byte gzip / 'BC' header, ONE raw deflate block (fixed Huffman codes, LZ77 with distances up to 32768), CRC32, ISIZE;
//                   a block whose coded form is not smaller than its input is written as a stored deflate block (input + 31 bytes)
//   k_tiles_top     (dg_wgscan.h) the exclusive scan of the block sizes, the total
//   k_bgzf_copy     slot -> its place in the contiguous stream
// The match search is made so that the bytes never depend on timing: the block is walked in strips of BGZF_STRIP bytes, a strip is cut into
// BGZF_SEG-byte segments (lane = segment).  A lane takes its segment greedily, serially; its candidates are
//   distance 1, distance BGZF_STRIP (the same offset in the previous strip), and the hash table's entry for the next four bytes,
// and the table holds positions of EARLIER strips only: the strip's own positions are inserted behind a barrier, with an LDS atomic max (the
// largest position wins whatever the order of the lanes).  A lane's match ends with its segment; a segment that is one whole match at its predecessor's
// distance is then absorbed into the predecessor's token (bgzf_lane_merge), so a token's length runs up to 258 within a strip.
// A strip's tokens wait in LDS for the workgroup scan of their bit counts, then go to the zeroed slot as whole words; the first and last word
// of a lane, which it may share with its neighbours, by atomic OR.
// LDS: 64 KB input + 32 KB tokens + 32 KB table + 3 KB = 131 KB of the CU's 160: one workgroup (four waves) per CU.
// The serial pieces -- a token's bits, the length and distance codes, CRC32 and its combination, a lane's part of every phase -- are __host__ __device__: the CPU suite runs them
// (tests/native/bam_lane_checks.hip) against zlib.
#ifndef DG_BGZF_H
#define DG_BGZF_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BGZF_HD __host__ __device__ __forceinline__
#define BGZF_BLOCK 0xff00u       // input bytes per block (htslib's BGZF_BLOCK_SIZE)
#define BGZF_SLOT 65536u         // a block's slot: no BGZF block is larger
#define BGZF_THREADS 256
#define BGZF_SEG 32u             // bytes a lane codes serially; a match never crosses a segment's end
#define BGZF_STRIP (BGZF_THREADS * BGZF_SEG)
#define BGZF_HASH_BITS 13
#define BGZF_OVERHEAD 31u        // header 18 + stored block 5 + CRC32 and ISIZE 8: the most a block adds to its input

// ---- tokens: a literal is its byte; a match is bit 31 | (length - 3) << 15 | (distance - 1) ----
BGZF_HD uint32_t bgzf_tok_match(uint32_t len, uint32_t dist) { return 0x80000000u | ((len - 3u) << 15) | (dist - 1u); }
BGZF_HD uint32_t bgzf_rev(uint32_t v, int n) { uint32_t r = 0; for (int i = 0; i < n; i++) { r = (r << 1) | (v & 1u); v >>= 1; } return r; }
BGZF_HD int bgzf_log2(uint32_t v) { int k = 0; while (v >>= 1) k++; return k; }
// RFC 1951 3.2.5: length 3..258 -> code 257..285, its number of extra bits and their value
BGZF_HD void bgzf_len_code(uint32_t len, uint32_t &code, uint32_t &ebits, uint32_t &eval)
{
    const uint32_t l = len - 3u;
    if (l < 8u) { code = 257u + l; ebits = 0; eval = 0; return; }
    if (len == 258u) { code = 285u; ebits = 0; eval = 0; return; }
    ebits = (uint32_t)bgzf_log2(l) - 2u;
    code = 261u + 4u * ebits + ((l >> ebits) & 3u);
    eval = l & ((1u << ebits) - 1u);
}
// distance 1..32768 -> code 0..29
BGZF_HD void bgzf_dist_code(uint32_t dist, uint32_t &code, uint32_t &ebits, uint32_t &eval)
{
    const uint32_t x = dist - 1u;
    if (x < 4u) { code = x; ebits = 0; eval = 0; return; }
    const uint32_t k = (uint32_t)bgzf_log2(x);
    ebits = k - 1u;
    code = 2u * k + ((x >> ebits) & 1u);
    eval = x & ((1u << ebits) - 1u);
}
// the fixed Huffman code of a literal / length symbol (RFC 1951 3.2.6) as deflate packs it: first bit of the code in bit 0
BGZF_HD uint32_t bgzf_litlen_bits(uint32_t sym, uint32_t &n)
{
    if (sym < 144u) { n = 8; return bgzf_rev(0x30u + sym, 8); }
    if (sym < 256u) { n = 9; return bgzf_rev(0x190u + (sym - 144u), 9); }
    if (sym < 280u) { n = 7; return bgzf_rev(sym - 256u, 7); }
    n = 8; return bgzf_rev(0xC0u + (sym - 280u), 8);
}
// a token's bits (at most 31), first bit in bit 0
BGZF_HD uint32_t bgzf_token_bits(uint32_t tok, uint32_t &nbits)
{
    if (!(tok & 0x80000000u)) return bgzf_litlen_bits(tok & 0xffu, nbits);
    uint32_t code, eb, ev, n;
    bgzf_len_code(((tok >> 15) & 0xffu) + 3u, code, eb, ev);
    uint32_t bits = bgzf_litlen_bits(code, n);
    bits |= ev << n; n += eb;
    bgzf_dist_code((tok & 0x7fffu) + 1u, code, eb, ev);
    bits |= bgzf_rev(code, 5) << n; n += 5u;
    bits |= ev << n; n += eb;
    nbits = n;
    return bits;
}
BGZF_HD uint32_t bgzf_token_nbits(uint32_t tok) { uint32_t n; (void)bgzf_token_bits(tok, n); return n; }

// ---- CRC32 (the gzip polynomial, reflected: bit 31 is x^0) ----
BGZF_HD uint32_t bgzf_crc_entry(uint32_t i) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xedb88320u : c >> 1; return c; }
BGZF_HD uint32_t bgzf_crc_mul(uint32_t a, uint32_t b)         // a * b mod P
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        if ((a >> i) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}
BGZF_HD uint32_t bgzf_crc_xpow8(uint32_t len)                 // x^(8 len) mod P
{
    uint32_t r = 0x80000000u, base = 0x00800000u;
    for (; len; len >>= 1) { if (len & 1u) r = bgzf_crc_mul(r, base); base = bgzf_crc_mul(base, base); }
    return r;
}
// CRC32 of A followed by B from the two CRCs and B's length
BGZF_HD uint32_t bgzf_crc_combine(uint32_t crc_a, uint32_t crc_b, uint32_t len_b) { return bgzf_crc_mul(crc_a, bgzf_crc_xpow8(len_b)) ^ crc_b; }
// CRC32 of a buffer, byte by byte through a 256-entry table the caller made with bgzf_crc_entry
BGZF_HD uint32_t bgzf_crc_bytes(const uint32_t *table, const unsigned char *p, uint32_t n)
{
    uint32_t c = 0xffffffffu;
    for (uint32_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return c ^ 0xffffffffu;
}
// the bytes in front of and behind a block's deflate stream; bsize = the whole block's size
BGZF_HD void bgzf_put_header(unsigned char *p, uint32_t bsize)
{
    const unsigned char hd[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int i = 0; i < 16; i++) p[i] = hd[i];
    p[16] = (unsigned char)(bsize - 1u); p[17] = (unsigned char)((bsize - 1u) >> 8);
}
BGZF_HD void bgzf_put_trailer(unsigned char *p, uint32_t crc, uint32_t isize)
{
    for (int k = 0; k < 4; k++) { p[k] = (unsigned char)(crc >> (8 * k)); p[4 + k] = (unsigned char)(isize >> (8 * k)); }
}

// ------------------------------------------------------------------------------------------
// the kernels
// ------------------------------------------------------------------------------------------
#define BGZF_IN_WORDS (BGZF_SLOT / 4 + 4)

struct BgzfLds {
    uint32_t in[BGZF_IN_WORDS];                     // the block, zeros behind its end
    uint32_t tok[BGZF_SEG * BGZF_THREADS];          // the strip's tokens: token i of lane l at [i * BGZF_THREADS + l]
    uint32_t tab[1u << BGZF_HASH_BITS];             // hash of four bytes -> position + 1 of their last occurrence in earlier strips, 0 = none
    uint32_t scan[BGZF_THREADS];
    uint32_t crc_tab[256];
    uint32_t len[BGZF_THREADS];
};

BGZF_HD uint32_t bgzf_ld4(const uint32_t *in, uint32_t p)
{
    const uint32_t w = p >> 2, s = (p & 3u) * 8u;
    return (uint32_t)((((uint64_t)in[w + 1] << 32) | in[w]) >> s);
}
BGZF_HD uint32_t bgzf_match_len(const uint32_t *in, uint32_t c, uint32_t p, uint32_t maxl)
{
    uint32_t l = 0;
    while (l < maxl) {
        const uint32_t x = bgzf_ld4(in, c + l) ^ bgzf_ld4(in, p + l);
        if (x) { l += (uint32_t)__builtin_ctz(x) >> 3; break; }
        l += 4u;
    }
    return l < maxl ? l : maxl;
}
BGZF_HD uint32_t bgzf_hash(uint32_t v) { return (v * 2654435761u) >> (32 - BGZF_HASH_BITS); }
// the two read-modify-write operations of the kernel; on the host (the CPU suite runs the lanes one after the other) they are plain
BGZF_HD void bgzf_or(uint32_t *w, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(w, v);
#else
    *w |= v;
#endif
}
BGZF_HD void bgzf_max(uint32_t *w, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(w, v);
#else
    if (v > *w) *w = v;
#endif
}

// A lane's part of the three phases of a strip (between them: the workgroup's barriers and the scan of the bit counts).
// phase 1: the tokens of segment [a, b) into the lane's column of s.tok, greedily; returns their number, nbits = their bits
BGZF_HD uint32_t bgzf_lane_tokens(BgzfLds &s, uint32_t lane, uint32_t a, uint32_t b, uint32_t &nbits)
{
    const unsigned char *inb = (const unsigned char *)s.in;
    uint32_t nt = 0;
    nbits = 0;
    for (uint32_t p = a; p < b;) {
        const uint32_t maxl = b - p;
        uint32_t best = 0, dist = 0;
        if (maxl >= 3u) {
            if (p > 0) { const uint32_t l = bgzf_match_len(s.in, p - 1u, p, maxl); if (l >= 3u) { best = l; dist = 1u; } }
            if (p >= BGZF_STRIP) { const uint32_t l = bgzf_match_len(s.in, p - BGZF_STRIP, p, maxl); if (l >= 4u && l > best) { best = l; dist = BGZF_STRIP; } }
            if (maxl >= 4u) {
                const uint32_t v = bgzf_ld4(s.in, p), c = s.tab[bgzf_hash(v)];
                if (c && p - (c - 1u) <= 32768u && bgzf_ld4(s.in, c - 1u) == v) { const uint32_t l = bgzf_match_len(s.in, c - 1u, p, maxl); if (l > best) { best = l; dist = p - (c - 1u); } }
            }
        }
        const uint32_t tok = best ? bgzf_tok_match(best, dist) : (uint32_t)inb[p];
        s.tok[nt * BGZF_THREADS + lane] = tok;
        nt++; nbits += bgzf_token_nbits(tok);
        p += best ? best : 1u;
    }
    return nt;
}
// phase 1b: matches longer than a segment.  meta of a lane: the distance of its last token if that is a match (else 0), that token's length - 3 in bits
// 16..23, bit 31 when the segment is ONE match of BGZF_SEG bytes.  Such a segment continues its predecessor's last match when the distances are equal
// (the same bytes lie `distance` back for both), so it is absorbed: the predecessor's token grows by BGZF_SEG, up to 258; the segment behind a full token
// leads the next group.  Chains do not cross a strip.  Every lane decides from the strip's meta words alone, whatever the order of the lanes.
BGZF_HD uint32_t bgzf_lane_meta(const BgzfLds &s, uint32_t lane, uint32_t nt)
{
    if (!nt) return 0;
    const uint32_t last = s.tok[(nt - 1u) * BGZF_THREADS + lane];
    if (!(last & 0x80000000u)) return 0;
    const uint32_t l3 = (last >> 15) & 0xffu;
    return ((last & 0x7fffu) + 1u) | (l3 << 16) | ((nt == 1u && l3 + 3u == BGZF_SEG) ? 0x80000000u : 0u);
}
BGZF_HD bool bgzf_absorbable(const uint32_t *meta, uint32_t x) { return x > 0 && (meta[x] >> 31) && (meta[x - 1] & 0xffffu) == (meta[x] & 0xffffu); }
// the lane's token count and bits after the merge (an absorbed lane has none; a leader's last token has grown)
BGZF_HD void bgzf_lane_merge(BgzfLds &s, const uint32_t *meta, uint32_t lane, uint32_t &nt, uint32_t &nbits)
{
    const uint32_t m = meta[lane];
    if (!(m & 0xffffu)) return;
    uint32_t len = ((m >> 16) & 0xffu) + 3u;
    if (bgzf_absorbable(meta, lane)) {
        uint32_t h = lane;
        while (bgzf_absorbable(meta, h)) h--;
        const uint32_t i = lane - h, first = (258u - (((meta[h] >> 16) & 0xffu) + 3u)) / BGZF_SEG;      // segments the chain's head takes
        const uint32_t group = 1u + (258u - BGZF_SEG) / BGZF_SEG;                                          // a later leader and what it takes
        if (i <= first || (i - first - 1u) % group) { nt = 0; nbits = 0; return; }
        len = BGZF_SEG;
    }
    const uint32_t cap = (258u - len) / BGZF_SEG;
    uint32_t k = 0;
    while (k < cap && lane + 1u + k < BGZF_THREADS && bgzf_absorbable(meta, lane + 1u + k)) k++;
    if (!k) return;
    const uint32_t at = (nt - 1u) * BGZF_THREADS + lane, old = s.tok[at], grown = bgzf_tok_match(len + k * BGZF_SEG, m & 0xffffu);
    s.tok[at] = grown;
    nbits = nbits - bgzf_token_nbits(old) + bgzf_token_nbits(grown);
}
// phase 2: the lane's nt tokens as bits from bit `pos` of the slot on (head: the three bits of the block header go in front, pos counts them already):
// whole words by plain stores, the first and the last word -- which neighbours may share -- by OR into the zeroed slot
BGZF_HD void bgzf_lane_emit(const BgzfLds &s, uint32_t lane, uint32_t nt, uint32_t pos, bool head, uint32_t *slot_w)
{
    uint32_t w = pos >> 5, nacc = pos & 31u;
    uint64_t acc = 0;
    bool first = true;
    if (head) {                                             // BFINAL = 1, BTYPE = 01
        const uint32_t hp = pos - 3u;
        if ((hp >> 5) == w) acc = 3ull << (hp & 31u); else bgzf_or(&slot_w[hp >> 5], 3u << (hp & 31u));      // (pos = 147: the same word)
    }
    for (uint32_t i = 0; i < nt; i++) {
        uint32_t nb;
        const uint32_t v = bgzf_token_bits(s.tok[i * BGZF_THREADS + lane], nb);
        acc |= (uint64_t)v << nacc; nacc += nb;
        if (nacc >= 32u) {
            if (first) { bgzf_or(&slot_w[w], (uint32_t)acc); first = false; } else slot_w[w] = (uint32_t)acc;
            acc >>= 32; nacc -= 32u; w++;
        }
    }
    if (nacc) bgzf_or(&slot_w[w], (uint32_t)acc);
}
// phase 3: the segment's positions enter the table
BGZF_HD void bgzf_lane_insert(BgzfLds &s, uint32_t a, uint32_t b, uint32_t n)
{
    for (uint32_t p = a; p < b; p++) if (p + 4u <= n) bgzf_max(&s.tab[bgzf_hash(bgzf_ld4(s.in, p))], p + 1u);
}
// the strip's verdict: with `strip_bits` more bits behind `bit_base`, is the coded form (3 header bits counted in bit_base, 7 for the end of the block) still
// smaller than the n bytes of input?  Once it is not the block goes out stored, and nothing more is written.
BGZF_HD bool bgzf_still_coded(uint32_t bit_base, uint32_t strip_bits, uint32_t n) { return (bit_base + strip_bits + 7u + 7u) / 8u < n; }
BGZF_HD void bgzf_put_stored_head(unsigned char *p, uint32_t n) { p[0] = 1; p[1] = (unsigned char)n; p[2] = (unsigned char)(n >> 8); p[3] = (unsigned char)~n; p[4] = (unsigned char)(~n >> 8); }

// in: n bytes, 4-byte aligned, readable up to the next multiple of 4.  Block b's slot is slots + b * BGZF_SLOT; size[b] its bytes (u64, for the scan).
__global__ void __launch_bounds__(BGZF_THREADS)
k_bgzf_deflate(const unsigned char *__restrict__ in, unsigned long long n_total, unsigned char *__restrict__ slots, uint64_t *__restrict__ size_scan, uint32_t *__restrict__ size)
{
    __shared__ BgzfLds s;
    const uint32_t tid = threadIdx.x;
    const unsigned long long at = (unsigned long long)blockIdx.x * BGZF_BLOCK;
    const uint32_t n = (uint32_t)(n_total - at < BGZF_BLOCK ? n_total - at : BGZF_BLOCK);
    unsigned char *slot = slots + (size_t)blockIdx.x * BGZF_SLOT;
    uint32_t *slot_w = (uint32_t *)slot;
    const uint32_t *src = (const uint32_t *)(in + at);

    // the block into LDS (zeros behind its end), the slot's words the coder may touch to zero, the tables
    for (uint32_t w = tid; w < BGZF_IN_WORDS; w += BGZF_THREADS) {
        uint32_t v = 0;
        if (4u * w < n) { v = src[w]; if (4u * w + 4u > n) v &= 0xffffffffu >> (8u * (4u * w + 4u - n)); }
        s.in[w] = v;
    }
    const uint32_t zero_words = (18u + n + 8u + 3u) / 4u + 1u;                // < BGZF_SLOT / 4: 18 + 0xff00 + 8 + 7 < 65536
    for (uint32_t w = tid; w < zero_words; w += BGZF_THREADS) slot_w[w] = 0;
    for (uint32_t w = tid; w < (1u << BGZF_HASH_BITS); w += BGZF_THREADS) s.tab[w] = 0;
    s.crc_tab[tid] = bgzf_crc_entry(tid);
    __syncthreads();
    const unsigned char *inb = (const unsigned char *)s.in;

    // CRC32: every lane its piece, combined pairwise
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

    // the deflate stream: 3 bits of block header, the tokens, 7 bits of end-of-block code (zeros)
    uint32_t bit_base = 3;                                  // bits of the stream before the current strip
    bool coded = true;
    for (uint32_t s0 = 0; s0 < n && coded; s0 += BGZF_STRIP) {
        const uint32_t a = s0 + tid * BGZF_SEG;
        const uint32_t b = a + BGZF_SEG < n ? a + BGZF_SEG : n;
        uint32_t nbits = 0;
        uint32_t nt = bgzf_lane_tokens(s, tid, a, b, nbits);
        s.len[tid] = bgzf_lane_meta(s, tid, nt);
        __syncthreads();
        bgzf_lane_merge(s, s.len, tid, nt, nbits);
        // where the lane's bits start
        s.scan[tid] = nbits;
        __syncthreads();
        for (uint32_t o = 1; o < BGZF_THREADS; o <<= 1) {
            const uint32_t t = tid >= o ? s.scan[tid - o] : 0u;
            __syncthreads();
            s.scan[tid] += t;
            __syncthreads();
        }
        const uint32_t strip_bits = s.scan[BGZF_THREADS - 1];
        // the coded form can only pay while it is smaller than the input: beyond that nothing more is written (and nothing is written past the slot)
        coded = bgzf_still_coded(bit_base, strip_bits, n);
        if (coded && nt) bgzf_lane_emit(s, tid, nt, 18u * 8u + bit_base + s.scan[tid] - nbits, s0 == 0 && tid == 0, slot_w);
        bit_base += strip_bits;
        bgzf_lane_insert(s, a, b, n);
        __syncthreads();
    }
    const uint32_t clen = coded ? (bit_base + 7u + 7u) / 8u : n + 5u;
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
}

// off: the exclusive scan of the sizes
__global__ void __launch_bounds__(256)
k_bgzf_copy(const unsigned char *__restrict__ slots, const uint64_t *__restrict__ off, const uint32_t *__restrict__ size, unsigned char *__restrict__ out)
{
    const unsigned char *src = slots + (size_t)blockIdx.x * BGZF_SLOT;
    unsigned char *dst = out + off[blockIdx.x];
    const uint32_t n = size[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
}
#endif
