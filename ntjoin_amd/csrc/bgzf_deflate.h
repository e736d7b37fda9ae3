// BGZF written: ONE member of at most 65 280 bytes of text put together -- gzip header with the 'B' 'C' subfield, deflate data,
// CRC-32 and ISIZE -- by a coder that uses literals and the end-of-block code only (no match search: on DNA text a Huffman code over
// the literals is what gzip's own output comes to).  Plain C++ over plain arrays, written the way bgzf_inflate.h is:
// the kernel (bgzf_deflate.hip, one member per work-group, the tables in LDS) and a CPU program (tests/test_bgzf_deflate_cpu.py,
// also under the sanitizers) compile the same text, and both produce the same bytes for the same payload: every decision -- the
// code lengths, the blocks' headers, dynamic or stored -- is made by bgzf_build and bgzf_plan_member below from the member's
// histograms alone, before a byte is written.
//
// The deflate data of a member:
//   - dynamic Huffman blocks (BTYPE 10), one for the text's first BGZF_SPLIT = 32 640 bytes and one for the rest (zlib starts a
//     new block every 32 767 literals too: text that changes its alphabet inside a member, upper case to lower case, gets a code
//     for either part).  Per block: lengths from the histogram of the 256 literals + the end-of-block code (count 1), limited to
//     15 bits, canonical codes, the lengths sent through the code-length alphabet with 16 / 17 / 18 for runs; HLIT = 257,
//     HDIST = 1 with the one distance code left without a length (a block of literals only: zlib's inflate and
//     bgzf_inflate_member take it);
//   - ONE stored block (BTYPE 00) whenever the dynamic blocks together would not be smaller than the text + 5 bytes, so a member
//     is never larger than its text + BGZF_SLACK;
//   - no text at all: the 28-byte end-of-file marker bgzip writes (a fixed-Huffman block that holds the end-of-block code alone).
#pragma once
#include <cstddef>
#include <cstdint>

#include "bgzf_inflate.h"  // MXG_BGZF_FN, bgzf_crc32_entry

namespace mxg {

constexpr uint32_t BGZF_MAX_PAYLOAD = 65280;  // bgzip's own value
constexpr uint32_t BGZF_HEAD = 18, BGZF_TRAIL = 8;
constexpr uint32_t BGZF_SLACK = BGZF_HEAD + 5 + BGZF_TRAIL;  // a stored member: header, 01 LEN NLEN, trailer
constexpr uint32_t BGZF_EOF_BYTES = 28;
constexpr uint32_t BGZF_NSYM = 257;  // literals + end-of-block
constexpr uint32_t BGZF_MAX_BLOCKS = 2;
constexpr uint32_t BGZF_SPLIT = 32640;  // text bytes of a member's first block (128 threads' shares of 255 bytes in the kernel)
static_assert(BGZF_MAX_PAYLOAD + BGZF_SLACK <= 65536, "BSIZE has 16 bits");

// what a member's coder works with: the kernel keeps one in LDS, the host one on its stack
struct BgzfEnc {
    uint32_t freq[BGZF_NSYM];  // in: the literals' counts ([256] is set by bgzf_build)
    uint32_t code[BGZF_NSYM];  // out: the symbol's code, bits reversed (deflate packs codes from their top bit), | length << 16
    uint32_t work[BGZF_NSYM];  // the tree in place (Moffat and Katajainen)
    uint16_t order[BGZF_NSYM];
    uint8_t len[BGZF_NSYM + 3];  // code lengths: 257 literal/length symbols and the one distance symbol
    uint32_t cl_freq[19], cl_code[19];
    uint8_t cl_len[20];
    uint32_t cnt[16], next[16];
    uint32_t hclen;      // code-length code lengths sent (4 .. 19)
    uint32_t hdr_bits;   // the block's bits in front of the first literal, BFINAL and BTYPE among them
    uint32_t data_bits;  // the literals' bits and the end-of-block code's
    uint32_t ok;         // 1: both sets of lengths fill their code space (else the member is stored)
};

// what bgzf_plan_member decides for a member from its blocks' coders
struct BgzfMemberPlan {
    uint32_t stored;         // 1: one stored block
    uint32_t n_blocks;       // dynamic blocks (1 or 2)
    uint32_t deflate_bytes;  // the member's bytes between header and trailer
    uint32_t bit0[BGZF_MAX_BLOCKS];  // where block b's header starts, in bits from the first deflate byte
};

// the order the code-length code's lengths are sent in: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
MXG_BGZF_FN uint32_t bgzf_cl_order(uint32_t i)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                        5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12u ? lo >> (5u * i) : hi >> (5u * (i - 12u))) & 31u);
}

// Code lengths of the n symbols counted in f (n <= 257, sum of f < 2^31), none above maxbits (2^maxbits >= n); len[s] = 0 for a
// symbol never seen.  Returns true when the lengths fill the code space exactly (what inflate asks of a literal/length set).
// The symbols in use are sorted by (count, symbol) by insertion -- DNA text has a handful --, the tree is built in place over the
// sorted counts, and depths beyond maxbits are brought back by the Kraft sum: the rarest symbols that can still grow get one bit
// more until the sum fits, then the most frequent ones that can take the room get one bit less until it is used up.
MXG_BGZF_FN bool bgzf_huff_lengths(const uint32_t *f, uint32_t n, uint32_t maxbits, uint32_t *A, uint16_t *ord, uint8_t *len)
{
    uint32_t m = 0;
    for (uint32_t s = 0; s < n; ++s) {
        len[s] = 0;
        if (!f[s]) continue;
        uint32_t j = m;
        for (; j > 0 && f[ord[j - 1]] > f[s]; --j) ord[j] = ord[j - 1];
        ord[j] = (uint16_t)s;
        ++m;
    }
    if (m == 0) return false;
    if (m == 1) {
        len[ord[0]] = 1;
        return false;
    }
    for (uint32_t i = 0; i < m; ++i) A[i] = f[ord[i]];
    // phase 1: parents (A[0 .. m - 2) become internal nodes' weights, then parent indices)
    A[0] += A[1];
    uint32_t root = 0, leaf = 2;
    for (uint32_t next = 1; next + 1 < m; ++next) {
        if (leaf >= m || A[root] < A[leaf]) {
            A[next] = A[root];
            A[root++] = next;
        } else {
            A[next] = A[leaf++];
        }
        if (leaf >= m || (root < next && A[root] < A[leaf])) {
            A[next] += A[root];
            A[root++] = next;
        } else {
            A[next] += A[leaf++];
        }
    }
    // phase 2: internal depths
    A[m - 2] = 0;
    for (uint32_t next = m - 2; next-- > 0;) A[next] = A[A[next]] + 1u;
    // phase 3: leaf depths, deepest (rarest) first
    {
        uint32_t avbl = 1, used = 0, dpth = 0;
        int32_t r = (int32_t)m - 2, nx = (int32_t)m - 1;
        while (avbl > 0) {
            while (r >= 0 && A[r] == dpth) {
                ++used;
                --r;
            }
            while (avbl > used) {
                A[nx--] = dpth;
                --avbl;
            }
            avbl = 2u * used;
            ++dpth;
            used = 0;
        }
    }
    // the limit: K = sum of 2^(maxbits - length), full = 2^maxbits
    const uint32_t full = 1u << maxbits;
    uint32_t K = 0;
    for (uint32_t i = 0; i < m; ++i) {
        if (A[i] > maxbits) A[i] = maxbits;
        K += 1u << (maxbits - A[i]);
    }
    while (K > full) {  // (m <= full: some length is below maxbits while K > full; lengths fall with i, so the first such is the longest)
        uint32_t i = 0;
        while (i < m && A[i] >= maxbits) ++i;
        if (i == m) break;
        K -= 1u << (maxbits - A[i] - 1u);
        ++A[i];
    }
    while (K < full) {
        const uint32_t room = full - K;
        uint32_t i = m;
        while (i > 0 && !(A[i - 1] > 1u && (1u << (maxbits - A[i - 1])) <= room)) --i;
        if (i == 0) break;
        K += 1u << (maxbits - A[i - 1]);
        --A[i - 1];
    }
    for (uint32_t i = 0; i < m; ++i) len[ord[i]] = (uint8_t)A[i];
    return K == full;
}

MXG_BGZF_FN uint32_t bgzf_bitrev(uint32_t v, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i, v >>= 1) r = r << 1 | (v & 1u);
    return r;
}

// canonical codes of the lengths (1 .. 15), reversed, | length << 16; 0 for a symbol without a code
MXG_BGZF_FN void bgzf_canonical(const uint8_t *len, uint32_t n, uint32_t *code, uint32_t *cnt, uint32_t *next)
{
    for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
    for (uint32_t s = 0; s < n; ++s) ++cnt[len[s] & 15u];
    cnt[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        c = (c + cnt[l - 1]) << 1;
        next[l] = c;
    }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = len[s] & 15u;
        code[s] = l ? bgzf_bitrev(next[l]++, l) | l << 16 : 0u;
    }
}

// the n code lengths as symbols of the code-length alphabet: f(symbol, extra bits, their value)
template <class F> MXG_BGZF_FN void bgzf_rle(const uint8_t *len, uint32_t n, F &f)
{
    uint32_t i = 0;
    while (i < n) {
        const uint32_t v = len[i];
        uint32_t run = 1;
        while (i + run < n && len[i + run] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11u) {
                const uint32_t t = run < 138u ? run : 138u;
                f(18u, 7u, t - 11u);
                run -= t;
            }
            if (run >= 3u) {
                f(17u, 3u, run - 3u);
                run = 0;
            }
            for (; run; --run) f(0u, 0u, 0u);
        } else {
            f(v, 0u, 0u);
            --run;
            while (run >= 3u) {
                const uint32_t t = run < 6u ? run : 6u;
                f(16u, 2u, t - 3u);
                run -= t;
            }
            for (; run; --run) f(v, 0u, 0u);
        }
    }
}

struct BgzfRleCount {
    uint32_t *freq;
    uint32_t extra = 0;
    MXG_BGZF_FN void operator()(uint32_t s, uint32_t eb, uint32_t) { ++freq[s], extra += eb; }
};

// bits into an image of 32-bit words that starts out zero; nothing is written at or beyond word `cap`
struct BgzfBitW {
    uint32_t *w;
    uint32_t cap, pos;
    MXG_BGZF_FN void put(uint32_t v, uint32_t n)  // n <= 16, v < 2^n
    {
        const uint32_t i = pos >> 5, sh = pos & 31u;
        if (i < cap) w[i] |= v << sh;
        if (sh + n > 32u && i + 1u < cap) w[i + 1u] |= v >> (32u - sh);
        pos += n;
    }
};

struct BgzfRleEmit {
    BgzfBitW &out;
    const uint32_t *cl_code;
    MXG_BGZF_FN void operator()(uint32_t s, uint32_t eb, uint32_t ev)
    {
        out.put(cl_code[s] & 0xFFFFu, cl_code[s] >> 16);
        if (eb) out.put(ev, eb);
    }
};

// e.freq[0 .. 256) counted over a block's text -> everything else of e
MXG_BGZF_FN void bgzf_build(BgzfEnc &e)
{
    e.freq[256] = 1;
    bool ok = bgzf_huff_lengths(e.freq, BGZF_NSYM, 15u, e.work, e.order, e.len);
    e.len[BGZF_NSYM] = 0;  // the distance symbol
    bgzf_canonical(e.len, BGZF_NSYM, e.code, e.cnt, e.next);
    uint32_t bits = 0;
    for (uint32_t s = 0; s < BGZF_NSYM; ++s) bits += e.freq[s] * e.len[s];
    e.data_bits = bits;
    for (uint32_t s = 0; s < 19; ++s) e.cl_freq[s] = 0;
    BgzfRleCount count{e.cl_freq};
    bgzf_rle(e.len, BGZF_NSYM + 1u, count);
    ok = bgzf_huff_lengths(e.cl_freq, 19u, 7u, e.work, e.order, e.cl_len) && ok;
    bgzf_canonical(e.cl_len, 19u, e.cl_code, e.cnt, e.next);
    uint32_t hclen = 19;
    while (hclen > 4u && e.cl_len[bgzf_cl_order(hclen - 1u)] == 0) --hclen;
    e.hclen = hclen;
    uint32_t hb = 3u + 14u + 3u * hclen + count.extra;
    for (uint32_t s = 0; s < 19; ++s) hb += e.cl_freq[s] * e.cl_len[s];
    e.hdr_bits = hb;
    e.ok = ok ? 1u : 0u;
}

// a member of n >= 1 bytes of text whose blocks' coders e[0 .. n_blocks) are built: n_blocks = 1 for n <= BGZF_SPLIT, else 2
MXG_BGZF_FN void bgzf_plan_member(const BgzfEnc *e, uint32_t n, BgzfMemberPlan &p)
{
    p.n_blocks = n > BGZF_SPLIT ? 2u : 1u;
    uint32_t bits = 0, ok = 1;
    for (uint32_t b = 0; b < BGZF_MAX_BLOCKS; ++b) {
        p.bit0[b] = bits;
        if (b < p.n_blocks) {
            bits += e[b].hdr_bits + e[b].data_bits;
            ok &= e[b].ok;
        }
    }
    const uint32_t dyn = (bits + 7u) >> 3;
    p.stored = !ok || dyn >= n + 5u ? 1u : 0u;
    p.deflate_bytes = p.stored ? n + 5u : dyn;
}

// the dynamic block's bits in front of the first literal, at out.pos
MXG_BGZF_FN void bgzf_put_block_header(const BgzfEnc &e, BgzfBitW &out, uint32_t final)
{
    out.put(final, 1u);  // BFINAL
    out.put(2u, 2u);  // BTYPE 10
    out.put(0u, 5u);  // HLIT: 257 codes
    out.put(0u, 5u);  // HDIST: 1 code
    out.put(e.hclen - 4u, 4u);
    for (uint32_t i = 0; i < e.hclen; ++i) out.put(e.cl_len[bgzf_cl_order(i)], 3u);
    BgzfRleEmit emit{out, e.cl_code};
    bgzf_rle(e.len, BGZF_NSYM + 1u, emit);
}

// the member's first 18 bytes as words 0 .. 3 and the low half of word 4 (little endian): 1f 8b 08 04 | mtime 0 | xfl 0, os ff,
// xlen 6 | 'B' 'C' 2 0 | BSIZE = member size - 1
MXG_BGZF_FN void bgzf_put_member_header(uint32_t *w, uint32_t member_bytes)
{
    w[0] = 0x04088b1fu;
    w[1] = 0u;
    w[2] = 0x0006ff00u;
    w[3] = 0x00024342u;
    w[4] |= (member_bytes - 1u) & 0xFFFFu;
}

// ---- CRC-32 of a text from the CRCs of its pieces -------------------------------------------------------------------------------
// a(x) b(x) mod P in the reflected representation (bit 31 = x^0), as zlib's multmodp
MXG_BGZF_FN uint32_t bgzf_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
MXG_BGZF_FN uint32_t bgzf_crc_shift(uint32_t crc, uint32_t bytes)  // the register after `bytes` more bytes of zeros: crc x^(8 bytes)
{
    uint32_t sq = 0x00800000u;  // x^8
    for (; bytes; bytes >>= 1) {
        if (bytes & 1u) crc = bgzf_crc_mul(sq, crc);
        sq = bgzf_crc_mul(sq, sq);
    }
    return crc;
}

// ---- the host's coder: what the kernel's output is compared with -----------------------------------------------------------------
// One member of n <= BGZF_MAX_PAYLOAD bytes into out (room for n + BGZF_SLACK, at least BGZF_EOF_BYTES); returns its size.
// *was_stored (if given): the block is a stored one.
inline uint32_t bgzf_deflate_member_host(const unsigned char *p, uint32_t n, unsigned char *out, bool *was_stored = nullptr)
{
    auto put32 = [](unsigned char *q, uint32_t v) {
        for (int b = 0; b < 4; ++b) q[b] = (unsigned char)(v >> (8 * b));
    };
    uint32_t head[5] = {0, 0, 0, 0, 0};
    if (was_stored) *was_stored = false;
    if (n == 0) {
        bgzf_put_member_header(head, BGZF_EOF_BYTES);
        for (uint32_t i = 0; i < 4; ++i) put32(out + 4 * i, head[i]);
        out[16] = (unsigned char)head[4], out[17] = (unsigned char)(head[4] >> 8);
        out[18] = 3, out[19] = 0;
        for (uint32_t i = 20; i < BGZF_EOF_BYTES; ++i) out[i] = 0;
        return BGZF_EOF_BYTES;
    }
    BgzfEnc e[BGZF_MAX_BLOCKS];
    for (uint32_t b = 0; b < BGZF_MAX_BLOCKS; ++b)
        for (uint32_t s = 0; s < BGZF_NSYM; ++s) e[b].freq[s] = 0;
    uint32_t crc = 0xFFFFFFFFu;
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) tab[i] = bgzf_crc32_entry(i);
    for (uint32_t i = 0; i < n; ++i) {
        ++e[i >= BGZF_SPLIT].freq[p[i]];
        crc = tab[(crc ^ p[i]) & 255u] ^ (crc >> 8);
    }
    crc ^= 0xFFFFFFFFu;
    BgzfMemberPlan plan;
    bgzf_build(e[0]);
    if (n > BGZF_SPLIT) bgzf_build(e[1]);
    bgzf_plan_member(e, n, plan);
    const uint32_t size = BGZF_HEAD + plan.deflate_bytes + BGZF_TRAIL;
    bgzf_put_member_header(head, size);
    for (uint32_t i = 0; i < 4; ++i) put32(out + 4 * i, head[i]);
    out[16] = (unsigned char)head[4], out[17] = (unsigned char)(head[4] >> 8);
    unsigned char *d = out + BGZF_HEAD;
    if (plan.stored) {
        if (was_stored) *was_stored = true;
        d[0] = 1;
        d[1] = (unsigned char)n, d[2] = (unsigned char)(n >> 8);
        d[3] = (unsigned char)~n, d[4] = (unsigned char)(~n >> 8);
        for (uint32_t i = 0; i < n; ++i) d[5 + i] = p[i];
    } else {
        // serially, bit by bit at the places the plan names: the kernel's threads write the same bits side by side
        for (uint32_t i = 0; i < plan.deflate_bytes; ++i) d[i] = 0;
        uint32_t pos = 0;
        auto put = [&](uint32_t v, uint32_t nb) {
            for (uint32_t k = 0; k < nb; ++k, ++pos)
                if ((v >> k & 1u) && (pos >> 3) < plan.deflate_bytes) d[pos >> 3] |= (unsigned char)(1u << (pos & 7u));
        };
        for (uint32_t b = 0; b < plan.n_blocks; ++b) {
            uint32_t hw[80];
            for (uint32_t i = 0; i < 80; ++i) hw[i] = 0;
            BgzfBitW w{hw, 80u, 0u};
            bgzf_put_block_header(e[b], w, b + 1u == plan.n_blocks ? 1u : 0u);
            pos = plan.bit0[b];
            for (uint32_t k = 0; k < w.pos; ++k) put(hw[k >> 5] >> (k & 31u) & 1u, 1u);
            const uint32_t lo = b ? BGZF_SPLIT : 0u, hi = b + 1u < plan.n_blocks ? BGZF_SPLIT : n;
            for (uint32_t i = lo; i < hi; ++i) put(e[b].code[p[i]] & 0xFFFFu, e[b].code[p[i]] >> 16);
            put(e[b].code[256] & 0xFFFFu, e[b].code[256] >> 16);
        }
    }
    put32(d + plan.deflate_bytes, crc);
    put32(d + plan.deflate_bytes + 4, n);
    return size;
}

}  // namespace mxg
