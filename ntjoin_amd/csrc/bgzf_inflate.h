// BGZF (what `bgzip` writes: a chain of independent gzip members of at most 64 KiB of text each) taken apart: the walk over a file's
// members and a raw DEFLATE decoder for ONE member.  Plain C++ over an abstract byte source, byte sink and table storage: the kernel
// (bgzf.hip, one member per lane, tables in LDS) and the CPU tests (tests/test_bgzf_cpu.py, tests/test_bgzf_craft_cpu.py, also
// under the sanitizers) compile the same text; the kernel's source, sink and table types are in bgzf_dev_io.h for the same reason.
//
// The decoder is safe on any input by construction, not by trust in the file:
//   - every input byte is fetched through BgzfBits::need, which stops at the member's deflate length;
//   - every output byte is counted against the member's ISIZE before it is put;
//   - a match distance never reaches in front of what THIS member has produced (no dictionary from another member);
//   - code-length sets are accepted by zlib's rules: an over-subscribed set is refused, an incomplete one too, except a literal/length
//     or distance set of exactly one code of one bit -- the other bit is then no code of the set -- and the distance set without any
//     code (a block of literals only); the code-length code itself must be complete, and the end-of-block code must have a length;
//   - the symbol tables are indexed only below the number of symbols that were counted into them;
//   - the decode must end on the end-of-block code of a final block, with exactly ISIZE bytes put and every input byte used.
// Every loop consumes input bits, produces output bytes or runs over a constant: `steps` counts the decoded symbols and block
// headers, each of which uses at least one bit, so steps <= 8 * (deflate length) + 1 whatever the bytes are.
#pragma once
#include <cstddef>
#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MXG_BGZF_FN __host__ __device__ __forceinline__
#else
#define MXG_BGZF_FN inline
#endif
#include <vector>

namespace mxg {

struct BgzfMember {    // one non-empty member
    uint64_t in_off;   // its raw deflate data in the file
    uint64_t out_off;  // its text in the inflated file (exclusive prefix sum of ISIZE)
    uint32_t in_len;
    uint32_t isize;    // bytes of text, 1 .. 65536
    uint32_t crc;      // CRC-32 of the text
    uint32_t head;     // bytes of the member's header in front of in_off
};

enum BgzfStatus : uint32_t {
    BGZF_OK = 0,
    BGZF_IN_END = 1,        // the deflate data ends inside a block
    BGZF_OUT_FULL = 2,      // more text than ISIZE
    BGZF_BLOCK_TYPE = 3,    // block type 11
    BGZF_STORED_LEN = 4,    // LEN and NLEN of a stored block do not agree
    BGZF_CODE_LENGTHS = 5,  // a set of code lengths zlib refuses
    BGZF_SYMBOL = 6,        // bits that are no code of the set, or a code without a meaning (286, 287; distance 30, 31)
    BGZF_DISTANCE = 7,      // a match that starts in front of the member's text
    BGZF_SIZE = 8,          // the final block ends with less text than ISIZE
    BGZF_TRAILING = 9,      // deflate data left behind the final block
    BGZF_CRC = 10,          // the text is not what the trailer's CRC-32 says
    BGZF_PLAN = 11,         // a member descriptor that leaves its buffers (the kernel's own check of the table)
};

// table storage of one decoder: BGZF_TAB_ELEMS values of 16 bits behind get(e) / set(e, v)
constexpr uint32_t BGZF_E_CNT_L = 0;     // [16]  codes of every length, literal/length set (and the code-length set before it)
constexpr uint32_t BGZF_E_SYM_L = 16;    // [288] its symbols in canonical order
constexpr uint32_t BGZF_E_CNT_D = 304;   // [16]  distance set
constexpr uint32_t BGZF_E_SYM_D = 320;   // [32]
constexpr uint32_t BGZF_E_OFFS = 352;    // [16]  where the symbols of every length start (while a set is built)
constexpr uint32_t BGZF_E_LEN = 368;     // [80]  320 code lengths of a dynamic block, four bits each
constexpr uint32_t BGZF_TAB_ELEMS = 448;
constexpr uint32_t BGZF_MAX_ISIZE = 65536;

MXG_BGZF_FN uint32_t bgzf_crc32_entry(uint32_t i)  // the CRC-32 table (reflected polynomial edb88320), entry i
{
    uint32_t c = i;
    for (int b = 0; b < 8; ++b) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}

// Src: uint32_t len() const, uint32_t byte(uint32_t i) for i < len()
template <class Src> struct BgzfBits {
    Src &src;
    uint32_t pos = 0, buf = 0, cnt = 0;  // next byte, bits fetched and not used yet (cnt < 32)
    MXG_BGZF_FN explicit BgzfBits(Src &s) : src(s) {}
    MXG_BGZF_FN bool need(uint32_t n)  // n <= 16: at most two bytes are fetched
    {
        while (cnt < n) {
            if (pos >= src.len()) return false;
            buf |= src.byte(pos++) << cnt;
            cnt += 8;
        }
        return true;
    }
    MXG_BGZF_FN uint32_t take(uint32_t n)  // after need(n)
    {
        const uint32_t v = buf & ((1u << n) - 1u);
        buf >>= n;
        cnt -= n;
        return v;
    }
};

template <class Tab> MXG_BGZF_FN uint32_t bgzf_len_get(const Tab &tab, uint32_t s)
{
    return (tab.get(BGZF_E_LEN + (s >> 2)) >> (4u * (s & 3u))) & 15u;
}
template <class Tab> MXG_BGZF_FN void bgzf_len_set(Tab &tab, uint32_t s, uint32_t v)
{
    const uint32_t e = BGZF_E_LEN + (s >> 2), sh = 4u * (s & 3u);
    tab.set(e, (tab.get(e) & ~(15u << sh)) | (v << sh));
}

// canonical code of the n lengths at len0: counts at `cnt`, symbols at `sym`.  Returns what is left of the code space: 0 complete,
// > 0 incomplete, < 0 over-subscribed (the tables are then not to be used).  No length at all counts as complete: nothing decodes.
template <class Tab> MXG_BGZF_FN int bgzf_construct(Tab &tab, uint32_t cnt, uint32_t sym, uint32_t len0, uint32_t n)
{
    for (uint32_t l = 0; l < 16; ++l) tab.set(cnt + l, 0);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = bgzf_len_get(tab, len0 + s);
        tab.set(cnt + l, tab.get(cnt + l) + 1u);
    }
    if (tab.get(cnt) == n) return 0;
    int left = 1;
    for (uint32_t l = 1; l < 16; ++l) {
        left <<= 1;
        left -= (int)tab.get(cnt + l);
        if (left < 0) return left;
    }
    tab.set(BGZF_E_OFFS + 1, 0);
    for (uint32_t l = 1; l < 15; ++l) tab.set(BGZF_E_OFFS + l + 1, tab.get(BGZF_E_OFFS + l) + tab.get(cnt + l));
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = bgzf_len_get(tab, len0 + s);
        if (l) {
            const uint32_t o = tab.get(BGZF_E_OFFS + l);  // < (codes of lengths 1 .. 15) <= n
            tab.set(sym + o, s);
            tab.set(BGZF_E_OFFS + l, o + 1u);
        }
    }
    return left;
}

// one symbol, bit by bit (at most 15); -1 with *err set when the input ends or the bits are no code of the set
template <class Src, class Tab> MXG_BGZF_FN int bgzf_decode(BgzfBits<Src> &in, const Tab &tab, uint32_t cnt, uint32_t sym, uint32_t *err)
{
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        if (!in.need(1)) {
            *err = BGZF_IN_END;
            return -1;
        }
        code |= in.take(1);
        const uint32_t count = tab.get(cnt + l);
        if (code < first + count) return (int)tab.get(sym + index + (code - first));  // index + (code - first) < index + count
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    *err = BGZF_SYMBOL;
    return -1;
}

// the blocks' symbols up to the end-of-block code; `out` = bytes put so far
template <class Src, class Sink, class Tab>
MXG_BGZF_FN uint32_t bgzf_codes(BgzfBits<Src> &in, Sink &sink, const Tab &tab, uint32_t isize, uint32_t &out, uint32_t &steps)
{
    for (;;) {
        ++steps;
        uint32_t err = BGZF_OK;
        const int s = bgzf_decode(in, tab, BGZF_E_CNT_L, BGZF_E_SYM_L, &err);
        if (s < 0) return err;
        if (s < 256) {
            if (out >= isize) return BGZF_OUT_FULL;
            sink.put((uint8_t)s);
            ++out;
            continue;
        }
        if (s == 256) return BGZF_OK;
        if (s >= 286) return BGZF_SYMBOL;
        // length 3 .. 258 from symbol 257 .. 285
        const uint32_t ls = (uint32_t)s - 257u;
        uint32_t len, eb;
        if (ls < 8u) {
            len = 3u + ls;
            eb = 0;
        } else if (ls == 28u) {
            len = 258u;
            eb = 0;
        } else {
            eb = (ls >> 2) - 1u;
            len = 3u + ((4u + (ls & 3u)) << eb);
        }
        if (!in.need(eb)) return BGZF_IN_END;
        len += in.take(eb);
        ++steps;
        const int d = bgzf_decode(in, tab, BGZF_E_CNT_D, BGZF_E_SYM_D, &err);
        if (d < 0) return err;
        if (d >= 30) return BGZF_SYMBOL;
        uint32_t dist;
        if (d < 4) {
            dist = 1u + (uint32_t)d;
            eb = 0;
        } else {
            eb = ((uint32_t)d >> 1) - 1u;  // <= 13
            dist = 1u + ((2u + ((uint32_t)d & 1u)) << eb);
        }
        if (!in.need(eb)) return BGZF_IN_END;
        dist += in.take(eb);
        if (dist > out) return BGZF_DISTANCE;
        if (len > isize - out) return BGZF_OUT_FULL;
        for (uint32_t i = 0; i < len; ++i) sink.put(sink.back(dist));  // (byte by byte: a distance below the length repeats)
        out += len;
    }
}

template <class Tab> MXG_BGZF_FN void bgzf_fixed_tables(Tab &tab)
{
    for (uint32_t l = 0; l < 16; ++l) {
        tab.set(BGZF_E_CNT_L + l, l == 7 ? 24u : l == 8 ? 152u : l == 9 ? 112u : 0u);
        tab.set(BGZF_E_CNT_D + l, l == 5 ? 30u : 0u);
    }
    uint32_t o = BGZF_E_SYM_L;
    for (uint32_t s = 256; s < 280; ++s) tab.set(o++, s);  // 7 bits
    for (uint32_t s = 0; s < 144; ++s) tab.set(o++, s);    // 8 bits
    for (uint32_t s = 280; s < 288; ++s) tab.set(o++, s);
    for (uint32_t s = 144; s < 256; ++s) tab.set(o++, s);  // 9 bits
    for (uint32_t s = 0; s < 30; ++s) tab.set(BGZF_E_SYM_D + s, s);
}

// the header of a dynamic block -> both sets
template <class Src, class Tab> MXG_BGZF_FN uint32_t bgzf_dynamic_tables(BgzfBits<Src> &in, Tab &tab, uint32_t &steps)
{
    if (!in.need(14)) return BGZF_IN_END;
    const uint32_t nlen = in.take(5) + 257u, ndist = in.take(5) + 1u, ncode = in.take(4) + 4u;
    if (nlen > 286u || ndist > 30u) return BGZF_CODE_LENGTHS;
    // the order the code-length code's lengths come in: 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15, five bits each
    const uint64_t ord_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                            5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t ord_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    for (uint32_t e = 0; e < 5; ++e) tab.set(BGZF_E_LEN + e, 0);  // lengths 0 .. 19
    for (uint32_t i = 0; i < ncode; ++i) {
        if (!in.need(3)) return BGZF_IN_END;
        const uint32_t s = (uint32_t)((i < 12u ? ord_lo >> (5u * i) : ord_hi >> (5u * (i - 12u))) & 31u);
        bgzf_len_set(tab, s, in.take(3));
    }
    if (bgzf_construct(tab, BGZF_E_CNT_L, BGZF_E_SYM_L, 0, 19) != 0) return BGZF_CODE_LENGTHS;  // (complete, as zlib asks)
    const uint32_t total = nlen + ndist;  // <= 316
    uint32_t index = 0;
    while (index < total) {
        ++steps;
        uint32_t err = BGZF_OK;
        const int s = bgzf_decode(in, tab, BGZF_E_CNT_L, BGZF_E_SYM_L, &err);
        if (s < 0) return err;
        if (s < 16) {
            bgzf_len_set(tab, index++, (uint32_t)s);
            continue;
        }
        uint32_t len = 0, rep;
        if (s == 16) {
            if (index == 0) return BGZF_CODE_LENGTHS;
            len = bgzf_len_get(tab, index - 1u);
            if (!in.need(2)) return BGZF_IN_END;
            rep = 3u + in.take(2);
        } else if (s == 17) {
            if (!in.need(3)) return BGZF_IN_END;
            rep = 3u + in.take(3);
        } else {
            if (!in.need(7)) return BGZF_IN_END;
            rep = 11u + in.take(7);
        }
        if (rep > total - index) return BGZF_CODE_LENGTHS;
        for (; rep; --rep) bgzf_len_set(tab, index++, len);
    }
    if (bgzf_len_get(tab, 256) == 0) return BGZF_CODE_LENGTHS;  // no end-of-block code
    // (an incomplete set of ONE code of one bit is zlib's exception for both sets: the other bit is no code, BGZF_SYMBOL)
    int left = bgzf_construct(tab, BGZF_E_CNT_L, BGZF_E_SYM_L, 0, nlen);
    if (left < 0) return BGZF_CODE_LENGTHS;
    if (left > 0 && !(tab.get(BGZF_E_CNT_L + 1) == 1u && tab.get(BGZF_E_CNT_L) + 1u == nlen)) return BGZF_CODE_LENGTHS;
    left = bgzf_construct(tab, BGZF_E_CNT_D, BGZF_E_SYM_D, nlen, ndist);
    if (left < 0) return BGZF_CODE_LENGTHS;
    if (left > 0 && !(tab.get(BGZF_E_CNT_D + 1) == 1u && tab.get(BGZF_E_CNT_D) + 1u == ndist)) return BGZF_CODE_LENGTHS;
    return BGZF_OK;
}

// One member: src = its raw deflate data, sink takes exactly `isize` bytes (put(byte) appends, back(d) is the byte d behind the
// end, 1 <= d <= bytes put).  Returns a BgzfStatus; *steps_out (if given) the symbols and block headers it decoded.
template <class Src, class Sink, class Tab>
MXG_BGZF_FN uint32_t bgzf_inflate_member(Src &src, Sink &sink, Tab &tab, uint32_t isize, uint32_t *steps_out = nullptr)
{
    BgzfBits<Src> in(src);
    uint32_t out = 0, steps = 0, st = BGZF_OK;
    for (;;) {
        ++steps;
        if (!in.need(3)) {
            st = BGZF_IN_END;
            break;
        }
        const uint32_t last = in.take(1), type = in.take(2);
        if (type == 0) {
            in.take(in.cnt & 7u);  // to the byte border
            if (!in.need(16)) {
                st = BGZF_IN_END;
                break;
            }
            const uint32_t len = in.take(16);
            if (!in.need(16)) {
                st = BGZF_IN_END;
                break;
            }
            const uint32_t nlen = in.take(16);  // (no fetched bit is left: the bytes follow at in.pos)
            if ((len ^ 0xFFFFu) != nlen) st = BGZF_STORED_LEN;
            else if (len > src.len() - in.pos) st = BGZF_IN_END;
            else if (len > isize - out) st = BGZF_OUT_FULL;
            if (st != BGZF_OK) break;
            for (uint32_t i = 0; i < len; ++i) sink.put((uint8_t)src.byte(in.pos++));
            out += len;
        } else if (type == 3) {
            st = BGZF_BLOCK_TYPE;
            break;
        } else {
            if (type == 1) bgzf_fixed_tables(tab);
            else if ((st = bgzf_dynamic_tables(in, tab, steps)) != BGZF_OK) break;
            if ((st = bgzf_codes(in, sink, tab, isize, out, steps)) != BGZF_OK) break;
        }
        if (last) break;
    }
    if (steps_out) *steps_out = steps;
    if (st != BGZF_OK) return st;
    if (out != isize) return BGZF_SIZE;
    if ((in.cnt >> 3) + (src.len() - in.pos) != 0) return BGZF_TRAILING;
    return BGZF_OK;
}

// ---- the walk over a file's members (host) ------------------------------------------------------------------------------------
struct BgzfHostSrc {
    const unsigned char *p;
    uint32_t n;
    uint32_t len() const { return n; }
    uint32_t byte(uint32_t i) const { return p[i]; }
};
struct BgzfHostTab {
    uint16_t e[BGZF_TAB_ELEMS] = {};
    uint32_t get(uint32_t i) const { return e[i]; }
    void set(uint32_t i, uint32_t v) { e[i] = (uint16_t)v; }
};
struct BgzfNoSink {  // a member without text: nothing may be put
    void put(uint8_t) {}
    uint8_t back(uint32_t) const { return 0; }
};

struct BgzfPlan {
    std::vector<BgzfMember> members;  // the non-empty ones, in file order
    uint64_t usz = 0;                 // bytes of text
    uint64_t n_all = 0;               // members, the empty ones too
};

// Is the file of n bytes a chain of BGZF members that ends exactly at its end?  Every member: 1f 8b 08, FLG = FEXTRA alone, an
// extra subfield 'B' 'C' of two bytes (BSIZE), BSIZE + 1 bytes inside the file with room for header and trailer, ISIZE <= 65536.
// A member without text (the 28-byte end marker is one) gets no descriptor; its few deflate bytes are decoded here, so that what
// zlib would refuse in them is refused here too.  false: not for the device (plain gzip, other flag bits, a cut file, ...).
inline bool bgzf_plan(const unsigned char *p, uint64_t n, BgzfPlan &plan)
{
    plan.members.clear();
    plan.usz = plan.n_all = 0;
    auto le16 = [&](uint64_t at) { return (uint32_t)p[at] | (uint32_t)p[at + 1] << 8; };
    auto le32 = [&](uint64_t at) { return le16(at) | le16(at + 2) << 16; };
    uint64_t at = 0;
    while (at < n) {
        if (n - at < 12 + 6 + 8) return false;
        if (p[at] != 0x1f || p[at + 1] != 0x8b || p[at + 2] != 8 || p[at + 3] != 4) return false;
        const uint64_t xlen = le16(at + 10), x0 = at + 12;
        if (xlen > n - x0) return false;
        uint64_t q = x0;
        int64_t bsize = -1;
        while (x0 + xlen - q >= 4) {
            const uint64_t slen = le16(q + 2);
            if (slen > x0 + xlen - q - 4) return false;
            if (p[q] == 'B' && p[q + 1] == 'C') {
                if (slen != 2 || bsize >= 0) return false;
                bsize = le16(q + 4);
            }
            q += 4 + slen;
        }
        if (q != x0 + xlen || bsize < 0) return false;
        const uint64_t total = (uint64_t)bsize + 1;
        if (total > n - at || total < 12 + xlen + 8) return false;
        BgzfMember m;
        m.in_off = x0 + xlen;
        m.in_len = (uint32_t)(total - 12 - xlen - 8);
        m.crc = le32(at + total - 8);
        m.isize = le32(at + total - 4);
        m.out_off = plan.usz;
        m.head = (uint32_t)(12 + xlen);
        if (m.isize > BGZF_MAX_ISIZE) return false;
        if (m.isize) {
            plan.members.push_back(m);
            plan.usz += m.isize;
        } else {
            BgzfHostSrc src{p + m.in_off, m.in_len};
            BgzfHostTab tab;
            BgzfNoSink sink;
            if (m.crc != 0 || bgzf_inflate_member(src, sink, tab, 0u) != BGZF_OK) return false;
        }
        ++plan.n_all;
        at += total;
    }
    return true;
}

}  // namespace mxg
