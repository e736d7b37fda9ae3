// The byte source, byte sink and table storage k_bgzf_inflate (bgzf.hip) hands to the decoder of bgzf_inflate.h, one set per lane.
// Plain C++ like the decoder itself, so that a CPU test (tests/test_bgzf_craft_cpu.py, also under the sanitizers) compiles the same
// text: there the "device buffers" are heap blocks of exactly the device's sizes and the "LDS" is an array for 64 lanes.
#pragma once
#include "bgzf_inflate.h"

namespace mxg {

constexpr uint32_t BGZF_BLOCK = 64;  // lanes = members per block
static_assert(BGZF_TAB_ELEMS % 2 == 0, "two entries per LDS word");
static_assert((BGZF_TAB_ELEMS / 2) * BGZF_BLOCK * 4 + 1024 <= 64 * 1024, "tables + CRC table fit a block's LDS");

struct BgzfLdsTab {
    uint16_t *lane;  // the lane's first entry: entries e and e + 1 (e even) share a word, the next pair is 64 words on
    MXG_BGZF_FN uint32_t get(uint32_t e) const { return lane[(e >> 1) * (2u * BGZF_BLOCK) + (e & 1u)]; }
    MXG_BGZF_FN void set(uint32_t e, uint32_t v) { lane[(e >> 1) * (2u * BGZF_BLOCK) + (e & 1u)] = (uint16_t)v; }
};

struct BgzfDevSrc {
    const unsigned char *p;  // the member's deflate data
    uint32_t n;
    uint32_t have = 0xFFFFFFFFu, word = 0;  // the aligned word fetched last (members start at any byte; the buffer ends on a whole word)
    MXG_BGZF_FN uint32_t len() const { return n; }
    MXG_BGZF_FN uint32_t byte(uint32_t i)  // i < n
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p) + i;
        const uint32_t w = (uint32_t)(a >> 2);
        if (w != have) {
            word = *reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
            have = w;
        }
        return (word >> (8u * ((uint32_t)a & 3u))) & 255u;
    }
};

struct BgzfDevSink {
    unsigned char *out;  // the member's text
    const uint32_t *crc_tab;
    uint32_t n = 0, acc = 0, pend = 0, crc = 0xFFFFFFFFu;  // bytes put, the word being filled, its bytes so far
    MXG_BGZF_FN uint32_t lane_of(uint32_t i) const { return 8u * ((uint32_t)(reinterpret_cast<uintptr_t>(out) + i) & 3u); }
    MXG_BGZF_FN void flush()
    {
        if (pend == 4u) *reinterpret_cast<uint32_t *>(out + n - 4u) = acc;  // (n - 4 is the word's first byte: it ends at n)
        else
            for (uint32_t i = n - pend; i < n; ++i) out[i] = (unsigned char)(acc >> lane_of(i));
        pend = 0;
        acc = 0;
    }
    MXG_BGZF_FN void put(uint8_t b)  // the decoder has counted the byte against ISIZE
    {
        crc = crc_tab[(crc ^ b) & 255u] ^ (crc >> 8);
        const uint32_t sh = lane_of(n);
        acc |= (uint32_t)b << sh;
        ++n;
        ++pend;
        if (sh == 24u) flush();
    }
    MXG_BGZF_FN uint8_t back(uint32_t d) const  // 1 <= d <= n
    {
        const uint32_t i = n - d;
        return d <= pend ? (uint8_t)(acc >> lane_of(i)) : out[i];
    }
};

}  // namespace mxg
