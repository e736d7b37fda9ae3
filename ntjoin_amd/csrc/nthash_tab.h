// nthash_tab.h -- the ntHash constants and the tables the device helpers of nthash_dev.h read, built on the host (SURVEY.md
// Appendix A.1).  Plain C++ with no HIP type in it: U4 is any struct of four 32-bit words x, y, z, w (HIP's uint4 in the
// library: host_io.cpp make_hash_tab / make_init_tab; a stand-in in tools/nthash_check.cpp, which runs the device helpers
// on the host against the oracle's direct formula).
#pragma once
#include <cstdint>
#include <vector>

namespace mxg {
namespace nttab {

static const uint64_t SEED[4] = {0x3c8bfbb395c60474ULL, 0x3193c18562a02b4cULL, 0x20323ed082572324ULL,
                                 0x295549f54be24456ULL};  // A C G T

inline uint64_t srol_n(uint64_t x, unsigned n)
{
    const uint64_t LO = 0x1FFFFFFFFULL;
    uint64_t lo = x & LO, hi = x >> 33;
    unsigned a = n % 33, b = n % 31;
    if (a) lo = ((lo << a) | (lo >> (33 - a))) & LO;
    if (b) hi = ((hi << b) | (hi >> (31 - b))) & 0x7FFFFFFFULL;
    return (hi << 33) | lo;
}

template <class U4>
inline U4 words(uint64_t f, uint64_t r)
{
    U4 e;
    e.x = (uint32_t)f, e.y = (uint32_t)(f >> 32), e.z = (uint32_t)r, e.w = (uint32_t)(r >> 32);
    return e;
}

// ntHash step table, 20 entries (out*4+in), out==4: warm-up step with no outgoing base (struct HashTab, mxg_internal.h)
template <class U4>
inline void hash_tab(uint32_t k, U4 *e)
{
    for (int o = 0; o < 5; ++o)
        for (int i = 0; i < 4; ++i) {
            uint64_t f = SEED[i], r = srol_n(SEED[3 - i], k);
            if (o < 4) {
                f ^= srol_n(SEED[o], k);
                r ^= SEED[3 - o];
            }
            e[o * 4 + i] = words<U4>(f, r);
        }
}

// Byte table of the direct hash formula (nthash_dev.h init_direct): the "warm-up state" after the first m = 4*(k/4) bases
// is  F = XOR_j srol^{m-1-j}(seed[c_j]),  R = XOR_j srol^{k-m+j}(seed'[c_j]).  Entry v (one packed byte = bases 4q..4q+3,
// base i in bits 2i..2i+1) holds the four terms of a byte at position 0: f4 = XOR_i srol^{3-i} seed[c_i],
// r4 = XOR_i srol^{i} seed'[c_i]; the byte's position enters through Horner rotations by 4 on the device.
template <class U4>
inline void init_tab(std::vector<U4> &out)
{
    out.assign(256 + 8 * 256, words<U4>(0, 0));
    for (uint32_t v = 0; v < 256; ++v) {
        uint64_t f = 0, r = 0;
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t c = (v >> (2 * i)) & 3u;
            f ^= srol_n(SEED[c], 3 - i);
            r ^= srol_n(SEED[3 - c], i);
        }
        out[v] = words<U4>(f, r);
        // position tables (nthash_dev.h init_pos): byte j of a group of 8 bytes (32 bases) contributes srol^{4(7-j)} f4 to the
        // forward hash and srol^{4j} r4 to the reverse-complement hash -- one lookup and four XORs per byte, no rotation
        for (uint32_t j = 0; j < 8; ++j) {
            const uint64_t fj = srol_n(f, 4 * (7 - j)), rj = srol_n(r, 4 * j);
            out[256 + j * 256 + v] = words<U4>(fj, rj);
        }
    }
}

// k = 32, init32_half: half[j][v] = {forward words of position table j + 4, reverse words of position table j}, j = 0..3, as
// k_hash_sparse gathers them from init_tab's entries into its LDS
template <class U4>
inline void half_tab(const std::vector<U4> &init, std::vector<U4> &out)
{
    out.resize(1024);
    for (uint32_t i = 0; i < 1024u; ++i) {
        const uint32_t j = i >> 8, v = i & 255u;
        const U4 f = init[256u + (j + 4u) * 256u + v], r = init[256u + j * 256u + v];
        U4 e;
        e.x = f.x, e.y = f.y, e.z = r.z, e.w = r.w;
        out[i] = e;
    }
}

}  // namespace nttab
}  // namespace mxg
