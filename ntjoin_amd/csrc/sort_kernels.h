// sort_kernels.h -- a stable LSD radix sort of 64-bit keys with a 32-bit payload for gfx950 (wave64), used by assess.hip: 8-bit
// digits, tiles of 1024 elements, per pass
//   k_rs_hist      per tile: its 256 digit counts (LDS atomics), stored digit-major: counts[digit * n_tiles + tile]
//   launch_scan_u32 over the counts: the first place of every (digit, tile)
//   k_rs_scatter   per tile: every element's rank among its tile's elements of the same digit, then the store
// Stability is the rank: wave w of a tile holds its elements [256 w, 256 w + 256), in four rounds of 64 by rising index.  In a
// round, the lanes of equal digit find one another with eight ballots (one per bit of the digit); a lane's rank is the number of
// such lanes below it plus what its wave has counted for the digit in earlier rounds (LDS, one row per wave); the rows of the waves
// in front of it are added once all four rounds are counted.  No atomics decide a place, so equal keys keep their order.
// The passes alternate between two buffers; launch_radix_sort returns which one holds the result.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "scan_kernels.h"

namespace mxg {

constexpr uint32_t RS_TILE = 1024;  // elements per work-group: 4 waves x 4 rounds x 64 lanes
constexpr uint32_t RS_BINS = 256;   // 8-bit digits

static __global__ __launch_bounds__(256) void k_rs_hist(const uint64_t *__restrict__ keys, uint32_t n, uint32_t shift, uint32_t n_tiles,
                                                        uint32_t *__restrict__ counts)
{
    __shared__ uint32_t h[RS_BINS];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * RS_TILE;
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
        const uint64_t i = base + u * 256u + threadIdx.x;
        if (i < n) atomicAdd(&h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    counts[(size_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];  // (256 threads: one digit each; blockIdx.x < n_tiles)
}

// first: the exclusive sums of counts.  Every element i < n is stored once, at a place below n (checked)
static __global__ __launch_bounds__(256) void k_rs_scatter(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t n, uint32_t shift,
                                                           uint32_t n_tiles, const uint32_t *__restrict__ first, uint64_t *__restrict__ keys_out,
                                                           uint32_t *__restrict__ vals_out)
{
    __shared__ uint32_t cnt[4][RS_BINS];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * RS_TILE + wv * 256u;
    uint64_t key[4];
    uint32_t val[4], rank[4];
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint64_t i = base + r * 64u + lane;
        const bool ok = i < n;
        key[r] = ok ? keys[i] : 0;
        val[r] = ok ? vals[i] : 0;
        const uint32_t d = (uint32_t)(key[r] >> shift) & 255u;
        uint64_t peers = __ballot(ok);  // the lanes of this round that hold an element of digit d
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t seen = cnt[wv][d];
        rank[r] = seen + (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        __syncthreads();  // (every lane has read its count before the digit's last lane raises it)
        if (ok && (peers >> lane) == 1ull) cnt[wv][d] = seen + (uint32_t)__popcll(peers);
        __syncthreads();
    }
    {  // thread t: digit t's first place for every wave of the tile
        const uint32_t c0 = cnt[0][threadIdx.x], c1 = cnt[1][threadIdx.x], c2 = cnt[2][threadIdx.x];
        const uint32_t g = first[(size_t)threadIdx.x * n_tiles + blockIdx.x];
        cnt[0][threadIdx.x] = g;
        cnt[1][threadIdx.x] = g + c0;
        cnt[2][threadIdx.x] = g + c0 + c1;
        cnt[3][threadIdx.x] = g + c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint64_t i = base + r * 64u + lane;
        if (i >= n) continue;
        const uint32_t at = cnt[wv][(uint32_t)(key[r] >> shift) & 255u] + rank[r];
        if (at >= n) continue;  // (cannot be: the counts of all tiles sum to n)
        keys_out[at] = key[r];
        vals_out[at] = val[r];
    }
}

constexpr uint32_t rs_tiles(uint32_t n) { return (n + RS_TILE - 1) / RS_TILE; }
// words of `counts` and of `first`, and of `bsum` (launch_scan_u32's scratch), for n elements
constexpr size_t rs_count_words(uint32_t n) { return (size_t)rs_tiles(n) * RS_BINS; }
constexpr size_t rs_bsum_words(uint32_t n) { return (rs_count_words(n) + TILE - 1) / TILE + 4; }

// Sorts n (key, value) pairs by the low key_bits bits of the keys (the bits above them must be equal in all keys), stably.
// (k0, v0) holds the input and, with (k1, v1), n elements each; returns 0 when the result lies in (k0, v0), 1 when in (k1, v1).
// n < 2^31; total: a device word the scans may write.
static inline int launch_radix_sort(hipStream_t stream, uint64_t *k0, uint32_t *v0, uint64_t *k1, uint32_t *v1, uint32_t n, uint32_t key_bits,
                                    uint32_t *counts, uint32_t *first, uint32_t *bsum, uint64_t *total)
{
    if (n < 2) return 0;
    const uint32_t n_tiles = rs_tiles(n);
    int at = 0;
    for (uint32_t shift = 0; shift < key_bits && shift < 64; shift += 8, at ^= 1) {
        const uint64_t *ki = at ? k1 : k0;
        const uint32_t *vi = at ? v1 : v0;
        hipLaunchKernelGGL(k_rs_hist, dim3(n_tiles), dim3(256), 0, stream, ki, n, shift, n_tiles, counts);
        launch_scan_u32(stream, counts, n_tiles * RS_BINS, bsum, first, total);
        hipLaunchKernelGGL(k_rs_scatter, dim3(n_tiles), dim3(256), 0, stream, ki, vi, n, shift, n_tiles, first, at ? k0 : k1, at ? v0 : v1);
    }
    return at;
}

}  // namespace mxg
