// scan64_kernels.h -- exclusive 64-bit prefix sums in place, for the device writers whose offsets are bytes of a file (pathtext.hip:
// .path and AGP; synteny.hip: PAF): tile sums -> one block over the tile sums -> tiles.  The 32-bit scans are scan_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mxg {

constexpr uint32_t PT_TILE = 1024;  // elements per work-group of the scans (4 per thread)

// exclusive prefix of per-thread sums `c` inside a block of 256; *total = the block's sum (all threads call)
__device__ __forceinline__ uint64_t pt_block_exclusive(uint64_t c, uint64_t *sh, uint64_t *total)
{
    const uint32_t t = threadIdx.x;
    sh[t] = c;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint64_t v = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    *total = sh[255];
    __syncthreads();  // (sh is free for the next call)
    return incl - c;
}

static __global__ __launch_bounds__(256) void k_pt_tile_sum(const uint64_t *__restrict__ in, uint32_t n, uint64_t *__restrict__ tsum)
{
    __shared__ uint64_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * PT_TILE + threadIdx.x * 4u;
    uint64_t c = 0, total;
    for (uint32_t u = 0; u < 4; ++u)
        if (base + u < n) c += in[base + u];
    (void)pt_block_exclusive(c, sh, &total);
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// tsum[0 .. n_tiles) -> its exclusive sums, in place, by ONE block
static __global__ __launch_bounds__(256) void k_pt_scan_tiles(uint64_t *__restrict__ tsum, uint32_t n_tiles)
{
    __shared__ uint64_t sh[256];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_tiles; base += 256) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < n_tiles ? tsum[i] : 0;
        uint64_t total;
        const uint64_t ex = pt_block_exclusive(v, sh, &total);
        if (i < n_tiles) tsum[i] = carry + ex;
        carry += total;
    }
}

// a[i] -> the sum of a[0 .. i), in place (tsum: the tiles' exclusive sums)
static __global__ __launch_bounds__(256) void k_pt_tile_excl(uint64_t *__restrict__ a, uint32_t n, const uint64_t *__restrict__ tsum)
{
    __shared__ uint64_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * PT_TILE + threadIdx.x * 4u;
    uint64_t v[4], c = 0, total;
    for (uint32_t u = 0; u < 4; ++u) {
        v[u] = base + u < n ? a[base + u] : 0;
        c += v[u];
    }
    uint64_t run = tsum[blockIdx.x] + pt_block_exclusive(c, sh, &total);
    for (uint32_t u = 0; u < 4; ++u) {
        if (base + u < n) a[base + u] = run;
        run += v[u];
    }
}

// a[0 .. n) -> its exclusive sums, in place; tsum: (n + PT_TILE - 1) / PT_TILE words of scratch
static inline void launch_scan_u64(hipStream_t stream, uint64_t *a, uint32_t n, uint64_t *tsum)
{
    const uint32_t n_tiles = (n + PT_TILE - 1) / PT_TILE;
    hipLaunchKernelGGL(k_pt_tile_sum, dim3(n_tiles), dim3(256), 0, stream, a, n, tsum);
    hipLaunchKernelGGL(k_pt_scan_tiles, dim3(1), dim3(256), 0, stream, tsum, n_tiles);
    hipLaunchKernelGGL(k_pt_tile_excl, dim3(n_tiles), dim3(256), 0, stream, a, n, tsum);
}

}  // namespace mxg
