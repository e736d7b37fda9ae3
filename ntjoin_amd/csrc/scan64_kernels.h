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

// ---- the running 64-bit maximum (assess.hip: the cover of the chains; lift.hip: the index of a piece table) -------------------------
// inside a block of 256: the maximum of the values of the threads in front of this one (0 for thread 0); *total = the block's
__device__ __forceinline__ uint64_t pt_block_exclusive_max(uint64_t c, uint64_t *sh, uint64_t *total)
{
    const uint32_t t = threadIdx.x;
    sh[t] = c;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint64_t v = t >= o ? sh[t - o] : 0;
        __syncthreads();
        if (v > sh[t]) sh[t] = v;
        __syncthreads();
    }
    const uint64_t ex = t ? sh[t - 1] : 0;
    *total = sh[255];
    __syncthreads();  // (sh is free for the next call)
    return ex;
}

static __global__ __launch_bounds__(256) void k_pt_max_tile(const uint64_t *__restrict__ in, uint32_t n, uint64_t *__restrict__ tmax)
{
    __shared__ uint64_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * PT_TILE + threadIdx.x * 4u;
    uint64_t c = 0, total;
    for (uint32_t u = 0; u < 4; ++u)
        if (base + u < n && in[base + u] > c) c = in[base + u];
    (void)pt_block_exclusive_max(c, sh, &total);
    if (threadIdx.x == 0) tmax[blockIdx.x] = total;
}

// tmax[0 .. n_tiles) -> the maximum of the tiles in front of each, in place, by ONE block
static __global__ __launch_bounds__(256) void k_pt_max_tiles(uint64_t *__restrict__ tmax, uint32_t n_tiles)
{
    __shared__ uint64_t sh[256];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_tiles; base += 256) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < n_tiles ? tmax[i] : 0;
        uint64_t total;
        const uint64_t ex = pt_block_exclusive_max(v, sh, &total);
        if (i < n_tiles) tmax[i] = ex > carry ? ex : carry;
        if (total > carry) carry = total;
    }
}

// a[i] -> the maximum of a[0 .. i], in place (tmax: the maximum of the tiles in front of each tile)
static __global__ __launch_bounds__(256) void k_pt_max_incl(uint64_t *__restrict__ a, uint32_t n, const uint64_t *__restrict__ tmax)
{
    __shared__ uint64_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * PT_TILE + threadIdx.x * 4u;
    uint64_t v[4], c = 0, total;
    for (uint32_t u = 0; u < 4; ++u) {
        v[u] = base + u < n ? a[base + u] : 0;
        if (v[u] > c) c = v[u];
    }
    uint64_t run = pt_block_exclusive_max(c, sh, &total);
    if (tmax[blockIdx.x] > run) run = tmax[blockIdx.x];
    for (uint32_t u = 0; u < 4; ++u) {
        if (base + u >= n) break;
        if (v[u] > run) run = v[u];
        a[base + u] = run;
    }
}

// a[0 .. n) -> its inclusive running maxima, in place; tmax: (n + PT_TILE - 1) / PT_TILE words of scratch
static inline void launch_max_scan_u64(hipStream_t stream, uint64_t *a, uint32_t n, uint64_t *tmax)
{
    const uint32_t n_tiles = (n + PT_TILE - 1) / PT_TILE;
    hipLaunchKernelGGL(k_pt_max_tile, dim3(n_tiles), dim3(256), 0, stream, a, n, tmax);
    hipLaunchKernelGGL(k_pt_max_tiles, dim3(1), dim3(256), 0, stream, tmax, n_tiles);
    hipLaunchKernelGGL(k_pt_max_incl, dim3(n_tiles), dim3(256), 0, stream, a, n, tmax);
}

}  // namespace mxg
