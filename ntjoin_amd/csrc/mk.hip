// mk.hip -- the per-run statistics of ntJoin's --mkt orientation test: determine_orientation (reference
// bin/ntjoin_assemble.py:30-50) hands every run of positions that is not strictly monotone to
// pymannkendall.original_test, whose decision reads two exact integers of the run x_0 .. x_{n-1}:
//   s         = sum over i < j of sign(x_j - x_i)                                   (int64)
//   tie_term  = sum over groups of t equal values of t(t-1)(2t+5)                   (uint64; 0 when all values differ)
//             = sum over i of (t_i - 1)(2 t_i + 5), t_i = number of values equal to x_i
// original_test does both in O(n^2) (and Sen's slope in O(n^2) memory); here:
//   runs of <= 64 values   one wave per run: lane i holds x_i and meets every other value through a broadcast (s, t_i)
//   longer runs            merge sort that counts while it merges.  Tiles of MK_TILE values (a run's own, from its first
//                          value on) are sorted in LDS; global levels then merge sorted blocks of width w = MK_TILE,
//                          2 MK_TILE, ... pairwise, launched over the runs longer than w only.  Every element of a left block
//                          has an earlier index than every element of its right block, so a right element x adds
//                          #left < x - #left > x to s (lower / upper bound by binary search); every element moves to its
//                          co-rank (ties: left before right).  s partials are summed per wave and added with one 64-bit
//                          atomic per run and wave: integer sums, so the result does not depend on arrival order.  Once a
//                          run is sorted, every value with an equal neighbour finds its group by binary search (t_i).
// The tie term's per-value parts are summed as low / high 32-bit halves; the host joins them and reports a total beyond
// 2^64 - 1 (a group of more than about 2 * 10^6 equal values) as an error.
#include <algorithm>

#include "bisect.h"
#include "mxg_internal.h"

namespace mxg {

static constexpr uint32_t MK_SHORT = 64;   // runs up to this long: one wave each
static constexpr uint32_t MK_TILE = 2048;  // values sorted in LDS by one block of 256 threads (power of two)
enum { MK_X, MK_ALT, MK_FIRST, MK_TAB, MK_OUT, MK_BUF_COUNT };
static_assert(MK_BUF_COUNT <= 8, "mxg_handle::mkbuf too small");

__device__ __forceinline__ uint64_t mk_wave_sum(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// arr[key] += the sum of `val` over the lanes that hold `key` (all 64 lanes must be here; `active` lanes contribute)
__device__ __forceinline__ void mk_add_by_key(unsigned long long *arr, uint32_t key, bool active, uint64_t val)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t todo = __ballot(active); todo;) {
        const int leader = __builtin_ctzll(todo);
        const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);
        const bool mine = active && key == k0;
        const uint64_t same = __ballot(mine);
        const uint64_t tot = mk_wave_sum(mine ? val : 0);
        if ((int)lane == leader && tot) atomicAdd(&arr[k0], (unsigned long long)tot);
        todo &= ~same;
    }
}

// One merge of sorted blocks of width w (a power of two) inside a run a[0, n): where element o (= x) goes, and what it adds
// to s.  The blocks [p0, p0 + w) and [p0 + w, p0 + 2w) merge into [p0, min(p0 + 2w, n)): destinations are distinct and < n.
__device__ __forceinline__ uint32_t mk_merge_dest(const uint32_t *a, uint32_t n, uint32_t o, uint32_t x, uint32_t w, int64_t &s)
{
    const uint32_t p0 = o & ~(2 * w - 1);
    if (o - p0 < w) {  // left block: behind the right block's values < x
        const uint32_t r0 = p0 + w;
        return r0 < n ? o + first_ge(a + r0, 0u, min(w, n - r0), x) : o;
    }
    // right block (its left block is full); the upper bound needs a second search only where x occurs in the left block
    const uint32_t lb = first_ge(a + p0, 0u, w, x);
    const uint32_t ub = lb < w && a[p0 + lb] == x ? lb + first_gt(a + p0 + lb, 0u, w - lb, x) : lb;
    s += (int64_t)lb - (int64_t)(w - ub);
    return o - w + ub;
}

// one wave per run: runs of <= MK_SHORT values complete; longer runs start at s = tie_term = 0 (the merge kernels add to them)
__global__ __launch_bounds__(256) void mk_short(const uint32_t *__restrict__ x, const uint32_t *__restrict__ first, uint32_t n_runs,
                                                unsigned long long *s_out, unsigned long long *tlo, unsigned long long *thi)
{
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (r >= n_runs) return;  // (uniform per wave)
    const uint32_t lo = first[r], n = first[r + 1] - lo;
    if (n > MK_SHORT) {
        if (lane == 0) s_out[r] = tlo[r] = thi[r] = 0;
        return;
    }
    const uint32_t xi = lane < n ? x[lo + lane] : 0u;
    int s = 0;
    uint32_t t = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t xj = (uint32_t)__shfl((int)xi, (int)j, 64);
        s += j > lane ? (int)(xj > xi) - (int)(xj < xi) : 0;
        t += xj == xi;
    }
    const uint64_t sum_s = mk_wave_sum(lane < n ? (uint64_t)(int64_t)s : 0);
    const uint64_t sum_t = mk_wave_sum(lane < n ? (uint64_t)(t - 1) * (2 * t + 5) : 0);
    if (lane == 0) {
        s_out[r] = sum_s;
        tlo[r] = sum_t;
        thi[r] = 0;
    }
}

// long runs: tile b of the list, sorted in place through LDS; its s partial added to the run
__global__ __launch_bounds__(256) void mk_tiles(uint32_t *x, const uint32_t *__restrict__ first, const uint32_t *__restrict__ lr_run,
                                                const uint32_t *__restrict__ lr_tile0, uint32_t m, unsigned long long *s_out)
{
    __shared__ uint32_t buf[2][MK_TILE];
    const uint32_t k = last_le(lr_tile0, 0u, m, blockIdx.x), r = lr_run[k];  // (lr_tile0[0] = 0, lr_tile0 increasing)
    const uint32_t q0 = (blockIdx.x - lr_tile0[k]) * MK_TILE;
    const uint32_t base = first[r] + q0, n = min(MK_TILE, first[r + 1] - first[r] - q0);
    for (uint32_t i = threadIdx.x; i < n; i += 256) buf[0][i] = x[base + i];
    __syncthreads();
    int64_t s = 0;
    int cur = 0;
    for (uint32_t w = 1; w < n; w <<= 1) {
        const uint32_t *src = buf[cur];
        uint32_t *dst = buf[cur ^ 1];
        for (uint32_t i = threadIdx.x; i < n; i += 256) {
            const uint32_t v = src[i];
            dst[mk_merge_dest(src, n, i, v, w, s)] = v;
        }
        __syncthreads();
        cur ^= 1;
    }
    for (uint32_t i = threadIdx.x; i < n; i += 256) x[base + i] = buf[cur][i];
    const uint64_t tot = mk_wave_sum((uint64_t)s);
    if ((threadIdx.x & 63u) == 0 && tot) atomicAdd(&s_out[r], (unsigned long long)tot);
}

// one global level: the first m long runs (those longer than w) merge their sorted blocks of width w, src -> dst
__global__ __launch_bounds__(256) void mk_level(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst,
                                                const uint32_t *__restrict__ first, const uint32_t *__restrict__ lr_run,
                                                const uint32_t *__restrict__ lr_off, uint32_t m, uint32_t n_elem, uint32_t w,
                                                unsigned long long *s_out)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const bool in = g < n_elem;
    uint32_t r = 0;
    int64_t s = 0;
    if (in) {
        const uint32_t k = last_le(lr_off, 0u, m, g);  // (lr_off[0] = 0, lr_off increasing)
        r = lr_run[k];
        const uint32_t o = g - lr_off[k], f = first[r], n = first[r + 1] - f;
        const uint32_t v = src[f + o];
        dst[f + mk_merge_dest(src + f, n, o, v, w, s)] = v;
    }
    mk_add_by_key(s_out, r, in, (uint64_t)s);
}

// every long run is sorted (in x0 or x1: the parity of the global levels it went through): (t_i - 1)(2 t_i + 5) per value
__global__ __launch_bounds__(256) void mk_ties(const uint32_t *__restrict__ x0, const uint32_t *__restrict__ x1,
                                               const uint32_t *__restrict__ first, const uint32_t *__restrict__ lr_run,
                                               const uint32_t *__restrict__ lr_off, uint32_t m, uint32_t n_elem,
                                               unsigned long long *tlo, unsigned long long *thi)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const bool in = g < n_elem;
    uint32_t r = 0;
    uint64_t term = 0;
    if (in) {
        const uint32_t k = last_le(lr_off, 0u, m, g);  // (lr_off[0] = 0, lr_off increasing)
        r = lr_run[k];
        const uint32_t o = g - lr_off[k], f = first[r], n = first[r + 1] - f;
        uint32_t odd = 0;
        for (uint64_t w = MK_TILE; w < n; w <<= 1) odd ^= 1u;
        const uint32_t *a = (odd ? x1 : x0) + f;
        const uint32_t v = a[o];
        if ((o > 0 && a[o - 1] == v) || (o + 1 < n && a[o + 1] == v)) {
            const uint64_t t = first_gt(a, 0u, n, v) - first_ge(a, 0u, n, v);
            term = (t - 1) * (2 * t + 5);
        }
    }
    mk_add_by_key(tlo, r, in, term & 0xFFFFFFFFull);
    mk_add_by_key(thi, r, in, term >> 32);
}

int mk_runs(mxg_handle *h, uint32_t *d_x, const uint32_t *d_first, uint32_t n_runs, uint32_t n_total,
            const std::vector<uint32_t> &len, int64_t *s, uint64_t *tie_term)
{
    if (n_runs == 0) return MXG_OK;
    DevBuf *B = h->mkbuf;
    const dim3 b(256);
    // the long runs, longest first: those a global level of width w merges are then a prefix of the list
    std::vector<uint32_t> ids;
    for (uint32_t r = 0; r < n_runs; ++r)
        if (len[r] > MK_SHORT) ids.push_back(r);
    std::stable_sort(ids.begin(), ids.end(), [&](uint32_t a, uint32_t c) { return len[a] > len[c]; });
    const uint32_t m = (uint32_t)ids.size();
    std::vector<uint32_t> tab(3 * (size_t)m + 2, 0u);  // lr_run[m] | lr_tile0[m + 1] | lr_off[m + 1]
    uint32_t *lr_run = tab.data(), *lr_tile0 = lr_run + m, *lr_off = lr_tile0 + m + 1;
    for (uint32_t k = 0; k < m; ++k) {
        lr_run[k] = ids[k];
        lr_tile0[k + 1] = lr_tile0[k] + (len[ids[k]] + MK_TILE - 1) / MK_TILE;
        lr_off[k + 1] = lr_off[k] + len[ids[k]];
    }
    MXG_HIP(h, B[MK_OUT].ensure((size_t)n_runs * 24 + 16));
    unsigned long long *d_s = B[MK_OUT].as<unsigned long long>(), *d_tlo = d_s + n_runs, *d_thi = d_tlo + n_runs;
    hipLaunchKernelGGL(mk_short, dim3((n_runs + 3) / 4), b, 0, h->stream, d_x, d_first, n_runs, d_s, d_tlo, d_thi);
    MXG_HIP(h, hipGetLastError());
    if (m) {
        MXG_HIP(h, B[MK_TAB].ensure(tab.size() * 4));
        MXG_HIP(h, B[MK_ALT].ensure((size_t)n_total * 4 + 16));
        MXG_HIP(h, hipMemcpyAsync(B[MK_TAB].p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, h->stream));
        const uint32_t *t_run = B[MK_TAB].as<uint32_t>(), *t_tile0 = t_run + m, *t_off = t_tile0 + m + 1;
        uint32_t *d_alt = B[MK_ALT].as<uint32_t>();
        hipLaunchKernelGGL(mk_tiles, dim3(lr_tile0[m]), b, 0, h->stream, d_x, d_first, t_run, t_tile0, m, d_s);
        int cur = 0;
        uint32_t m_w = m;
        for (uint64_t w = MK_TILE; w < len[ids[0]]; w <<= 1) {
            while (len[ids[m_w - 1]] <= w) --m_w;  // (ids[0] is longer than w)
            const uint32_t n_elem = lr_off[m_w];
            hipLaunchKernelGGL(mk_level, dim3((n_elem + 255) / 256), b, 0, h->stream, cur ? d_alt : d_x, cur ? d_x : d_alt,
                               d_first, t_run, t_off, m_w, n_elem, (uint32_t)w, d_s);
            cur ^= 1;
        }
        hipLaunchKernelGGL(mk_ties, dim3((lr_off[m] + 255) / 256), b, 0, h->stream, d_x, d_alt, d_first, t_run, t_off, m, lr_off[m],
                           d_tlo, d_thi);
        MXG_HIP(h, hipGetLastError());
    }
    std::vector<uint64_t> out((size_t)n_runs * 3);
    MXG_HIP(h, hipMemcpyAsync(out.data(), d_s, out.size() * 8, hipMemcpyDeviceToHost, h->stream));
    MXG_HIP(h, hipStreamSynchronize(h->stream));
    const uint64_t *o_s = out.data(), *o_lo = o_s + n_runs, *o_hi = o_lo + n_runs;
    for (uint32_t r = 0; r < n_runs; ++r)
        if (o_hi[r] >> 32 || (o_hi[r] << 32) + o_lo[r] < o_lo[r])
            return set_err(h, MXG_ELIMIT, "Mann-Kendall tie term of run %u exceeds 2^64 - 1 (a group of more than about 2e6 equal "
                           "values)", r);
    for (uint32_t r = 0; r < n_runs; ++r) {
        s[r] = (int64_t)o_s[r];
        tie_term[r] = (o_hi[r] << 32) + o_lo[r];
    }
    return MXG_OK;
}

int mk_stats(mxg_handle *h, const uint32_t *values, const uint64_t *run_first, uint64_t n_runs, int64_t *s, uint64_t *tie_term)
{
    if (n_runs == 0) return MXG_OK;
    const uint64_t n_total = run_first[n_runs];
    if (n_runs >= 0x7FFFFFFFull || n_total >= 0x7FFFFFFFull)
        return set_err(h, MXG_ELIMIT, "mxg_mk_stats: %llu runs of %llu values in all (at most 2^31 - 2 each)",
                       (unsigned long long)n_runs, (unsigned long long)n_total);
    std::vector<uint32_t> first(n_runs + 1), len(n_runs);
    for (uint64_t r = 0; r <= n_runs; ++r) {
        if (r && run_first[r] < run_first[r - 1])
            return set_err(h, MXG_EINVAL, "mxg_mk_stats: run_first decreases at run %llu", (unsigned long long)r);
        first[r] = (uint32_t)run_first[r];
        if (r) len[r - 1] = first[r] - first[r - 1];
    }
    MXG_HIP(h, hipSetDevice(h->device));
    DevBuf *B = h->mkbuf;
    MXG_HIP(h, B[MK_X].ensure(n_total * 4 + 16));
    MXG_HIP(h, B[MK_FIRST].ensure(first.size() * 4));
    if (n_total) MXG_HIP(h, hipMemcpyAsync(B[MK_X].p, values, n_total * 4, hipMemcpyHostToDevice, h->stream));
    MXG_HIP(h, hipMemcpyAsync(B[MK_FIRST].p, first.data(), first.size() * 4, hipMemcpyHostToDevice, h->stream));
    return mk_runs(h, B[MK_X].as<uint32_t>(), B[MK_FIRST].as<uint32_t>(), (uint32_t)n_runs, (uint32_t)n_total, len, s, tie_term);
}

}  // namespace mxg
