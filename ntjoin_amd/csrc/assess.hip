// assess.hip -- mxg_synteny_assess: chains of the kept synteny blocks, the breakpoints between them, and the summary a reference-based
// assessment reads first: aligned and covered bases, NA50 / NGA50 / NG50, misassembly counts (include/ntjoin_mx.h, row f13; the rules
// themselves are assess.h; the sort is sort_kernels.h).  The blocks come from the host copy the blocks view holds;
// everything per block, chain, chain boundary or length runs on the device:
//   k_as_heads     per block: is it the head of a chain (not joined to its predecessor: two bisections into the record's piece
//                  offsets), and its anchor count for the scan behind
//   scan, scan     over the head flags (a block's chain = the heads at or before it, less one) and over the anchor counts
//   k_as_ends      per block: a head stores itself as its chain's first block, a block in front of a head as its chain's last
//   k_as_chains    per chain: its fields from its first and last block, its key in subject order, the two sums of spans
//   k_as_bp_flag   per chain boundary: is it a breakpoint, its kind and whether it falls on a join; six counters per thread block
//                  in LDS, then one atomic each
//   scan, k_as_bp_emit   the breakpoints, in order
//   sort           chains by (s_record, s_start)
//   k_as_cover_words, k_pt_max_tile, k_pt_max_tiles, k_as_cover   the running maximum of (s_record, s_end) in front of every chain
//                  -- a plain 64-bit max scan, see assess.h -- gives what the chain adds to the union; their sum
//   k_as_span_keys / k_as_len_keys, sort, k_as_lens, 64-bit scan, k_as_nx   lengths descending, their running sums, and per x one
//                  lower bound: once over the chains' query spans (na, nga), once over the query's record lengths (ng)
// Two host syncs: the number of chains (it sizes the chain arrays), and the end.  Plain loads and stores throughout; every write is
// at an index below the size its array was allocated for (see the launches).
#include <algorithm>

#include "assess.h"
#include "mxg_internal.h"
#include "scan64_kernels.h"
#include "scan_kernels.h"
#include "sort_kernels.h"

namespace mxg {

enum { AB_BLK, AB_PRE, AB_FIRST, AB_HEAD, AB_HSCAN, AB_ACNT, AB_ASCAN, AB_BSUM, AB_CFIRST, AB_CLAST, AB_CHAIN, AB_BPFLAG, AB_BPSCAN, AB_BPKJ, AB_BP,
       AB_SUM, AB_K0, AB_K1, AB_V0, AB_V1, AB_COUNTS, AB_RFIRST, AB_RBSUM, AB_CW, AB_TMAX, AB_LEN64, AB_TSUM, AB_QLEN, AB_BUF_COUNT };
static_assert(AB_BUF_COUNT <= 32, "mxg_handle::asbuf too small");
constexpr uint32_t AS_BP_FIELDS = 5;

__global__ __launch_bounds__(256) void k_as_heads(const uint32_t *__restrict__ blk, uint32_t n, uint32_t k, const mxg_assess_params p,
                                                  const uint32_t *__restrict__ pre, const uint32_t *__restrict__ first, uint32_t *__restrict__ head,
                                                  uint32_t *__restrict__ acnt)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        acnt[n] = 0;  // (so that the exclusive sums end with the total)
        return;
    }
    const SynBlock b = as_block(blk, n, i);
    head[i] = (i == 0 || !as_joined(as_block(blk, n, i - 1u), b, k, p, pre, first)) ? 1u : 0u;
    acnt[i] = b.n_anchors;
}

__global__ __launch_bounds__(256) void k_as_ends(const uint32_t *__restrict__ head, const uint32_t *__restrict__ hscan, uint32_t n, uint32_t n_ch,
                                                 uint32_t *__restrict__ cfirst, uint32_t *__restrict__ clast)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t hd = head[i], c = hscan[i] + hd - 1u;  // (block 0 is a head: hscan + hd >= 1)
    if (c >= n_ch) return;                                // (cannot be: hscan counts the heads in front of i)
    if (hd) cfirst[c] = i;
    if (i + 1u == n || head[i + 1u]) clast[c] = i;
}

// chain: ten arrays of n_ch words, in the order of AsChain's fields
__global__ __launch_bounds__(256) void k_as_chains(const uint32_t *__restrict__ blk, uint32_t n, const uint32_t *__restrict__ cfirst,
                                                   const uint32_t *__restrict__ clast, const uint32_t *__restrict__ ascan, uint32_t n_ch,
                                                   uint32_t *__restrict__ chain, uint64_t *__restrict__ key, uint32_t *__restrict__ val,
                                                   unsigned long long *__restrict__ sum)
{
    __shared__ uint64_t sh[256];
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    uint64_t aligned = 0, chained = 0;
    if (c < n_ch) {
        uint32_t f = cfirst[c], l = clast[c];
        if (f > l || l >= n) f = l = 0;  // (cannot be: every chain has one head and, at or behind it, one last block)
        const AsChain o = as_chain(as_block(blk, n, f), as_block(blk, n, l), f, l, ascan[l + 1u] - ascan[f]);
        const uint32_t fld[AS_CHAIN_FIELDS] = {o.n_blocks, o.first_block, o.n_anchors, o.q_record, o.q_start, o.q_end, o.s_record, o.s_start, o.s_end, o.reverse};
#pragma unroll
        for (uint32_t u = 0; u < AS_CHAIN_FIELDS; ++u) chain[(size_t)u * n_ch + c] = fld[u];
        key[c] = as_place_key(o.s_record, o.s_start);
        val[c] = c;
        aligned = o.q_end - o.q_start;
        chained = o.s_end - o.s_start;
    }
    uint64_t total;
    (void)pt_block_exclusive(aligned, sh, &total);
    if (threadIdx.x == 0 && total) atomicAdd(sum + AS_ALIGNED, (unsigned long long)total);
    (void)pt_block_exclusive(chained, sh, &total);
    if (threadIdx.x == 0 && total) atomicAdd(sum + AS_CHAINED, (unsigned long long)total);
}

// per chain c: is (c, c + 1) a breakpoint; kj = kind * 2 + at_join
__global__ __launch_bounds__(256) void k_as_bp_flag(const uint32_t *__restrict__ chain, uint32_t n_ch, const uint32_t *__restrict__ blk, uint32_t n,
                                                    const uint32_t *__restrict__ pre, const uint32_t *__restrict__ first, uint32_t *__restrict__ flag,
                                                    uint32_t *__restrict__ kj, unsigned long long *__restrict__ sum)
{
    __shared__ uint32_t cnt[6];
    if (threadIdx.x < 6) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < n_ch) {
        uint32_t f = 0, v = 0;
        const uint32_t *q_rec = chain + (size_t)3 * n_ch, *s_rec = chain + (size_t)6 * n_ch, *rev = chain + (size_t)9 * n_ch;
        if (c + 1u < n_ch && q_rec[c] == q_rec[c + 1u]) {
            const uint32_t la = chain[(size_t)n_ch + c] + chain[c] - 1u, fb = chain[(size_t)n_ch + c + 1u];  // last block of c, first of c + 1
            if (la < n && fb < n) {
                f = 1;
                v = as_kind(s_rec[c], rev[c], s_rec[c + 1u], rev[c + 1u]) * 2u + (as_at_join(as_block(blk, n, la), as_block(blk, n, fb), pre, first) ? 1u : 0u);
                atomicAdd(&cnt[v], 1u);
            }
        }
        flag[c] = f;
        kj[c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6 && cnt[threadIdx.x]) atomicAdd(sum + AS_BP0 + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

// bp: five arrays of n_ch words (as many as there could be): chain, kind, at_join, q_lo, q_hi
__global__ __launch_bounds__(256) void k_as_bp_emit(const uint32_t *__restrict__ chain, uint32_t n_ch, const uint32_t *__restrict__ flag,
                                                    const uint32_t *__restrict__ scan, const uint32_t *__restrict__ kj, uint32_t *__restrict__ bp)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c + 1u >= n_ch || !flag[c]) return;
    const uint32_t at = scan[c];
    if (at >= n_ch) return;  // (cannot be: scan counts the breakpoints in front of c)
    bp[at] = c;
    bp[(size_t)n_ch + at] = kj[c] >> 1;
    bp[(size_t)2 * n_ch + at] = kj[c] & 1u;
    bp[(size_t)3 * n_ch + at] = chain[(size_t)5 * n_ch + c];       // q_end[c]
    bp[(size_t)4 * n_ch + at] = chain[(size_t)4 * n_ch + c + 1u];  // q_start[c + 1]
}

// ---- the union of the subject intervals ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_as_cover_words(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, const uint32_t *__restrict__ s_end,
                                                        uint32_t n_ch, uint64_t *__restrict__ cw)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_ch) return;
    const uint32_t c = val[j];
    cw[j] = c < n_ch ? as_cover_word((uint32_t)(key[j] >> 32), s_end[c]) : 0;  // (c < n_ch: the payloads are a permutation)
}

// (the running maximum itself: pt_block_exclusive_max, k_pt_max_tile, k_pt_max_tiles of scan64_kernels.h)
__global__ __launch_bounds__(256) void k_as_cover(const uint64_t *__restrict__ key, const uint64_t *__restrict__ cw, uint32_t n,
                                                  const uint64_t *__restrict__ tmax, unsigned long long *__restrict__ sum)
{
    __shared__ uint64_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * PT_TILE + threadIdx.x * 4u;
    uint64_t v[4], c = 0, total;
    for (uint32_t u = 0; u < 4; ++u) {
        v[u] = base + u < n ? cw[base + u] : 0;
        if (v[u] > c) c = v[u];
    }
    uint64_t run = pt_block_exclusive_max(c, sh, &total);
    if (tmax[blockIdx.x] > run) run = tmax[blockIdx.x];
    uint64_t add = 0;
    for (uint32_t u = 0; u < 4; ++u) {
        if (base + u >= n) break;
        const uint64_t kx = key[base + u];
        add += as_uncovered(run, (uint32_t)(kx >> 32), (uint32_t)kx, (uint32_t)v[u]);
        if (v[u] > run) run = v[u];
    }
    (void)pt_block_exclusive(add, sh, &total);
    if (threadIdx.x == 0 && total) atomicAdd(sum + AS_COVERED, (unsigned long long)total);
}

// ---- Nx ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_as_span_keys(const uint32_t *__restrict__ q_start, const uint32_t *__restrict__ q_end, uint32_t n,
                                                      uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    key[j] = as_len_key(q_end[j] - q_start[j]);
    val[j] = j;
}

__global__ __launch_bounds__(256) void k_as_len_keys(const uint32_t *__restrict__ len, uint32_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    key[j] = as_len_key(len[j]);
    val[j] = j;
}

// len64: n + 1 words, the last one 0 (so that the exclusive sums end with the total)
__global__ __launch_bounds__(256) void k_as_lens(const uint64_t *__restrict__ key, uint32_t n, uint64_t *__restrict__ len64)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j > n) return;
    len64[j] = j < n ? as_key_len(key[j]) : 0;
}

// out: {n50, l50, n75, l75, n90, l90} (ex: the n + 1 running sums of the lengths, which `key` holds sorted)
__global__ void k_as_nx(const uint64_t *__restrict__ ex, const uint64_t *__restrict__ key, uint32_t n, uint64_t d, unsigned long long *__restrict__ out)
{
    const uint32_t t = threadIdx.x;
    if (t >= 3) return;
    const uint32_t x = t == 0 ? 50u : t == 1 ? 75u : 90u;
    const uint64_t l = as_lx(ex, n, x, d);
    out[2 * t] = l ? as_key_len(key[l - 1]) : 0;
    out[2 * t + 1] = l;
}

static uint32_t bits_of(uint64_t v)
{
    uint32_t b = 0;
    while (v) ++b, v >>= 1;
    return b;
}

// the two events of an MXG_DEBUG_IO timing; they go with the call however it returns
struct AsTimer {
    hipEvent_t ev[2] = {};
    ~AsTimer()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

int synteny_assess(mxg_handle *h, const mxg_assess_params &p)
{
    const mxg_handle::Synteny &S = h->syn;
    mxg_handle::Assess &A = h->assess;
    A.n_chains = A.n_bp = 0;
    A.chain.clear();
    A.bp.clear();
    std::fill(std::begin(A.sum), std::end(A.sum), 0);
    const uint64_t n64 = S.reverse.size();
    if (n64 >= 0x7FFFFFFFull) return set_err(h, MXG_ELIMIT, "mxg_synteny_assess: %llu blocks (fewer than 2^31)", (unsigned long long)n64);
    const uint32_t n = (uint32_t)n64, k = h->cfg.k, n_q = (uint32_t)S.q_len.size();
    uint64_t query_bases = 0, subject_bases = 0;
    for (uint32_t v : S.q_len) query_bases += v;
    for (uint32_t v : S.s_len) subject_bases += v;
    MXG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    DevBuf *B = h->asbuf;
    const dim3 b(256);
    auto grid = [](uint64_t m) { return dim3((uint32_t)((m + 255u) / 256u)); };
    const bool dbg = getenv("MXG_DEBUG_IO") != nullptr;
    AsTimer timer;
    hipEvent_t *ev = timer.ev;
    if (dbg && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess) (void)hipEventRecord(ev[0], st);
    MXG_HIP(h, B[AB_SUM].ensure(AS_WORDS * 8));
    MXG_HIP(h, hipMemsetAsync(B[AB_SUM].p, 0, AS_WORDS * 8, st));
    unsigned long long *d_sum = B[AB_SUM].as<unsigned long long>();
    uint64_t *d_scratch = reinterpret_cast<uint64_t *>(d_sum + AS_SCRATCH);
    // what the sorts and the Nx passes need for m elements (every array below holds at least m, len64 and the scans m + 1)
    auto ensure_sort = [&](uint32_t m) -> hipError_t {
        hipError_t e;
        for (int id : {AB_K0, AB_K1})
            if ((e = B[id].ensure((size_t)m * 8)) != hipSuccess) return e;
        for (int id : {AB_V0, AB_V1})
            if ((e = B[id].ensure((size_t)m * 4)) != hipSuccess) return e;
        for (int id : {AB_COUNTS, AB_RFIRST})
            if ((e = B[id].ensure(rs_count_words(m) * 4)) != hipSuccess) return e;
        if ((e = B[AB_RBSUM].ensure(rs_bsum_words(m) * 4)) != hipSuccess) return e;
        if ((e = B[AB_LEN64].ensure(((size_t)m + 1) * 8)) != hipSuccess) return e;
        return B[AB_TSUM].ensure((((size_t)m + 1 + PT_TILE - 1) / PT_TILE) * 8);
    };
    // the keys of AB_K0 / AB_V0 sorted by their low key_bits bits -> where they lie
    auto sort = [&](uint32_t m, uint32_t key_bits, const uint64_t *&ks, const uint32_t *&vs) {
        const int at = launch_radix_sort(st, B[AB_K0].as<uint64_t>(), B[AB_V0].as<uint32_t>(), B[AB_K1].as<uint64_t>(), B[AB_V1].as<uint32_t>(), m, key_bits,
                                         B[AB_COUNTS].as<uint32_t>(), B[AB_RFIRST].as<uint32_t>(), B[AB_RBSUM].as<uint32_t>(), d_scratch);
        ks = B[at ? AB_K1 : AB_K0].as<uint64_t>();
        vs = B[at ? AB_V1 : AB_V0].as<uint32_t>();
    };
    // lengths sorted descending in ks[0, m) -> the Nx block(s) at word `at` of the summary, one per D
    auto nx = [&](const uint64_t *ks, uint32_t m, std::initializer_list<std::pair<int, uint64_t>> blocks) {
        uint64_t *len64 = B[AB_LEN64].as<uint64_t>();
        hipLaunchKernelGGL(k_as_lens, grid((uint64_t)m + 1), b, 0, st, ks, m, len64);
        launch_scan_u64(st, len64, m + 1u, B[AB_TSUM].as<uint64_t>());
        for (const auto &blk : blocks) hipLaunchKernelGGL(k_as_nx, dim3(1), dim3(64), 0, st, len64, ks, m, blk.second, d_sum + blk.first);
    };
    uint32_t n_ch = 0;
    if (n) {
        // 1: the blocks, the table; heads and anchor counts, scanned (head: n words, acnt / ascan: n + 1)
        const bool tab = S.q_table && !S.q_pre.empty();
        MXG_HIP(h, B[AB_BLK].ensure((size_t)n * 32));
        for (int id : {AB_HEAD, AB_HSCAN, AB_ACNT, AB_ASCAN}) MXG_HIP(h, B[id].ensure(((size_t)n + 1) * 4));
        MXG_HIP(h, B[AB_BSUM].ensure((((size_t)n + 1 + TILE - 1) / TILE) * 4 + 16));
        MXG_HIP(h, hipMemcpyAsync(B[AB_BLK].p, S.block.data(), (size_t)n * 32, hipMemcpyHostToDevice, st));
        const uint32_t *d_pre = nullptr, *d_first = nullptr;
        if (tab) {
            MXG_HIP(h, B[AB_PRE].ensure(S.q_pre.size() * 4));
            MXG_HIP(h, B[AB_FIRST].ensure(S.q_first.size() * 4));
            MXG_HIP(h, hipMemcpyAsync(B[AB_PRE].p, S.q_pre.data(), S.q_pre.size() * 4, hipMemcpyHostToDevice, st));
            MXG_HIP(h, hipMemcpyAsync(B[AB_FIRST].p, S.q_first.data(), S.q_first.size() * 4, hipMemcpyHostToDevice, st));
            d_pre = B[AB_PRE].as<uint32_t>(), d_first = B[AB_FIRST].as<uint32_t>();
        }
        const uint32_t *d_blk = B[AB_BLK].as<uint32_t>();
        uint32_t *d_head = B[AB_HEAD].as<uint32_t>(), *d_hscan = B[AB_HSCAN].as<uint32_t>(), *d_ascan = B[AB_ASCAN].as<uint32_t>();
        hipLaunchKernelGGL(k_as_heads, grid((uint64_t)n + 1), b, 0, st, d_blk, n, k, p, d_pre, d_first, d_head, B[AB_ACNT].as<uint32_t>());
        launch_scan_u32(st, d_head, n, B[AB_BSUM].as<uint32_t>(), d_hscan, reinterpret_cast<uint64_t *>(d_sum + AS_HEADS));
        launch_scan_u32(st, B[AB_ACNT].as<uint32_t>(), n + 1u, B[AB_BSUM].as<uint32_t>(), d_ascan, d_scratch);
        MXG_HIP(h, hipGetLastError());
        // (every copy home lands in memory of the handle's, which outlives an early return with the copy still in flight)
        MXG_HIP(h, hipMemcpyAsync(&A.sum[AS_HEADS], d_sum + AS_HEADS, 8, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
        const uint64_t heads = A.sum[AS_HEADS];
        if (!heads || heads > n) return set_err(h, MXG_EDEVICE, "mxg_synteny_assess: internal error (%llu chains of %u blocks)", (unsigned long long)heads, n);
        n_ch = (uint32_t)heads;
        // 2: the chains (cfirst / clast: n_ch words; chain: 10 n_ch; the keys: n_ch)
        for (int id : {AB_CFIRST, AB_CLAST, AB_BPFLAG, AB_BPSCAN, AB_BPKJ}) MXG_HIP(h, B[id].ensure((size_t)n_ch * 4));
        MXG_HIP(h, B[AB_CHAIN].ensure((size_t)n_ch * 4 * AS_CHAIN_FIELDS));
        MXG_HIP(h, B[AB_BP].ensure((size_t)n_ch * 4 * AS_BP_FIELDS));
        MXG_HIP(h, B[AB_CW].ensure((size_t)n_ch * 8));
        MXG_HIP(h, B[AB_TMAX].ensure((((size_t)n_ch + PT_TILE - 1) / PT_TILE) * 8));
        MXG_HIP(h, ensure_sort(std::max(n_ch, n_q)));
        uint32_t *d_chain = B[AB_CHAIN].as<uint32_t>();
        hipLaunchKernelGGL(k_as_ends, grid(n), b, 0, st, d_head, d_hscan, n, n_ch, B[AB_CFIRST].as<uint32_t>(), B[AB_CLAST].as<uint32_t>());
        hipLaunchKernelGGL(k_as_chains, grid(n_ch), b, 0, st, d_blk, n, B[AB_CFIRST].as<uint32_t>(), B[AB_CLAST].as<uint32_t>(), d_ascan, n_ch, d_chain,
                           B[AB_K0].as<uint64_t>(), B[AB_V0].as<uint32_t>(), d_sum);
        // 3: the breakpoints
        hipLaunchKernelGGL(k_as_bp_flag, grid(n_ch), b, 0, st, d_chain, n_ch, d_blk, n, d_pre, d_first, B[AB_BPFLAG].as<uint32_t>(),
                           B[AB_BPKJ].as<uint32_t>(), d_sum);
        launch_scan_u32(st, B[AB_BPFLAG].as<uint32_t>(), n_ch, B[AB_BSUM].as<uint32_t>(), B[AB_BPSCAN].as<uint32_t>(),
                        reinterpret_cast<uint64_t *>(d_sum + AS_NBP));
        hipLaunchKernelGGL(k_as_bp_emit, grid(n_ch), b, 0, st, d_chain, n_ch, B[AB_BPFLAG].as<uint32_t>(), B[AB_BPSCAN].as<uint32_t>(),
                           B[AB_BPKJ].as<uint32_t>(), B[AB_BP].as<uint32_t>());
        MXG_HIP(h, hipGetLastError());
        // 4: the union of the subject intervals, chains in subject order
        const uint64_t *ks;
        const uint32_t *vs;
        sort(n_ch, 32u + bits_of(S.s_len.size()), ks, vs);
        const uint32_t max_tiles = (n_ch + PT_TILE - 1) / PT_TILE;
        uint64_t *d_cw = B[AB_CW].as<uint64_t>(), *d_tmax = B[AB_TMAX].as<uint64_t>();
        hipLaunchKernelGGL(k_as_cover_words, grid(n_ch), b, 0, st, ks, vs, d_chain + (size_t)8 * n_ch, n_ch, d_cw);
        hipLaunchKernelGGL(k_pt_max_tile, dim3(max_tiles), b, 0, st, d_cw, n_ch, d_tmax);
        hipLaunchKernelGGL(k_pt_max_tiles, dim3(1), b, 0, st, d_tmax, max_tiles);
        hipLaunchKernelGGL(k_as_cover, dim3(max_tiles), b, 0, st, ks, d_cw, n_ch, d_tmax, d_sum);
        MXG_HIP(h, hipGetLastError());
        // 5: na, nga over the chains' query spans
        hipLaunchKernelGGL(k_as_span_keys, grid(n_ch), b, 0, st, d_chain + (size_t)4 * n_ch, d_chain + (size_t)5 * n_ch, n_ch, B[AB_K0].as<uint64_t>(),
                           B[AB_V0].as<uint32_t>());
        sort(n_ch, 32u, ks, vs);
        nx(ks, n_ch, {{AS_NA, query_bases}, {AS_NGA, subject_bases}});
        MXG_HIP(h, hipGetLastError());
    }
    // 6: ng over the query's record lengths
    if (n_q) {
        if (!n) MXG_HIP(h, ensure_sort(n_q));
        MXG_HIP(h, B[AB_QLEN].ensure((size_t)n_q * 4));
        MXG_HIP(h, hipMemcpyAsync(B[AB_QLEN].p, S.q_len.data(), (size_t)n_q * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_as_len_keys, grid(n_q), b, 0, st, B[AB_QLEN].as<uint32_t>(), n_q, B[AB_K0].as<uint64_t>(), B[AB_V0].as<uint32_t>());
        const uint64_t *ks;
        const uint32_t *vs;
        sort(n_q, 32u, ks, vs);
        nx(ks, n_q, {{AS_NG, subject_bases}});
        MXG_HIP(h, hipGetLastError());
    }
    // 7: home
    std::vector<uint32_t> &bp_all = A.bp_all;
    bp_all.resize((size_t)n_ch * AS_BP_FIELDS);
    A.chain.resize((size_t)n_ch * AS_CHAIN_FIELDS);
    if (n_ch) {
        MXG_HIP(h, hipMemcpyAsync(A.chain.data(), B[AB_CHAIN].p, A.chain.size() * 4, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipMemcpyAsync(bp_all.data(), B[AB_BP].p, bp_all.size() * 4, hipMemcpyDeviceToHost, st));
    }
    MXG_HIP(h, hipMemcpyAsync(A.sum, d_sum, AS_WORDS * 8, hipMemcpyDeviceToHost, st));
    if (dbg && ev[1]) (void)hipEventRecord(ev[1], st);
    MXG_HIP(h, hipStreamSynchronize(st));
    uint64_t counted = 0;
    for (int u = 0; u < 6; ++u) counted += A.sum[AS_BP0 + u];
    if (A.sum[AS_NBP] != counted || counted >= std::max<uint64_t>(n_ch, 1))
        return set_err(h, MXG_EDEVICE, "mxg_synteny_assess: internal error (%llu breakpoints placed, %llu counted, %u chains)",
                       (unsigned long long)A.sum[AS_NBP], (unsigned long long)counted, n_ch);
    A.n_chains = n_ch;
    A.n_bp = counted;
    A.bp.resize((size_t)counted * AS_BP_FIELDS);
    for (uint32_t u = 0; u < AS_BP_FIELDS; ++u) std::copy_n(bp_all.begin() + (size_t)u * n_ch, counted, A.bp.begin() + (size_t)u * counted);
    A.query_bases = query_bases;
    A.subject_bases = subject_bases;
    if (dbg) {
        float ms = 0;
        if (ev[0] && ev[1]) (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        fprintf(stderr, "[mxg] synteny_assess blocks=%u chains=%u breakpoints=%llu query_records=%u ms=%.3f\n", n, n_ch, (unsigned long long)counted, n_q, ms);
    }
    return MXG_OK;
}

}  // namespace mxg
