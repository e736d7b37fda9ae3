// compose.hip -- mxg_compose_pieces: the piece tables of two scaffolding rounds composed into one (include/ntjoin_mx.h, row f11;
// the rule itself is compose.h).  The host checks both tables and makes the inner table's prefix while it converts the offsets
// (cmp_table: one pass over arrays it has to read for the upload anyway); everything per piece runs on the device:
//   k_cmp_count    per outer piece: how many pieces it becomes (two bisections over its inner record's prefix); per block their
//                  64-bit sum, so the host knows the size of the result before anything is scanned in 32 bits
//   scan           exclusive, over the counts (scan_kernels.h)
//   k_cmp_emit     one thread per expanded piece: its outer piece by bisection over the scanned counts, the inner piece clipped
//   k_cmp_flag     an expanded piece survives unless it is a GAP behind a GAP of the same outer record
//   scan           over the flags
//   k_cmp_compact  a surviving piece moves to its place; a GAP takes the lengths of the GAPs behind it that do not survive
//   k_cmp_first    where every outer record starts in the result
// Plain loads and stores throughout; every write is at an index below the size its array was allocated for (see the launches).
#include "compose.h"
#include "mxg_internal.h"
#include "scan_kernels.h"

namespace mxg {

enum { CMP_OUTER, CMP_OREC, CMP_OFIRST, CMP_INNER, CMP_IFIRST, CMP_IPRE, CMP_CNT, CMP_ESCAN, CMP_BSUM, CMP_BSUM64, CMP_EXP, CMP_EREC,
       CMP_FLAG, CMP_FSCAN, CMP_RES, CMP_RFIRST, CMP_BUF_COUNT };
static_assert(CMP_BUF_COUNT <= 16, "mxg_handle::cmpbuf too small");

// the inner pieces an outer FWD / REV piece becomes: [j_lo, j_hi] relative to its inner record's first piece f
__device__ __forceinline__ void cmp_dev_range(const mxg_seq_piece &p, const uint32_t *__restrict__ ifirst, const uint32_t *__restrict__ ipre,
                                              uint32_t &f, uint32_t &j_lo, uint32_t &j_hi)
{
    f = ifirst[p.record];
    cmp_range(ipre + f, ifirst[p.record + 1] - f, p.start, p.end, j_lo, j_hi);
}

__global__ __launch_bounds__(256) void k_cmp_count(const mxg_seq_piece *__restrict__ op, uint32_t n_op, const uint32_t *__restrict__ ifirst,
                                                   const uint32_t *__restrict__ ipre, uint32_t *__restrict__ cnt, uint64_t *__restrict__ bsum64)
{
    __shared__ uint64_t sh[256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t c = 0;
    if (i < n_op) {
        const mxg_seq_piece p = op[i];
        c = 1;
        if (p.kind != MXG_PIECE_GAP) {
            uint32_t f, j_lo, j_hi;
            cmp_dev_range(p, ifirst, ipre, f, j_lo, j_hi);
            c = j_hi - j_lo + 1u;
        }
        cnt[i] = c;
    }
    sh[threadIdx.x] = c;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum64[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(256) void k_cmp_emit(const mxg_seq_piece *__restrict__ op, const uint32_t *__restrict__ orec, uint32_t n_op,
                                                  const mxg_seq_piece *__restrict__ ip, const uint32_t *__restrict__ ifirst,
                                                  const uint32_t *__restrict__ ipre, const uint32_t *__restrict__ escan, uint32_t n_exp,
                                                  mxg_seq_piece *__restrict__ exp, uint32_t *__restrict__ erec)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_exp) return;
    // the outer piece that expanded piece g comes from: the largest i < n_op with escan[i] <= g (escan[0] = 0, escan strictly
    // increasing: every outer piece becomes at least one piece)
    const uint32_t i = last_le(escan, 0u, n_op, g);
    const mxg_seq_piece p = op[i];
    mxg_seq_piece o;
    if (p.kind == MXG_PIECE_GAP) {
        o.record = 0;
        o.start = 0;
        o.end = cmp_len(p);
        o.kind = MXG_PIECE_GAP;
    } else {
        uint32_t f, j_lo, j_hi;
        cmp_dev_range(p, ifirst, ipre, f, j_lo, j_hi);
        o = cmp_expand(p, ip + f, ipre + f, j_lo, j_hi, g - escan[i]);
    }
    exp[g] = o;
    erec[g] = orec[i];
}

__global__ __launch_bounds__(256) void k_cmp_flag(const mxg_seq_piece *__restrict__ exp, const uint32_t *__restrict__ erec, uint32_t n_exp,
                                                  uint32_t *__restrict__ flag)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_exp) return;
    const bool joins = g > 0 && exp[g].kind == MXG_PIECE_GAP && exp[g - 1].kind == MXG_PIECE_GAP && erec[g] == erec[g - 1];
    flag[g] = joins ? 0u : 1u;
}

__global__ __launch_bounds__(256) void k_cmp_compact(const mxg_seq_piece *__restrict__ exp, const uint32_t *__restrict__ flag,
                                                     const uint32_t *__restrict__ fscan, uint32_t n_exp, mxg_seq_piece *__restrict__ res)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_exp || !flag[g]) return;
    mxg_seq_piece o = exp[g];
    if (o.kind == MXG_PIECE_GAP)
        for (uint32_t t = g + 1; t < n_exp && !flag[t]; ++t) o.end += cmp_len(exp[t]);  // (a record's length fits 32 bits: cmp_table)
    res[fscan[g]] = o;  // fscan[g] < the number of set flags = the pieces res was allocated for
}

// a record's first expanded piece always survives: its place in the result is the record's start
__global__ __launch_bounds__(256) void k_cmp_first(const uint32_t *__restrict__ ofirst, uint32_t n_outer, const uint32_t *__restrict__ escan,
                                                   const uint32_t *__restrict__ fscan, const uint64_t *__restrict__ n_res,
                                                   uint64_t *__restrict__ rfirst)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r > n_outer) return;
    rfirst[r] = r == n_outer ? *n_res : (uint64_t)fscan[escan[ofirst[r]]];
}

int compose_pieces(mxg_handle *h, const mxg_seq_piece *outer, const uint64_t *outer_first, uint64_t n_outer, const mxg_seq_piece *inner,
                   const uint64_t *inner_first, uint64_t n_inner)
{
    h->cmp_pieces.clear();
    h->cmp_first.assign(1, 0);
    CmpTable ti, to;
    std::string msg;
    int rc = cmp_table("inner", inner, inner_first, n_inner, ~0ull, nullptr, ti, msg);
    if (rc == MXG_OK) rc = cmp_table("outer", outer, outer_first, n_outer, n_inner, ti.len.data(), to, msg);
    if (rc != MXG_OK) return set_err(h, rc, "mxg_compose_pieces: %s", msg.c_str());
    if (n_outer == 0) return MXG_OK;
    const uint32_t n_op = to.first[n_outer], n_ip = ti.first[n_inner], n_or = (uint32_t)n_outer, n_ir = (uint32_t)n_inner;
    MXG_HIP(h, hipSetDevice(h->device));
    DevBuf *B = h->cmpbuf;
    const dim3 b(256);
    const uint32_t blocks_op = (n_op + 255u) / 256u;
    MXG_HIP(h, B[CMP_OUTER].ensure((size_t)n_op * sizeof(mxg_seq_piece)));
    MXG_HIP(h, B[CMP_OREC].ensure((size_t)n_op * 4));
    MXG_HIP(h, B[CMP_OFIRST].ensure(((size_t)n_or + 1) * 4));
    MXG_HIP(h, B[CMP_INNER].ensure((size_t)n_ip * sizeof(mxg_seq_piece)));
    MXG_HIP(h, B[CMP_IFIRST].ensure(((size_t)n_ir + 1) * 4));
    MXG_HIP(h, B[CMP_IPRE].ensure((size_t)n_ip * 4));
    MXG_HIP(h, B[CMP_CNT].ensure((size_t)n_op * 4));
    MXG_HIP(h, B[CMP_ESCAN].ensure((size_t)n_op * 4));
    MXG_HIP(h, B[CMP_BSUM64].ensure((size_t)blocks_op * 8));
    MXG_HIP(h, B[CMP_RFIRST].ensure(((size_t)n_or + 1) * 8 + 16));  // [0]: the scans' totals; [2 ..]: the result's `first`
    MXG_HIP(h, hipMemcpyAsync(B[CMP_OUTER].p, outer, (size_t)n_op * sizeof(mxg_seq_piece), hipMemcpyHostToDevice, h->stream));
    MXG_HIP(h, hipMemcpyAsync(B[CMP_OREC].p, to.rec.data(), (size_t)n_op * 4, hipMemcpyHostToDevice, h->stream));
    MXG_HIP(h, hipMemcpyAsync(B[CMP_OFIRST].p, to.first.data(), ((size_t)n_or + 1) * 4, hipMemcpyHostToDevice, h->stream));
    MXG_HIP(h, hipMemcpyAsync(B[CMP_INNER].p, inner, (size_t)n_ip * sizeof(mxg_seq_piece), hipMemcpyHostToDevice, h->stream));
    MXG_HIP(h, hipMemcpyAsync(B[CMP_IFIRST].p, ti.first.data(), ((size_t)n_ir + 1) * 4, hipMemcpyHostToDevice, h->stream));
    MXG_HIP(h, hipMemcpyAsync(B[CMP_IPRE].p, ti.pre.data(), (size_t)n_ip * 4, hipMemcpyHostToDevice, h->stream));
    const mxg_seq_piece *d_op = B[CMP_OUTER].as<mxg_seq_piece>(), *d_ip = B[CMP_INNER].as<mxg_seq_piece>();
    const uint32_t *d_orec = B[CMP_OREC].as<uint32_t>(), *d_ofirst = B[CMP_OFIRST].as<uint32_t>();
    const uint32_t *d_ifirst = B[CMP_IFIRST].as<uint32_t>(), *d_ipre = B[CMP_IPRE].as<uint32_t>();
    uint32_t *d_cnt = B[CMP_CNT].as<uint32_t>(), *d_escan = B[CMP_ESCAN].as<uint32_t>();
    uint64_t *d_tot = B[CMP_RFIRST].as<uint64_t>(), *d_rfirst = d_tot + 2;
    // 1: count.  The result's size as a 64-bit sum, before the 32-bit scan
    hipLaunchKernelGGL(k_cmp_count, dim3(blocks_op), b, 0, h->stream, d_op, n_op, d_ifirst, d_ipre, d_cnt, B[CMP_BSUM64].as<uint64_t>());
    MXG_HIP(h, hipGetLastError());
    std::vector<uint64_t> bsum(blocks_op);
    MXG_HIP(h, hipMemcpyAsync(bsum.data(), B[CMP_BSUM64].p, (size_t)blocks_op * 8, hipMemcpyDeviceToHost, h->stream));
    MXG_HIP(h, hipStreamSynchronize(h->stream));
    uint64_t n_exp64 = 0;
    for (uint64_t v : bsum) n_exp64 += v;
    if (n_exp64 >= CMP_MAX_PIECES)
        return set_err(h, MXG_ELIMIT, "mxg_compose_pieces: the result has %llu pieces (at most 2^31 - 2)", (unsigned long long)n_exp64);
    const uint32_t n_exp = (uint32_t)n_exp64, blocks_exp = (n_exp + 255u) / 256u;  // n_exp >= n_op >= 1
    MXG_HIP(h, B[CMP_BSUM].ensure(((size_t)(n_exp + TILE - 1) / TILE) * 4 + 16));
    MXG_HIP(h, B[CMP_EXP].ensure((size_t)n_exp * sizeof(mxg_seq_piece)));
    MXG_HIP(h, B[CMP_EREC].ensure((size_t)n_exp * 4));
    MXG_HIP(h, B[CMP_FLAG].ensure((size_t)n_exp * 4));
    MXG_HIP(h, B[CMP_FSCAN].ensure((size_t)n_exp * 4));
    mxg_seq_piece *d_exp = B[CMP_EXP].as<mxg_seq_piece>();
    uint32_t *d_erec = B[CMP_EREC].as<uint32_t>(), *d_flag = B[CMP_FLAG].as<uint32_t>(), *d_fscan = B[CMP_FSCAN].as<uint32_t>();
    // 2, 3: scan, emit (every thread g < n_exp writes exp[g], erec[g])
    launch_scan_u32(h->stream, d_cnt, n_op, B[CMP_BSUM].as<uint32_t>(), d_escan, d_tot);
    hipLaunchKernelGGL(k_cmp_emit, dim3(blocks_exp), b, 0, h->stream, d_op, d_orec, n_op, d_ip, d_ifirst, d_ipre, d_escan, n_exp, d_exp, d_erec);
    // 4, 5: flag, scan
    hipLaunchKernelGGL(k_cmp_flag, dim3(blocks_exp), b, 0, h->stream, d_exp, d_erec, n_exp, d_flag);
    launch_scan_u32(h->stream, d_flag, n_exp, B[CMP_BSUM].as<uint32_t>(), d_fscan, d_tot + 1);
    MXG_HIP(h, hipGetLastError());
    uint64_t tot[2] = {0, 0};
    MXG_HIP(h, hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, h->stream));
    MXG_HIP(h, hipStreamSynchronize(h->stream));
    if (tot[0] != n_exp64 || tot[1] == 0 || tot[1] > n_exp64)
        return set_err(h, MXG_EDEVICE, "mxg_compose_pieces: the scans give %llu and %llu pieces, the count gave %llu", (unsigned long long)tot[0],
                       (unsigned long long)tot[1], (unsigned long long)n_exp64);
    // 6: compact into tot[1] pieces
    const uint64_t n_res = tot[1];
    MXG_HIP(h, B[CMP_RES].ensure((size_t)n_res * sizeof(mxg_seq_piece)));
    hipLaunchKernelGGL(k_cmp_compact, dim3(blocks_exp), b, 0, h->stream, d_exp, d_flag, d_fscan, n_exp, B[CMP_RES].as<mxg_seq_piece>());
    hipLaunchKernelGGL(k_cmp_first, dim3((n_or + 256u) / 256u), b, 0, h->stream, d_ofirst, n_or, d_escan, d_fscan, d_tot + 1, d_rfirst);
    MXG_HIP(h, hipGetLastError());
    h->cmp_pieces.resize(n_res);
    h->cmp_first.resize((size_t)n_or + 1);
    MXG_HIP(h, hipMemcpyAsync(h->cmp_pieces.data(), B[CMP_RES].p, (size_t)n_res * sizeof(mxg_seq_piece), hipMemcpyDeviceToHost, h->stream));
    MXG_HIP(h, hipMemcpyAsync(h->cmp_first.data(), d_rfirst, ((size_t)n_or + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    MXG_HIP(h, hipStreamSynchronize(h->stream));
    return MXG_OK;
}

}  // namespace mxg
