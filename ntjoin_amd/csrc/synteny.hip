// synteny.hip -- mxg_synteny_blocks and mxg_write_synteny_paf: the maximal collinear runs of graph vertices between a query and a
// subject assembly, and their PAF text (include/ntjoin_mx.h, row f12; the rules themselves are synteny.h).
// The host checks the arguments and the piece table (compose.h's cmp_table); everything per anchor, piece or block runs on the device:
//   k_syn_gather   per vertex, in the query's (record, position) order: the 16-byte anchor.  That order is row q of the graph
//                  stage's filtered lists (g_fv / g_frec: vertex and record of every shared minimizer of an assembly, in sketch
//                  order), so the query's sketch is not compacted a second time
//   k_syn_count    (piece table) per piece: the anchors it takes -- two lower bounds on (record, position) -- and per block their
//                  64-bit sum, so the host knows the list's size before anything is scanned in 32 bits
//   scan, k_syn_emit   one thread per anchor of the new list: its piece by bisection over the scanned counts, REV pieces backwards
//   k_syn_heads    per link: is it the head of a block; the number of links
//   scan           over the head flags.  Heads and tails alternate, so ONE scan places both: the block of a tail at link i is the
//                  number of heads at links <= i, less one
//   k_syn_ends     per link: a head stores its first anchor, a tail its last, at the block's index
//   k_syn_blocks   per block: its fields from the two anchors, and whether it is kept
//   scan, k_syn_compact   the kept blocks, in order, as eight arrays
// The PAF writer is pathtext.hip's shape: one formatter over the two sinks of text_dev.h, a 64-bit scan of the lines' lengths,
// per window the first block by bisection (k_win_bounds), then write_windows (both win_out.hip); MXG_SYN_WIN sets the bytes per window.
// Plain loads and stores throughout; every write is at an index below the size its array was allocated for (see the launches).
#include <algorithm>
#include <string>

#include "compose.h"
#include "mxg_internal.h"
#include "scan64_kernels.h"
#include "scan_kernels.h"
#include "synteny.h"
#include "text_dev.h"

namespace mxg {

enum { SY_A0, SY_A1, SY_PIECES, SY_PREC, SY_POFF, SY_PLO, SY_CNT, SY_ESCAN, SY_BSUM, SY_BSUM64, SY_HEAD, SY_HSCAN, SY_FIRST, SY_LAST, SY_BLK,
       SY_KEEP, SY_KSCAN, SY_OUT, SY_TOT, SY_QLEN, SY_SLEN, SY_IDOFF, SY_IDS, SY_LOFF, SY_TSUM, SY_BOUNDS, SY_IDY, SY_BUF_COUNT };
static_assert(SY_BUF_COUNT <= 32, "mxg_handle::synbuf too small");
enum { ST_EXP, ST_HEADS, ST_KEPT, ST_LINKS, ST_BAD, ST_WORDS };  // the words of SY_TOT
constexpr uint64_t SYN_MAX = 0x7FFFFFFFull;                         // 2^31 anchors or blocks or more: MXG_ELIMIT

__global__ __launch_bounds__(256) void k_syn_gather(const uint32_t *__restrict__ fv_q, const uint32_t *__restrict__ frec_q,
                                                    const uint32_t *__restrict__ vpos_q, const uint32_t *__restrict__ vrec_s,
                                                    const uint32_t *__restrict__ vpos_s, uint32_t n, SynAnchor *__restrict__ out,
                                                    unsigned long long *__restrict__ tot)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t v = fv_q[i];
    if (v >= n) {  // (no vertex of the graph stage is: reported, not followed)
        atomicAdd(tot + ST_BAD, 1ull);
        v = 0;
    }
    SynAnchor a;
    a.qrec = frec_q[i];
    a.qpos = vpos_q[v];
    a.srec = vrec_s[v];
    a.spos = vpos_s[v];
    out[i] = a;
}

__global__ __launch_bounds__(256) void k_syn_count(const mxg_seq_piece *__restrict__ pc, uint32_t n_pc, const SynAnchor *__restrict__ a, uint32_t n,
                                                   uint32_t k, uint32_t *__restrict__ cnt, uint32_t *__restrict__ plo, uint64_t *__restrict__ bsum64)
{
    __shared__ uint64_t sh[256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t c = 0;
    if (i < n_pc) {
        uint64_t lo, hi;
        syn_piece_range(a, n, pc[i], k, lo, hi);
        c = (uint32_t)(hi - lo);  // (hi - lo <= n < 2^31)
        cnt[i] = c;
        plo[i] = (uint32_t)lo;
    }
    sh[threadIdx.x] = c;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum64[blockIdx.x] = sh[0];
}

// one thread per anchor of the new list; its piece is the largest i with escan[i] <= g (pieces without anchors share their
// successor's offset and are passed over)
__global__ __launch_bounds__(256) void k_syn_emit(const mxg_seq_piece *__restrict__ pc, const uint32_t *__restrict__ prec,
                                                  const uint32_t *__restrict__ poff, const uint32_t *__restrict__ plo,
                                                  const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ escan, uint32_t n_pc,
                                                  const SynAnchor *__restrict__ in, uint32_t n_exp, uint32_t k, SynAnchor *__restrict__ out)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_exp) return;
    const uint32_t i = last_le(escan, 0u, n_pc, g), t = g - escan[i];
    if (t >= cnt[i]) return;  // (cannot be: g lies below the scan's total)
    out[g] = syn_piece_anchor(in, pc[i], k, plo[i], (uint64_t)plo[i] + cnt[i], t, prec[i], poff[i]);
}

__global__ __launch_bounds__(256) void k_syn_heads(const SynAnchor *__restrict__ a, uint32_t n, uint32_t max_gap, uint32_t *__restrict__ head,
                                                   unsigned long long *__restrict__ tot)
{
    __shared__ uint32_t sh[256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t c = SYN_NONE;
    if (i < n) {
        c = syn_link_at(a, n, (int64_t)i, max_gap);
        head[i] = syn_is_head(syn_link_at(a, n, (int64_t)i - 1, max_gap), c) ? 1u : 0u;
    }
    sh[threadIdx.x] = c != SYN_NONE ? 1u : 0u;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0]) atomicAdd(tot + ST_LINKS, (unsigned long long)sh[0]);
}

__global__ __launch_bounds__(256) void k_syn_ends(const SynAnchor *__restrict__ a, uint32_t n, uint32_t max_gap, const uint32_t *__restrict__ head,
                                                  const uint32_t *__restrict__ hscan, uint32_t n_blk, uint32_t *__restrict__ first,
                                                  uint32_t *__restrict__ last)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = syn_link_at(a, n, (int64_t)i, max_gap);
    if (c == SYN_NONE) return;
    const uint32_t hd = head[i], b = hscan[i];
    if (hd && b < n_blk) first[b] = i;
    if (syn_is_tail(c, syn_link_at(a, n, (int64_t)i + 1, max_gap))) {
        const uint32_t tb = b + hd - 1u;  // (a link with a code has a head at or before it: b + hd >= 1)
        if (tb < n_blk) last[tb] = i + 1u;
    }
}

__global__ __launch_bounds__(256) void k_syn_blocks(const SynAnchor *__restrict__ a, const uint32_t *__restrict__ first,
                                                    const uint32_t *__restrict__ last, uint32_t n, uint32_t n_blk, uint32_t k,
                                                    uint32_t min_anchors, uint32_t min_span, SynBlock *__restrict__ blk, uint32_t *__restrict__ keep)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_blk) return;
    const uint32_t j = first[b], l = last[b];
    if (j >= l || l >= n) {  // (cannot be: every block has one head and, behind it, one tail)
        keep[b] = 0;
        return;
    }
    const SynBlock o = syn_block(a[j], a[l], j, (uint64_t)l - 1u, k);
    blk[b] = o;
    keep[b] = syn_keep(o, min_anchors, min_span) ? 1u : 0u;
}

// out: eight arrays of n_keep words, one behind the other, in the order of SynBlock's fields
__global__ __launch_bounds__(256) void k_syn_compact(const SynBlock *__restrict__ blk, const uint32_t *__restrict__ keep,
                                                     const uint32_t *__restrict__ kscan, uint32_t n_blk, uint32_t n_keep, uint32_t *__restrict__ out)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_blk || !keep[b]) return;
    const uint32_t at = kscan[b];
    if (at >= n_keep) return;  // (cannot be: kscan counts the kept blocks before b)
    const SynBlock o = blk[b];
    const uint32_t f[8] = {o.n_anchors, o.q_record, o.q_start, o.q_end, o.s_record, o.s_start, o.s_end, o.reverse};
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) out[(size_t)u * n_keep + at] = f[u];
}

// the handle's lengths of an assembly's records as 32-bit words, or why not
static int syn_lengths(mxg_handle *h, const Assembly *a, int assembly, const uint32_t *given, const char *what, std::vector<uint32_t> &out)
{
    const size_t n = a->recs.size();
    if (given) {
        out.assign(given, given + n);
        return MXG_OK;
    }
    out.resize(n);
    bool any = false;
    for (size_t r = 0; r < n; ++r) {
        if (a->recs[r].len > 0xFFFFFFFFull)
            return set_err(h, MXG_ELIMIT, "mxg_synteny_blocks: record %s of the %s is longer than 2^32 - 1 bases", a->recs[r].id.c_str(), what);
        any = any || a->recs[r].len != 0;
        out[r] = (uint32_t)a->recs[r].len;
    }
    if (!any && n)
        return set_err(h, MXG_EINVAL, "mxg_synteny_blocks: assembly %d holds no record lengths (minimizer input); pass %s_length", assembly, what);
    return MXG_OK;
}

int synteny_blocks(mxg_handle *h, int q, int s, const mxg_synteny_params &p, const mxg_seq_piece *pieces, const uint64_t *first, uint64_t n_records,
                   const uint32_t *query_length, const uint32_t *subject_length)
{
    mxg_handle::Synteny &S = h->syn;
    S.valid = false;
    h->idy.valid = false;  // (mxg_synteny_identity is about the blocks of the call before it)
    S.d_anchor = nullptr, S.n_dev_blocks = 0;
    const Graph &g = h->graph;
    const Assembly *aq = h->asms[q], *as = h->asms[s];
    int rc;
    std::vector<uint32_t> qlen_in;
    if ((rc = syn_lengths(h, aq, q, query_length, "query", qlen_in)) != MXG_OK) return rc;
    if ((rc = syn_lengths(h, as, s, subject_length, "subject", S.s_len)) != MXG_OK) return rc;
    CmpTable tab;
    if (pieces) {
        std::string msg;
        rc = cmp_table("query", pieces, first, n_records, qlen_in.size(), qlen_in.data(), tab, msg);
        if (rc != MXG_OK) return set_err(h, rc, "mxg_synteny_blocks: %s", msg.c_str());
        S.q_len = tab.len;
        S.q_pre = tab.pre, S.q_first = tab.first;  // (what mxg_synteny_assess asks of the table: the piece of a base)
    } else {
        S.q_len = qlen_in;
        S.q_pre.clear(), S.q_first.clear();
    }
    S.q = q, S.s = s, S.q_table = pieces != nullptr;
    S.n_anchors = S.n_links = 0;
    S.block.clear();
    S.reverse.clear();
    if (g.nv >= SYN_MAX) return set_err(h, MXG_ELIMIT, "mxg_synteny_blocks: %llu anchors (fewer than 2^31)", (unsigned long long)g.nv);
    const uint32_t nv = (uint32_t)g.nv, k = h->cfg.k;
    if (!nv || (pieces && !tab.pre.size())) {
        S.valid = true;
        return MXG_OK;
    }
    MXG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    DevBuf *B = h->synbuf;
    const dim3 b(256);
    auto grid = [](uint64_t n) { return dim3((uint32_t)((n + 255u) / 256u)); };
    const bool dbg = getenv("MXG_DEBUG_IO") != nullptr;
    hipEvent_t ev[2] = {};
    if (dbg && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess) (void)hipEventRecord(ev[0], st);
    MXG_HIP(h, B[SY_TOT].ensure(ST_WORDS * 8));
    MXG_HIP(h, hipMemsetAsync(B[SY_TOT].p, 0, ST_WORDS * 8, st));
    unsigned long long *d_tot = B[SY_TOT].as<unsigned long long>();
    // 1: the anchors in the query's order (every thread i < nv writes a0[i])
    MXG_HIP(h, B[SY_A0].ensure((size_t)nv * sizeof(SynAnchor)));
    SynAnchor *a0 = B[SY_A0].as<SynAnchor>();
    {
        const size_t rq = (size_t)q * g.nv_stride, rs = (size_t)s * g.nv_stride;
        const uint32_t *fv = h->g_fv.as<uint32_t>(), *frec = h->g_frec.as<uint32_t>(), *vpos = h->g_vpos.as<uint32_t>(), *vrec = h->g_vrec.as<uint32_t>();
        hipLaunchKernelGGL(k_syn_gather, grid(nv), b, 0, st, fv + rq, frec + rq, vpos + rq, vrec + rs, vpos + rs, nv, a0, d_tot);
        MXG_HIP(h, hipGetLastError());
    }
    const SynAnchor *d_a = a0;
    uint32_t n = nv;
    // 2: through the piece table
    if (pieces) {
        const uint32_t n_pc = (uint32_t)tab.pre.size(), blocks_pc = (n_pc + 255u) / 256u;
        MXG_HIP(h, B[SY_PIECES].ensure((size_t)n_pc * sizeof(mxg_seq_piece)));
        for (int id : {SY_PREC, SY_POFF, SY_PLO, SY_CNT, SY_ESCAN}) MXG_HIP(h, B[id].ensure((size_t)n_pc * 4));
        MXG_HIP(h, B[SY_BSUM64].ensure((size_t)blocks_pc * 8));
        MXG_HIP(h, hipMemcpyAsync(B[SY_PIECES].p, pieces, (size_t)n_pc * sizeof(mxg_seq_piece), hipMemcpyHostToDevice, st));
        MXG_HIP(h, hipMemcpyAsync(B[SY_PREC].p, tab.rec.data(), (size_t)n_pc * 4, hipMemcpyHostToDevice, st));
        MXG_HIP(h, hipMemcpyAsync(B[SY_POFF].p, tab.pre.data(), (size_t)n_pc * 4, hipMemcpyHostToDevice, st));
        const mxg_seq_piece *d_pc = B[SY_PIECES].as<mxg_seq_piece>();
        uint32_t *d_cnt = B[SY_CNT].as<uint32_t>(), *d_plo = B[SY_PLO].as<uint32_t>(), *d_escan = B[SY_ESCAN].as<uint32_t>();
        hipLaunchKernelGGL(k_syn_count, dim3(blocks_pc), b, 0, st, d_pc, n_pc, a0, nv, k, d_cnt, d_plo, B[SY_BSUM64].as<uint64_t>());
        MXG_HIP(h, hipGetLastError());
        std::vector<uint64_t> bsum(blocks_pc);
        MXG_HIP(h, hipMemcpyAsync(bsum.data(), B[SY_BSUM64].p, (size_t)blocks_pc * 8, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
        uint64_t n_exp64 = 0;
        for (uint64_t v : bsum) n_exp64 += v;
        if (n_exp64 >= SYN_MAX)
            return set_err(h, MXG_ELIMIT, "mxg_synteny_blocks: %llu anchors behind the piece table (fewer than 2^31)", (unsigned long long)n_exp64);
        n = (uint32_t)n_exp64;
        if (n) {
            MXG_HIP(h, B[SY_BSUM].ensure(((size_t)(n_pc + TILE - 1) / TILE) * 4 + 16));
            MXG_HIP(h, B[SY_A1].ensure((size_t)n * sizeof(SynAnchor)));
            launch_scan_u32(st, d_cnt, n_pc, B[SY_BSUM].as<uint32_t>(), d_escan, reinterpret_cast<uint64_t *>(d_tot + ST_EXP));
            // (every thread g < n writes a1[g])
            hipLaunchKernelGGL(k_syn_emit, grid(n), b, 0, st, d_pc, B[SY_PREC].as<uint32_t>(), B[SY_POFF].as<uint32_t>(), d_plo, d_cnt, d_escan, n_pc, a0,
                               n, k, B[SY_A1].as<SynAnchor>());
            MXG_HIP(h, hipGetLastError());
            d_a = B[SY_A1].as<SynAnchor>();
        }
    }
    S.n_anchors = n;
    uint64_t tot[ST_WORDS] = {};
    uint32_t n_blk = 0, n_keep = 0;
    if (n) {
        // 3: heads, scanned (every thread i < n writes head[i])
        MXG_HIP(h, B[SY_HEAD].ensure((size_t)n * 4));
        MXG_HIP(h, B[SY_HSCAN].ensure((size_t)n * 4));
        MXG_HIP(h, B[SY_BSUM].ensure(((size_t)(n + TILE - 1) / TILE) * 4 + 16));
        uint32_t *d_head = B[SY_HEAD].as<uint32_t>(), *d_hscan = B[SY_HSCAN].as<uint32_t>();
        hipLaunchKernelGGL(k_syn_heads, grid(n), b, 0, st, d_a, n, p.max_gap, d_head, d_tot);
        launch_scan_u32(st, d_head, n, B[SY_BSUM].as<uint32_t>(), d_hscan, reinterpret_cast<uint64_t *>(d_tot + ST_HEADS));
        MXG_HIP(h, hipGetLastError());
        MXG_HIP(h, hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
        if (tot[ST_BAD] || (pieces && tot[ST_EXP] != n) || tot[ST_HEADS] > tot[ST_LINKS] || tot[ST_LINKS] >= n)
            return set_err(h, MXG_EDEVICE, "mxg_synteny_blocks: internal error (%llu vertices out of range, %llu of %u anchors emitted, %llu heads of %llu links)",
                           (unsigned long long)tot[ST_BAD], (unsigned long long)tot[ST_EXP], n, (unsigned long long)tot[ST_HEADS],
                           (unsigned long long)tot[ST_LINKS]);
        n_blk = (uint32_t)tot[ST_HEADS];  // (< n < 2^31)
        S.n_links = tot[ST_LINKS];
    }
    if (n_blk) {
        // 4: the blocks' ends (first and last hold n_blk words; every block has one head and one tail), their fields, the kept ones
        for (int id : {SY_FIRST, SY_LAST, SY_KEEP, SY_KSCAN}) MXG_HIP(h, B[id].ensure((size_t)n_blk * 4));
        MXG_HIP(h, B[SY_BLK].ensure((size_t)n_blk * sizeof(SynBlock)));
        uint32_t *d_first = B[SY_FIRST].as<uint32_t>(), *d_last = B[SY_LAST].as<uint32_t>(), *d_keep = B[SY_KEEP].as<uint32_t>();
        hipLaunchKernelGGL(k_syn_ends, grid(n), b, 0, st, d_a, n, p.max_gap, B[SY_HEAD].as<uint32_t>(), B[SY_HSCAN].as<uint32_t>(), n_blk, d_first, d_last);
        hipLaunchKernelGGL(k_syn_blocks, grid(n_blk), b, 0, st, d_a, d_first, d_last, n, n_blk, k, p.min_anchors, p.min_span, B[SY_BLK].as<SynBlock>(), d_keep);
        launch_scan_u32(st, d_keep, n_blk, B[SY_BSUM].as<uint32_t>(), B[SY_KSCAN].as<uint32_t>(), reinterpret_cast<uint64_t *>(d_tot + ST_KEPT));
        MXG_HIP(h, hipGetLastError());
        uint64_t kept = 0;
        MXG_HIP(h, hipMemcpyAsync(&kept, d_tot + ST_KEPT, 8, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
        if (kept > n_blk) return set_err(h, MXG_EDEVICE, "mxg_synteny_blocks: internal error (%llu of %u blocks kept)", (unsigned long long)kept, n_blk);
        n_keep = (uint32_t)kept;
    }
    if (n_keep) {
        MXG_HIP(h, B[SY_OUT].ensure((size_t)n_keep * 32));
        hipLaunchKernelGGL(k_syn_compact, grid(n_blk), b, 0, st, B[SY_BLK].as<SynBlock>(), B[SY_KEEP].as<uint32_t>(), B[SY_KSCAN].as<uint32_t>(), n_blk, n_keep,
                           B[SY_OUT].as<uint32_t>());
        MXG_HIP(h, hipGetLastError());
        S.block.resize((size_t)n_keep * 8);
        MXG_HIP(h, hipMemcpyAsync(S.block.data(), B[SY_OUT].p, (size_t)n_keep * 32, hipMemcpyDeviceToHost, st));
    }
    if (dbg && ev[1]) (void)hipEventRecord(ev[1], st);
    MXG_HIP(h, hipStreamSynchronize(st));
    if (n_keep) {  // (what mxg_synteny_identity reads, where it lies already)
        S.d_anchor = d_a, S.n_dev_blocks = n_blk;
        S.d_first = B[SY_FIRST].as<uint32_t>(), S.d_last = B[SY_LAST].as<uint32_t>();
        S.d_keep = B[SY_KEEP].as<uint32_t>(), S.d_kscan = B[SY_KSCAN].as<uint32_t>();
    }
    S.reverse.resize(n_keep);
    for (uint32_t i = 0; i < n_keep; ++i) S.reverse[i] = (uint8_t)S.block[(size_t)7 * n_keep + i];
    if (dbg) {
        float ms = 0;
        if (ev[0] && ev[1]) (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        fprintf(stderr, "[mxg] synteny_blocks q=%d s=%d vertices=%u anchors=%u links=%llu blocks=%u kept=%u ms=%.3f\n", q, s, nv, n,
                (unsigned long long)S.n_links, n_blk, n_keep, ms);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    S.valid = true;
    return MXG_OK;
}

// ---- the PAF text ------------------------------------------------------------------------------------------------------------------
struct SynPaf {
    const uint32_t *blk;  // eight arrays of n words (k_syn_compact)
    const uint32_t *qlen, *slen;
    const uint64_t *qid_off, *sid_off;  // into ids
    const char *ids;
    uint64_t *loff;  // [n + 1] bytes of the lines, then their offsets
    uint32_t n, k;
    const uint64_t *idy;  // MXG_PAF_IDENTITY: the eight arrays of n words of mxg_synteny_identity; else null
};

template <class Sink> __device__ __forceinline__ void syn_paf_line(const SynPaf &q, uint32_t i, Sink &o)
{
    SynBlock b;
    b.n_anchors = q.blk[i], b.q_record = q.blk[(size_t)q.n + i], b.q_start = q.blk[(size_t)2 * q.n + i], b.q_end = q.blk[(size_t)3 * q.n + i];
    b.s_record = q.blk[(size_t)4 * q.n + i], b.s_start = q.blk[(size_t)5 * q.n + i], b.s_end = q.blk[(size_t)6 * q.n + i];
    b.reverse = q.blk[(size_t)7 * q.n + i];
    o.bytes(q.ids + q.qid_off[b.q_record], q.qid_off[b.q_record + 1] - q.qid_off[b.q_record]);
    o.ch('\t');
    o.num(q.qlen[b.q_record]);
    o.ch('\t');
    o.num(b.q_start);
    o.ch('\t');
    o.num(b.q_end);
    o.ch('\t');
    o.ch(b.reverse ? '-' : '+');
    o.ch('\t');
    o.bytes(q.ids + q.sid_off[b.s_record], q.sid_off[b.s_record + 1] - q.sid_off[b.s_record]);
    o.ch('\t');
    o.num(q.slen[b.s_record]);
    o.ch('\t');
    o.num(b.s_start);
    o.ch('\t');
    o.num(b.s_end);
    o.ch('\t');
    o.num(syn_matches(b, q.k));
    o.ch('\t');
    o.num(syn_blocklen(b));
    o.lit("\t255\tcm:i:", 10u);
    o.num(b.n_anchors);
    if (q.idy) {  // al:i:<aligned_q>, and where anything was aligned NM:i:<edits> and dv:f:<edits / the longer aligned side>, four digits, floored
        const uint64_t aq = q.idy[(size_t)5 * q.n + i], as = q.idy[(size_t)6 * q.n + i], ed = q.idy[(size_t)7 * q.n + i];
        o.lit("\tal:i:", 6u);
        o.num(aq);
        if (aq) {
            o.lit("\tNM:i:", 6u);
            o.num(ed);
            o.lit("\tdv:f:", 6u);
            const uint64_t den = aq > as ? aq : as;
            if (ed >= den) {
                o.lit("1.0000", 6u);
            } else {
                const uint32_t d = (uint32_t)(ed * 10000ull / den);  // (ed < den < 2^50: no overflow)
                o.lit("0.", 2u);
                o.ch((char)('0' + d / 1000u));
                o.ch((char)('0' + d / 100u % 10u));
                o.ch((char)('0' + d / 10u % 10u));
                o.ch((char)('0' + d % 10u));
            }
        }
    }
    o.ch('\n');
}

__global__ __launch_bounds__(256) void k_syn_paf_len(const SynPaf q)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > q.n) return;
    CountSink c;
    if (i < q.n) syn_paf_line(q, i, c);
    q.loff[i] = c.n;  // (entry n: 0, so that the exclusive sums end with the total)
}

// blocks [i0, i1): what their lines have inside the window [lo, hi)
__global__ __launch_bounds__(256) void k_syn_paf_emit(const SynPaf q, uint32_t i0, uint32_t i1, uint64_t lo, uint64_t hi, char *__restrict__ out)
{
    const uint32_t i = i0 + blockIdx.x * 256u + threadIdx.x;
    if (i >= i1) return;
    const uint64_t f_lo = q.loff[i], f_hi = q.loff[i + 1];
    if (f_hi <= lo || f_lo >= hi) return;
    WinSink w{f_lo, lo, hi, out};
    syn_paf_line(q, i, w);
}

int write_synteny_paf(mxg_handle *h, const char *const *query_names, const char *path, int append, uint32_t flags)
{
    const mxg_handle::Synteny &S = h->syn;
    const bool with_idy = (flags & MXG_PAF_IDENTITY) != 0;
    const uint32_t n = (uint32_t)S.reverse.size();
    const Assembly *aq = h->asms[S.q], *as = h->asms[S.s];
    const size_t n_q = S.q_len.size(), n_s = S.s_len.size();
    // ---- names, lengths and the blocks on the device; the lines' offsets
    std::vector<uint64_t> id_off(n_q + n_s + 2, 0);
    std::string ids;
    for (size_t r = 0; r < n_q; ++r) {
        ids += query_names ? query_names[r] : aq->recs[r].id.c_str();
        id_off[r + 1] = ids.size();
    }
    id_off[n_q + 1] = ids.size();
    for (size_t r = 0; r < n_s; ++r) {
        ids += as->recs[r].id;
        id_off[n_q + 2 + r] = ids.size();
    }
    MXG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    DevBuf *B = h->synbuf;
    uint64_t total = 0;
    SynPaf q{};
    const bool dbg = getenv("MXG_DEBUG_IO") != nullptr;
    hipEvent_t ev[2] = {};
    if (dbg && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess) (void)hipEventRecord(ev[0], st);
    if (n) {
        const size_t cnt = (size_t)n + 1, n_tiles = (cnt + PT_TILE - 1) / PT_TILE;
        MXG_HIP(h, B[SY_OUT].ensure((size_t)n * 32));
        MXG_HIP(h, B[SY_QLEN].ensure(n_q * 4 + 4));
        MXG_HIP(h, B[SY_SLEN].ensure(n_s * 4 + 4));
        MXG_HIP(h, B[SY_IDOFF].ensure(id_off.size() * 8));
        MXG_HIP(h, B[SY_IDS].ensure(ids.size() + 16));
        MXG_HIP(h, B[SY_LOFF].ensure(cnt * 8));
        MXG_HIP(h, B[SY_TSUM].ensure(n_tiles * 8));
        // (the blocks from the host copy: the view's arrays are what the text is promised to spell, whatever ran on the handle since)
        MXG_HIP(h, hipMemcpyAsync(B[SY_OUT].p, S.block.data(), (size_t)n * 32, hipMemcpyHostToDevice, st));
        if (n_q) MXG_HIP(h, hipMemcpyAsync(B[SY_QLEN].p, S.q_len.data(), n_q * 4, hipMemcpyHostToDevice, st));
        if (n_s) MXG_HIP(h, hipMemcpyAsync(B[SY_SLEN].p, S.s_len.data(), n_s * 4, hipMemcpyHostToDevice, st));
        MXG_HIP(h, hipMemcpyAsync(B[SY_IDOFF].p, id_off.data(), id_off.size() * 8, hipMemcpyHostToDevice, st));
        if (!ids.empty()) MXG_HIP(h, hipMemcpyAsync(B[SY_IDS].p, ids.data(), ids.size(), hipMemcpyHostToDevice, st));
        q.blk = B[SY_OUT].as<uint32_t>();
        q.qlen = B[SY_QLEN].as<uint32_t>(), q.slen = B[SY_SLEN].as<uint32_t>();
        q.qid_off = B[SY_IDOFF].as<uint64_t>(), q.sid_off = q.qid_off + n_q + 1;
        q.ids = B[SY_IDS].as<char>();
        q.loff = B[SY_LOFF].as<uint64_t>();
        q.n = n, q.k = h->cfg.k;
        if (with_idy) {  // (from the host copy, as the blocks: what the identity view spells)
            MXG_HIP(h, B[SY_IDY].ensure((size_t)n * 64));
            MXG_HIP(h, hipMemcpyAsync(B[SY_IDY].p, h->idy.blk.data(), (size_t)n * 64, hipMemcpyHostToDevice, st));
            q.idy = B[SY_IDY].as<uint64_t>();
        }
        hipLaunchKernelGGL(k_syn_paf_len, dim3((uint32_t)((cnt + 255) / 256)), dim3(256), 0, st, q);
        launch_scan_u64(st, q.loff, n + 1, B[SY_TSUM].as<uint64_t>());
        MXG_HIP(h, hipGetLastError());
        MXG_HIP(h, hipMemcpyAsync(&total, q.loff + n, 8, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
    }
    // ---- the file
    const uint64_t WIN = std::max<uint64_t>(1, std::min<uint64_t>(knob_u64(h, "MXG_SYN_WIN", PIN_HALF), PIN_HALF));
    OutFile of;
    uint64_t base = 0;
    if (!(append ? of.open_append(path, &base) : of.open(path))) return set_err(h, MXG_EIO, "cannot open '%s' for writing", path);
    if (total) {
        const uint64_t n_win = (total + WIN - 1) / WIN;
        if (n_win >= 0xFFFFFFFFull)
            return set_err(h, MXG_ELIMIT, "mxg_write_synteny_paf: %llu windows of MXG_SYN_WIN bytes for '%s'", (unsigned long long)n_win, path);
        std::vector<uint32_t> bounds(n_win);
        MXG_HIP(h, B[SY_BOUNDS].ensure(n_win * 4));
        // bounds[c] = the block whose line holds byte c * WIN
        launch_win_bounds(st, q.loff, n, WIN, (uint32_t)n_win, B[SY_BOUNDS].as<uint32_t>());
        MXG_HIP(h, hipGetLastError());
        MXG_HIP(h, hipMemcpyAsync(bounds.data(), B[SY_BOUNDS].p, n_win * 4, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
        const WinFill fill = [&](uint64_t c, unsigned char *d_win, uint64_t lo, uint64_t hi) -> int {
            // (the block that holds byte hi holds byte hi - 1 or follows the block that does)
            const uint32_t i0 = bounds[c], i1 = c + 1 < n_win ? std::min(n, bounds[c + 1] + 1) : n;
            hipLaunchKernelGGL(k_syn_paf_emit, dim3((i1 - i0 + 255) / 256), dim3(256), 0, st, q, i0, i1, lo, hi, reinterpret_cast<char *>(d_win));
            MXG_HIP(h, hipGetLastError());
            return MXG_OK;
        };
        const int rc = write_windows(h, of, total, WIN, base, fill, "mxg_write_synteny_paf");
        if (rc != MXG_OK) return rc;
    }
    if (!of.close()) return set_err(h, MXG_EIO, "mxg_write_synteny_paf: write error while closing '%s'", path);
    of.complete = true;
    if (dbg) {
        float ms = 0;
        if (ev[1]) (void)hipEventRecord(ev[1], st);
        (void)hipStreamSynchronize(st);
        if (ev[0] && ev[1]) (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        fprintf(stderr, "[mxg] write_synteny_paf blocks=%u bytes=%llu ms=%.3f\n", n, (unsigned long long)total, ms);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    return MXG_OK;
}

}  // namespace mxg
