// identity.hip -- mxg_identity_segments: the banded edit distance of explicit segments over texts the handle holds on the device
// (include/ntjoin_mx.h, row f14; the per-segment routine is identity.h).
// The host resolves the two texts, checks every interval against its record and uploads the segments; then
//   k_idy_segments   one lane per segment: the status rules that need no base; the first byte of either interval (text_of_base for
//                    a file's text, an offset per record for the kept scaffold text); idy_align over two byte streams
// A stream hands out one base class per call from an aligned 8-byte word held in registers: a load per eight bytes, line breaks
// passed over, the subject's walked backwards and complemented for a reverse segment.  No LDS, no scratch: the band, the four
// match masks and the two words are the lane's state.
// mxg_synteny_identity runs the same kernel over segments made on the device from what mxg_synteny_blocks left in its scratch:
//   k_idy_kept       per block: a kept block's first anchor and anchor count at its place among the kept
//   scan             over the counts: a kept block's first segment
//   k_idy_build      one thread per anchor of a kept block (its block by bisection over the scan): the segment of the link to the
//                    next anchor, or the tail segment of the block's last anchor
//   k_idy_keys, radix sort (sort_kernels.h)   the segments by falling length: the order in which the lanes take them
//   k_idy_segments   (the results go to the segment's own place)
//   k_idy_fill       per segment six 64-bit words: its status counters in pairs of 32 bits, the flag, lq, ls, edits
//   6 scans (scan64_kernels.h), k_idy_block_sums   a block's sums are the differences of the prefix sums at its borders
// Plain loads and stores; a lane writes edits[i] and status[i] of its own segment i < n only.  A stream reads the aligned word
// that holds a base of a checked interval: inside the text's allocation, which is padded to whole tiles behind its last byte.
#include <algorithm>
#include <string>

#include "identity.h"
#include "mxg_internal.h"
#include "scan64_kernels.h"
#include "scan_kernels.h"
#include "sort_kernels.h"
#include "synteny.h"
#include "text_index.h"

namespace mxg {

enum { IB_SEGS, IB_EDITS, IB_STATUS, IB_QORG, IB_SORG, IB_KFIRST, IB_KCNT, IB_KOFF, IB_BSUM, IB_TOT, IB_VALS, IB_TSUM, IB_OUT, IB_K0, IB_K1, IB_V0, IB_V1,
       IB_RCNT, IB_RFIRST, IB_RBSUM, IB_BUF_COUNT };
static_assert(IB_BUF_COUNT <= 24, "mxg_handle::idybuf too small");
constexpr uint32_t IDY_VALS = 6;   // 64-bit words scanned per segment (k_idy_fill)
constexpr uint32_t IDY_FIELDS = 8; // per-block results (mxg_identity_view)
constexpr uint64_t IDY_MAX = 0x7FFFFFFFull;  // 2^31 segments or more: MXG_ELIMIT

struct IdyText {
    const unsigned char *text;
    uint32_t indexed;         // 1: a file's text with line ends and its tile index; 0: rec_org[r] is the byte of record r's first base
    TextIndex ix;
    const uint64_t *rec_org;  // indexed: the records' packed base offsets (ix.rec_base)
};

__device__ __forceinline__ uint64_t idy_byte_of(const IdyText &t, uint32_t rec, uint32_t pos)
{
    return t.indexed ? text_of_base(t.ix, rec, pos) : t.rec_org[rec] + pos;
}

// the base classes of a text from byte `at` on, forwards (dir = 1) or backwards and complemented (dir = -1)
struct IdyStream {
    const unsigned char *text;
    uint64_t at, wbase, word;
    int64_t dir;
    __device__ __forceinline__ IdyStream(const unsigned char *t, uint64_t a, bool backwards) : text(t), at(a), wbase(~0ull), word(0), dir(backwards ? -1 : 1) {}
    __device__ __forceinline__ uint32_t next()
    {
        uint32_t c;
        do {
            const uint64_t wb = at & ~7ull;
            if (wb != wbase) {
                word = *reinterpret_cast<const uint64_t *>(text + wb);
                wbase = wb;
            }
            c = idy_byte_class((uint32_t)(word >> (8u * (uint32_t)(at & 7u))) & 0xFFu);
            at += (uint64_t)dir;
        } while (c == 5u);
        return dir < 0 && c < 4u ? 3u - c : c;
    }
};

// order: null, or a permutation of 0 .. n - 1: lane t takes segment order[t] (mxg_synteny_identity: the segments by falling length)
__global__ __launch_bounds__(64) void k_idy_segments(const IdyText tq, const IdyText ts, const mxg_identity_seg *__restrict__ segs, uint32_t n,
                                                     uint32_t max_seg, const uint32_t *__restrict__ order, uint32_t *__restrict__ edits,
                                                     uint32_t *__restrict__ status)
{
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= n) return;
    const uint32_t i = order ? order[t] : t;
    if (i >= n) return;  // (cannot be: the sort moves the values 0 .. n - 1 about)
    const mxg_identity_seg g = segs[i];
    uint32_t e = 0, sat = 0;
    uint32_t st = idy_precheck(g.lq, g.ls, max_seg);
    if (!g.lq || !g.ls) st = MXG_IDY_SKIP_SHIFT;  // (cannot be: the host refuses such a segment, neighbouring anchors differ in both positions)
    if (st == MXG_IDY_ALIGNED) {
        const bool rev = g.reverse != 0;
        IdyStream q(tq.text, idy_byte_of(tq, g.q_record, g.q_start), false);
        IdyStream s(ts.text, idy_byte_of(ts, g.s_record, rev ? g.s_start + g.ls - 1u : g.s_start), rev);
        st = idy_align(q, s, g.lq, g.ls, &e, &sat);
        if (st != MXG_IDY_ALIGNED) e = 0, sat = 0;
    }
    edits[i] = e;
    status[i] = st | (sat ? MXG_IDY_SATURATED : 0u);
}

// text `which` of the handle as the kernel reads it, and its records' lengths; org: the slot of the records' offsets
static int idy_text(mxg_handle *h, const char *who, int which, int org, IdyText &t, std::vector<uint64_t> &len)
{
    hipStream_t st = h->stream;
    DevBuf *B = h->idybuf;
    std::vector<uint64_t> off;
    t = IdyText{};
    if (which == MXG_TEXT_SCAFFOLDS) {
        if (!h->scaf_keep_valid || !h->scaf_keep.p)
            return set_err(h, MXG_EINVAL, "%s: the handle's last mxg_write_scaffolds kept no text (MXG_SCAF_KEEP)", who);
        // the kept text is ">id\n" + bases + "\n" per record: every record one line
        const size_t n_rec = h->scaf_keep_first.size() - 1;
        len.assign(n_rec, 0);
        off.resize(n_rec);
        uint64_t at = 0;
        for (size_t r = 0; r < n_rec; ++r) {
            for (uint64_t p = h->scaf_keep_first[r]; p < h->scaf_keep_first[r + 1]; ++p) len[r] += h->scaf_keep_pieces[p].end - h->scaf_keep_pieces[p].start;
            off[r] = at + h->scaf_keep_id[r].size() + 2;
            at = off[r] + len[r] + 1;
        }
        if (at != h->scaf_keep_bytes)
            return set_err(h, MXG_EDEVICE, "%s: internal error (the kept text has %llu bytes, its records spell %llu)", who,
                           (unsigned long long)h->scaf_keep_bytes, (unsigned long long)at);
        t.text = h->scaf_keep.as<unsigned char>();
        t.indexed = 0;
    } else {
        if (which < 0 || (size_t)which >= h->asms.size()) return set_err(h, MXG_EINVAL, "%s: no assembly %d", who, which);
        Assembly *a = h->asms[which];
        if (a->holds_pieces || a->shard_lo != 0 || a->shard_hi < a->recs.size())
            return set_err(h, MXG_EINVAL, "%s: assembly %d holds a shard or pieces of its file, not the whole text", who, which);
        if (!(a->text_on_device && a->d_text.p) || a->ing_item0.size() != a->recs.size() + 1)
            return set_err(h, MXG_EINVAL, "%s: assembly %d: the handle does not hold the file's text on the device (a minimizer table from a TSV, "
                           "side-car or arrays, packed bases, MXG_HOST_INGEST=1, plain gzip, a pipe, text dropped by MXG_FLAG_DROP_SEQ or "
                           "released by a one-shot handle)", who, which);
        const size_t n_rec = a->recs.size();
        len.resize(n_rec);
        off.resize(n_rec);
        for (size_t r = 0; r < n_rec; ++r) len[r] = std::min<uint64_t>(a->recs[r].len, 0xFFFFFFFFull), off[r] = a->recs[r].base_off;  // (starts are 32-bit)
        if (!a->d_ing_item0.p) {
            MXG_HIP(h, a->d_ing_item0.ensure(a->ing_item0.size() * 8));
            MXG_HIP(h, hipMemcpyAsync(a->d_ing_item0.p, a->ing_item0.data(), a->ing_item0.size() * 8, hipMemcpyHostToDevice, st));
        }
        t.text = a->d_text.as<unsigned char>();
        t.indexed = 1;
    }
    MXG_HIP(h, B[org].ensure(off.size() * 8 + 16));
    if (!off.empty()) MXG_HIP(h, hipMemcpyAsync(B[org].p, off.data(), off.size() * 8, hipMemcpyHostToDevice, st));
    MXG_HIP(h, hipStreamSynchronize(st));  // (off has left the host)
    t.rec_org = B[org].as<uint64_t>();
    if (t.indexed) {
        const Assembly *a = h->asms[which];
        t.ix = TextIndex{t.text, a->d_ing_items.as<IngItem>(), a->d_ing_pbase.as<uint64_t>(), a->d_ing_sub.as<uint16_t>(), a->d_ing_item0.as<uint64_t>(),
                         t.rec_org};
    }
    return MXG_OK;
}

int identity_segments(mxg_handle *h, int q_text, int s_text, const mxg_identity_seg *segs, uint64_t n, uint32_t max_seg, uint32_t *out_edits,
                      uint32_t *out_status)
{
    if (n >= IDY_MAX) return set_err(h, MXG_ELIMIT, "mxg_identity_segments: %llu segments (fewer than 2^31)", (unsigned long long)n);
    MXG_HIP(h, hipSetDevice(h->device));
    IdyText tq, ts;
    std::vector<uint64_t> qlen, slen;
    int rc;
    if ((rc = idy_text(h, "mxg_identity_segments", q_text, IB_QORG, tq, qlen)) != MXG_OK) return rc;
    if ((rc = idy_text(h, "mxg_identity_segments", s_text, IB_SORG, ts, slen)) != MXG_OK) return rc;
    for (uint64_t i = 0; i < n; ++i) {
        const mxg_identity_seg &g = segs[i];
        const unsigned long long ui = i;
        if (g.q_record >= qlen.size()) return set_err(h, MXG_EINVAL, "mxg_identity_segments: segment %llu: no query record %u", ui, g.q_record);
        if (g.s_record >= slen.size()) return set_err(h, MXG_EINVAL, "mxg_identity_segments: segment %llu: no subject record %u", ui, g.s_record);
        if (!g.lq || !g.ls) return set_err(h, MXG_EINVAL, "mxg_identity_segments: segment %llu: lq = %u, ls = %u (at least one base each)", ui, g.lq, g.ls);
        if ((uint64_t)g.q_start + g.lq > qlen[g.q_record])
            return set_err(h, MXG_EINVAL, "mxg_identity_segments: segment %llu: query bases [%u, +%u) end beyond record %u (%llu bases)", ui, g.q_start, g.lq,
                           g.q_record, (unsigned long long)qlen[g.q_record]);
        if ((uint64_t)g.s_start + g.ls > slen[g.s_record])
            return set_err(h, MXG_EINVAL, "mxg_identity_segments: segment %llu: subject bases [%u, +%u) end beyond record %u (%llu bases)", ui, g.s_start,
                           g.ls, g.s_record, (unsigned long long)slen[g.s_record]);
    }
    if (!n) return MXG_OK;
    hipStream_t st = h->stream;
    DevBuf *B = h->idybuf;
    const bool dbg = getenv("MXG_DEBUG_IO") != nullptr;
    hipEvent_t ev[2] = {};
    MXG_HIP(h, B[IB_SEGS].ensure((size_t)n * sizeof(mxg_identity_seg)));
    MXG_HIP(h, B[IB_EDITS].ensure((size_t)n * 4));
    MXG_HIP(h, B[IB_STATUS].ensure((size_t)n * 4));
    MXG_HIP(h, hipMemcpyAsync(B[IB_SEGS].p, segs, (size_t)n * sizeof(mxg_identity_seg), hipMemcpyHostToDevice, st));
    if (dbg && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess) (void)hipEventRecord(ev[0], st);
    // (every lane i < n writes edits[i] and status[i])
    hipLaunchKernelGGL(k_idy_segments, dim3((uint32_t)((n + 63u) / 64u)), dim3(64), 0, st, tq, ts, B[IB_SEGS].as<mxg_identity_seg>(), (uint32_t)n, max_seg,
                       static_cast<const uint32_t *>(nullptr), B[IB_EDITS].as<uint32_t>(), B[IB_STATUS].as<uint32_t>());
    MXG_HIP(h, hipGetLastError());
    if (dbg && ev[1]) (void)hipEventRecord(ev[1], st);
    MXG_HIP(h, hipMemcpyAsync(out_edits, B[IB_EDITS].p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipMemcpyAsync(out_status, B[IB_STATUS].p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    if (dbg) {
        float ms = 0;
        if (ev[0] && ev[1]) (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        fprintf(stderr, "[mxg] identity_segments q_text=%d s_text=%d segments=%llu ms=%.3f\n", q_text, s_text, (unsigned long long)n, ms);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    return MXG_OK;
}

// ---- the segments of the kept blocks ----------------------------------------------------------------------------------------------
// first / last: a block's first and last anchor (k_syn_ends); kscan: the kept blocks before it
__global__ __launch_bounds__(256) void k_idy_kept(const uint32_t *__restrict__ first, const uint32_t *__restrict__ last, const uint32_t *__restrict__ keep,
                                                  const uint32_t *__restrict__ kscan, uint32_t n_blk, uint32_t n_keep, uint32_t n_anchor,
                                                  uint32_t *__restrict__ kfirst, uint32_t *__restrict__ kcnt)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_blk || !keep[b]) return;
    const uint32_t at = kscan[b], j = first[b], l = last[b];
    if (at >= n_keep) return;  // (cannot be: kscan counts the kept blocks before b)
    const bool ok = j < l && l < n_anchor;  // (every kept block is: k_syn_blocks keeps no other)
    kfirst[at] = ok ? j : 0u;
    kcnt[at] = ok ? l - j + 1u : 0u;
}

// one thread per segment g; its block is the largest i with koff[i] <= g (every kept block has segments)
__global__ __launch_bounds__(256) void k_idy_build(const SynAnchor *__restrict__ a, const uint32_t *__restrict__ kfirst, const uint32_t *__restrict__ kcnt,
                                                   const uint32_t *__restrict__ koff, uint32_t n_keep, uint32_t k, uint32_t n_seg,
                                                   mxg_identity_seg *__restrict__ segs)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_seg) return;
    const uint32_t lo = last_le(koff, 0u, n_keep, g);
    const uint32_t t = g - koff[lo], cnt = kcnt[lo], j = kfirst[lo];
    mxg_identity_seg o{};
    if (t < cnt && cnt >= 2u) {  // (else cannot be: g lies below the scan's total; lq = ls = 0 is passed over by the segment kernel)
        const bool rev = a[j + 1u].spos < a[j].spos;
        const SynAnchor x = a[j + t];
        o.q_record = x.qrec, o.s_record = x.srec, o.reverse = rev ? 1u : 0u;
        o.q_start = x.qpos;
        if (t + 1u < cnt) {
            const SynAnchor y = a[j + t + 1u];
            o.lq = y.qpos - x.qpos;
            o.s_start = rev ? y.spos + k : x.spos;
            o.ls = rev ? x.spos - y.spos : y.spos - x.spos;
        } else {
            o.lq = o.ls = k;
            o.s_start = x.spos;
        }
    }
    segs[g] = o;
}

// the sort key of a segment, so that a wave's lanes run about equally long: 0xFFFF less the longer side (the long
// ones first), 0xFFFF for a segment no base of which is read
__global__ __launch_bounds__(256) void k_idy_keys(const mxg_identity_seg *__restrict__ segs, uint32_t n, uint32_t max_seg, uint64_t *__restrict__ key,
                                                  uint32_t *__restrict__ val)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t lq = segs[i].lq, ls = segs[i].ls, m = lq > ls ? lq : ls;
    const bool run = lq && ls && idy_precheck(lq, ls, max_seg) == MXG_IDY_ALIGNED;
    key[i] = run ? 0xFFFFu - (m < 0xFFFEu ? m : 0xFFFEu) : 0xFFFFu;
    val[i] = i;
}

// v: IDY_VALS arrays of n + 1 words (entry n: 0, so that the exclusive sums end with the totals)
__global__ __launch_bounds__(256) void k_idy_fill(const mxg_identity_seg *__restrict__ segs, const uint32_t *__restrict__ edits,
                                                  const uint32_t *__restrict__ status, uint32_t n, uint64_t *__restrict__ v)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    uint64_t w[IDY_VALS] = {0, 0, 0, 0, 0, 0};
    if (i < n) {
        const uint32_t st = status[i] & MXG_IDY_STATUS_MASK;
        const bool al = st == MXG_IDY_ALIGNED;
        w[0] = (al ? 1ull : 0ull) | (st == MXG_IDY_SKIP_LEN ? 1ull << 32 : 0ull);
        w[1] = (st == MXG_IDY_SKIP_SHIFT ? 1ull : 0ull) | (st == MXG_IDY_SKIP_N ? 1ull << 32 : 0ull);
        w[2] = status[i] & MXG_IDY_SATURATED ? 1ull : 0ull;
        w[3] = al ? segs[i].lq : 0ull;
        w[4] = al ? segs[i].ls : 0ull;
        w[5] = al ? edits[i] : 0ull;
    }
#pragma unroll
    for (uint32_t u = 0; u < IDY_VALS; ++u) v[(size_t)u * (n + 1u) + i] = w[u];
}

// v: the exclusive sums of k_idy_fill's words; out: IDY_FIELDS arrays of n_keep words, in the view's order
__global__ __launch_bounds__(256) void k_idy_block_sums(const uint32_t *__restrict__ koff, const uint32_t *__restrict__ kcnt, uint32_t n_keep,
                                                        const uint64_t *__restrict__ v, uint32_t n_seg, uint64_t *__restrict__ out)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_keep) return;
    const uint32_t lo = koff[b], hi = lo + kcnt[b];
    if (hi > n_seg) return;  // (cannot be: the counts sum to n_seg)
    uint64_t d[IDY_VALS];
#pragma unroll
    for (uint32_t u = 0; u < IDY_VALS; ++u) d[u] = v[(size_t)u * (n_seg + 1u) + hi] - v[(size_t)u * (n_seg + 1u) + lo];
    // (a block has fewer than 2^31 segments: neither half of a pair carries into the other)
    const uint64_t f[IDY_FIELDS] = {d[0] & 0xFFFFFFFFull, d[0] >> 32, d[1] & 0xFFFFFFFFull, d[1] >> 32, d[2], d[3], d[4], d[5]};
#pragma unroll
    for (uint32_t u = 0; u < IDY_FIELDS; ++u) out[(size_t)u * n_keep + b] = f[u];
}

int synteny_identity(mxg_handle *h, const mxg_identity_params &p)
{
    const char *who = "mxg_synteny_identity";
    mxg_handle::Synteny &S = h->syn;
    mxg_handle::Identity &I = h->idy;
    I.valid = false;
    I.n_segments = 0;
    I.blk.clear();
    const uint32_t n_keep = (uint32_t)S.reverse.size();
    MXG_HIP(h, hipSetDevice(h->device));
    // ---- the two texts, and that they are the records the blocks were made over
    IdyText tq, ts;
    std::vector<uint64_t> qlen, slen;
    int rc;
    if (S.q_table && h->scaf_keep_valid && h->scaf_keep_asm != S.q)
        return set_err(h, MXG_EINVAL, "%s: the blocks' query went through a piece table over assembly %d; the kept scaffold text was cut from assembly %d", who,
                       S.q, h->scaf_keep_asm);
    if ((rc = idy_text(h, who, S.q_table ? MXG_TEXT_SCAFFOLDS : S.q, IB_QORG, tq, qlen)) != MXG_OK) return rc;
    if ((rc = idy_text(h, who, S.s, IB_SORG, ts, slen)) != MXG_OK) return rc;
    auto same = [](const std::vector<uint64_t> &x, const std::vector<uint32_t> &y) {
        if (x.size() != y.size()) return false;
        for (size_t r = 0; r < x.size(); ++r)
            if (x[r] != y[r]) return false;
        return true;
    };
    if (!same(qlen, S.q_len))
        return set_err(h, MXG_EINVAL, S.q_table ? "%s: the piece table of the blocks call is not the one of the kept scaffold text (mxg_scaffold_pieces): "
                                                  "%zu records against %zu, or other lengths"
                                                : "%s: the query lengths of the blocks call are not those of the assembly's text: %zu records against %zu, "
                                                  "or other lengths", who, S.q_len.size(), qlen.size());
    if (!same(slen, S.s_len))
        return set_err(h, MXG_EINVAL, "%s: the subject lengths of the blocks call are not those of the assembly's text: %zu records against %zu, or other lengths",
                       who, S.s_len.size(), slen.size());
    if (!n_keep) {
        I.valid = true;
        return MXG_OK;
    }
    if (!S.d_anchor || !S.n_dev_blocks) return set_err(h, MXG_EDEVICE, "%s: internal error (the blocks call left no anchors on the device)", who);
    hipStream_t st = h->stream;
    DevBuf *B = h->idybuf;
    const dim3 b(256);
    auto grid = [](uint64_t n) { return dim3((uint32_t)((n + 255u) / 256u)); };
    const bool dbg = getenv("MXG_DEBUG_IO") != nullptr;
    hipEvent_t ev[2] = {};
    if (dbg && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess) (void)hipEventRecord(ev[0], st);
    // ---- 1: the kept blocks' first anchors and counts (every kept block writes its entry at < n_keep), the scan
    for (int id : {IB_KFIRST, IB_KCNT, IB_KOFF}) MXG_HIP(h, B[id].ensure((size_t)n_keep * 4));
    MXG_HIP(h, B[IB_BSUM].ensure(((size_t)(n_keep + TILE - 1) / TILE) * 4 + 16));
    MXG_HIP(h, B[IB_TOT].ensure(8));
    uint32_t *d_kfirst = B[IB_KFIRST].as<uint32_t>(), *d_kcnt = B[IB_KCNT].as<uint32_t>(), *d_koff = B[IB_KOFF].as<uint32_t>();
    MXG_HIP(h, hipMemsetAsync(d_kcnt, 0, (size_t)n_keep * 4, st));
    MXG_HIP(h, hipMemsetAsync(d_kfirst, 0, (size_t)n_keep * 4, st));
    hipLaunchKernelGGL(k_idy_kept, grid(S.n_dev_blocks), b, 0, st, S.d_first, S.d_last, S.d_keep, S.d_kscan, S.n_dev_blocks, n_keep, (uint32_t)S.n_anchors,
                       d_kfirst, d_kcnt);
    // (a 32-bit scan: the counts sum to at most twice the anchors, fewer than 2^32; the 64-bit total says whether to 2^31)
    launch_scan_u32(st, d_kcnt, n_keep, B[IB_BSUM].as<uint32_t>(), d_koff, B[IB_TOT].as<uint64_t>());
    MXG_HIP(h, hipGetLastError());
    uint64_t n_seg64 = 0;
    MXG_HIP(h, hipMemcpyAsync(&n_seg64, B[IB_TOT].p, 8, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    uint64_t expect = 0;
    for (uint32_t i = 0; i < n_keep; ++i) expect += S.block[i];  // (n_anchors of the kept blocks, as the view spells them)
    if (n_seg64 != expect) return set_err(h, MXG_EDEVICE, "%s: internal error (%llu segments on the device, %llu anchors in the kept blocks)", who,
                                          (unsigned long long)n_seg64, (unsigned long long)expect);
    if (n_seg64 >= IDY_MAX) return set_err(h, MXG_ELIMIT, "%s: %llu segments (fewer than 2^31)", who, (unsigned long long)n_seg64);
    const uint32_t n_seg = (uint32_t)n_seg64;
    // ---- 2: the segments (every thread g < n_seg writes segs[g]), their distances
    MXG_HIP(h, B[IB_SEGS].ensure((size_t)n_seg * sizeof(mxg_identity_seg)));
    MXG_HIP(h, B[IB_EDITS].ensure((size_t)n_seg * 4));
    MXG_HIP(h, B[IB_STATUS].ensure((size_t)n_seg * 4));
    mxg_identity_seg *d_segs = B[IB_SEGS].as<mxg_identity_seg>();
    hipLaunchKernelGGL(k_idy_build, grid(n_seg), b, 0, st, static_cast<const SynAnchor *>(S.d_anchor), d_kfirst, d_kcnt, d_koff, n_keep, h->cfg.k, n_seg, d_segs);
    // the lanes' segments by falling length (a stable radix sort of 16-bit keys), so that a wave's lanes end together: twice as fast as the
    // list's own order at 4.5 M segments (DESIGN.md 4p has both measured); MXG_IDY_ORDER=0: in list order, without the sort
    const uint32_t *d_order = nullptr;
    if (knob_u64(h, "MXG_IDY_ORDER", 1) != 0) {
        for (int id : {IB_K0, IB_K1}) MXG_HIP(h, B[id].ensure((size_t)n_seg * 8));
        for (int id : {IB_V0, IB_V1}) MXG_HIP(h, B[id].ensure((size_t)n_seg * 4));
        for (int id : {IB_RCNT, IB_RFIRST}) MXG_HIP(h, B[id].ensure(rs_count_words(n_seg) * 4));
        MXG_HIP(h, B[IB_RBSUM].ensure(rs_bsum_words(n_seg) * 4 + 16));
        hipLaunchKernelGGL(k_idy_keys, grid(n_seg), b, 0, st, d_segs, n_seg, p.max_seg, B[IB_K0].as<uint64_t>(), B[IB_V0].as<uint32_t>());
        const int at = launch_radix_sort(st, B[IB_K0].as<uint64_t>(), B[IB_V0].as<uint32_t>(), B[IB_K1].as<uint64_t>(), B[IB_V1].as<uint32_t>(), n_seg, 16u,
                                         B[IB_RCNT].as<uint32_t>(), B[IB_RFIRST].as<uint32_t>(), B[IB_RBSUM].as<uint32_t>(), B[IB_TOT].as<uint64_t>());
        d_order = B[at ? IB_V1 : IB_V0].as<uint32_t>();
        // (a lane whose place the sort left unwritten would skip its segment: the results start as "skipped by shift", edits 0)
        MXG_HIP(h, hipMemsetAsync(B[IB_EDITS].p, 0, (size_t)n_seg * 4, st));
        MXG_HIP(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(B[IB_STATUS].p), (int)MXG_IDY_SKIP_SHIFT, n_seg, st));
    }
    hipLaunchKernelGGL(k_idy_segments, dim3((n_seg + 63u) / 64u), dim3(64), 0, st, tq, ts, d_segs, n_seg, p.max_seg, d_order, B[IB_EDITS].as<uint32_t>(),
                       B[IB_STATUS].as<uint32_t>());
    MXG_HIP(h, hipGetLastError());
    // ---- 3: per segment six words (every thread i <= n_seg writes entry i of each), scanned; per block the differences
    const size_t cnt = (size_t)n_seg + 1;
    MXG_HIP(h, B[IB_VALS].ensure(cnt * 8 * IDY_VALS));
    MXG_HIP(h, B[IB_TSUM].ensure(((cnt + PT_TILE - 1) / PT_TILE) * 8));
    MXG_HIP(h, B[IB_OUT].ensure((size_t)n_keep * 8 * IDY_FIELDS));
    uint64_t *d_v = B[IB_VALS].as<uint64_t>();
    hipLaunchKernelGGL(k_idy_fill, grid(cnt), b, 0, st, d_segs, B[IB_EDITS].as<uint32_t>(), B[IB_STATUS].as<uint32_t>(), n_seg, d_v);
    for (uint32_t u = 0; u < IDY_VALS; ++u) launch_scan_u64(st, d_v + (size_t)u * cnt, n_seg + 1u, B[IB_TSUM].as<uint64_t>());
    MXG_HIP(h, hipMemsetAsync(B[IB_OUT].p, 0, (size_t)n_keep * 8 * IDY_FIELDS, st));
    hipLaunchKernelGGL(k_idy_block_sums, grid(n_keep), b, 0, st, d_koff, d_kcnt, n_keep, d_v, n_seg, B[IB_OUT].as<uint64_t>());
    MXG_HIP(h, hipGetLastError());
    I.blk.resize((size_t)n_keep * IDY_FIELDS);
    MXG_HIP(h, hipMemcpyAsync(I.blk.data(), B[IB_OUT].p, (size_t)n_keep * 8 * IDY_FIELDS, hipMemcpyDeviceToHost, st));
    if (dbg && ev[1]) (void)hipEventRecord(ev[1], st);
    MXG_HIP(h, hipStreamSynchronize(st));
    I.n_segments = n_seg;
    I.valid = true;
    if (dbg) {
        float ms = 0;
        if (ev[0] && ev[1]) (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        fprintf(stderr, "[mxg] synteny_identity q=%d s=%d table=%d order=%d blocks=%u segments=%u ms=%.3f\n", S.q, S.s, S.q_table ? 1 : 0, d_order ? 1 : 0,
                n_keep, n_seg, ms);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    return MXG_OK;
}

}  // namespace mxg
