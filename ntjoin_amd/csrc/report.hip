// report.hip -- the assembly report (row f10): contiguity, base composition and N gaps of a loaded assembly's text
// (mxg_assembly_report) and of the scaffold files on their way out (MXG_SCAF_REPORT, mxg_scaffold_report).  The contract is in
// include/ntjoin_mx.h and, executable, in tests/_seqreport_restatement.py; the summaries and the state are in seqstat.h.
//
// The unit of work is an item of at most 4096 bytes of text, 16 per thread in one load.  Three sources give items:
//   RS_INDEXED  the file's text as the device ingest left it, in its work items (text_index.h): one record each, line ends inside;
//   RS_FLAT     host-ingested text without line ends: aligned tiles, a record begins where its origin says;
//   RS_WINDOW   a window of a scaffold file in device memory: aligned tiles, the segment table (from the piece table) says which
//               bytes are sequence and where a header begins.
//   k_rep_items   pass 1.  The lane's bytes -> class masks by bit operations on whole words (seq_lane) -> its counts and its
//                 summary (runs of one class at a time, never byte by byte).  An item without N and without a border is PLAIN: its
//                 summary is its base count.  Otherwise the 256 summaries are folded in order in LDS.  Per item: the summary, the
//                 counts, the N runs that begin in it (what the lists can hold at the most) and the plain flag.
//   k_rep_agg / k_rep_tile_scan / k_rep_states   the ordered scan over the items with seq_combine: every item's incoming state.
//                 The one block of the middle kernel starts from the state the device keeps and leaves the state behind the last
//                 item there: between the windows of a file it never comes to the host.  An N run of any length is a chain of
//                 summaries that are all N: the scan carries it, nothing walks it.  k_rep_agg also adds the counts up.
//   k_rep_emit    pass 2, for the items that are not plain only: the lanes' summaries again, scanned in LDS behind the item's
//                 incoming state, then every lane walks its runs from ITS incoming state and appends the gaps and contigs that end
//                 in its bytes to the two lists through an atomic cursor.  Plain items are not read a second time: one thread ends
//                 the run such an item is entered with, if there is one.
//   k_rep_close   the end of the text closes the last record.
// Between the scan and pass 2 the host reads the totals (one small copy) and makes the lists large enough: N runs begun so far for
// the gaps, that plus the records plus one for the contigs.  The lists come to the host once, at the end; the contiguity blocks
// are made there (seq_contiguity).
#include <algorithm>
#include <string>

#include "bisect.h"
#include "mxg_internal.h"
#include "seqstat.h"
#include "text_index.h"

namespace mxg {

enum : uint32_t { RS_INDEXED = 0, RS_FLAT = 1, RS_WINDOW = 2 };
enum { RB_ITEMS, RB_AGG, RB_EXCL, RB_STATES, RB_TOT, RB_STATE, RB_GAPS, RB_CTGS, RB_ORG, RB_SEGS, RB_BUF_COUNT };
static_assert(RB_BUF_COUNT <= 16, "mxg_handle::repbuf too small");
enum : uint32_t { RT_STARTS = SQ_COUNTS, RT_OVERFLOW = SQ_COUNTS + 1, RT_NGAP = SQ_COUNTS + 2, RT_NCTG = SQ_COUNTS + 3, RT_WORDS = SQ_COUNTS + 4 };
constexpr uint32_t REP_TILE = 4096;

struct RepSrc {
    const unsigned char *text;
    uint32_t route;
    const IngItem *items;       // RS_INDEXED
    const uint64_t *rec_item0;
    const uint64_t *org;        // RS_FLAT: [n_org] where every record begins in text[0, len)
    uint32_t n_org;
    uint64_t len;
    const RepSeg *segs;         // RS_WINDOW: text holds bytes [lo, hi) of the file; segs[n_segs] ends the last one
    uint32_t n_segs;
    uint64_t lo, hi;
};

struct RepItem {
    SeqSum s;
    uint32_t pk[4];  // A | C << 16, G | T << 16, N | other << 16, lower | N runs begun << 16
    uint32_t plain;
};

struct RepLists {
    uint64_t *gaps, *ctgs;
    uint64_t gap_cap, ctg_cap;
    unsigned long long *tot;  // [RT_WORDS]
};

struct RepSink {
    RepLists l;
    __device__ void gap(uint64_t n)
    {
        const unsigned long long at = atomicAdd(l.tot + RT_NGAP, 1ull);
        if (at < l.gap_cap) l.gaps[at] = n; else l.tot[RT_OVERFLOW] = 1ull;
    }
    __device__ void contig(uint64_t n)
    {
        const unsigned long long at = atomicAdd(l.tot + RT_NCTG, 1ull);
        if (at < l.ctg_cap) l.ctgs[at] = n; else l.tot[RT_OVERFLOW] = 1ull;
    }
};

#define REP_LDS(name) \
    __shared__ __attribute__((aligned(16))) unsigned char name##_raw[256 * sizeof(SeqSum)]; \
    SeqSum *name = reinterpret_cast<SeqSum *>(name##_raw)

// inclusive scan of one summary per thread over a block of 256; afterwards sh[t] holds thread t's result (all threads call)
__device__ __forceinline__ SeqSum rep_block_inclusive(SeqSum v, SeqSum *sh, uint64_t mg)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        SeqSum u;
        if (t >= o) u = sh[t - o];
        __syncthreads();
        if (t >= o) {
            v = seq_combine(u, v, mg);
            sh[t] = v;
        }
        __syncthreads();
    }
    return v;
}

__device__ __forceinline__ uint32_t rep_bits(uint32_t lo, uint32_t hi)  // bits [lo, hi), hi <= 16
{
    return ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// the last j in [lo, hi] with segs[j].out <= x (segs[lo].out <= x)
__device__ __forceinline__ uint32_t rep_seg_of(const RepSeg *segs, uint32_t lo, uint32_t hi, uint64_t x)
{
    return last_where(lo, hi + 1u, [&](uint32_t j) { return segs[j].out <= x; });
}

struct RepLane {
    SeqLane L;
    uint32_t r = 0;  // bit j: a record begins in front of byte j
};

// thread t's 16 bytes of item i (all threads call; s_rng: two words of LDS)
__device__ __forceinline__ RepLane rep_fetch(const RepSrc &q, uint64_t i, uint32_t *s_rng)
{
    const uint32_t t = threadIdx.x;
    RepLane out;
    uint32_t valid = 0;
    uint64_t a0 = 0;  // where the lane's bytes are in q.text
    if (q.route == RS_INDEXED) {
        const IngItem it = q.items[i];
        a0 = (it.lo & ~(uint64_t)(ING_TILE - 1)) + 16u * t;
        const uint64_t lo = max(a0, it.lo), hi = min(a0 + 16u, it.lo + it.len);
        if (lo < hi) {
            valid = rep_bits((uint32_t)(lo - a0), (uint32_t)(hi - a0));
            if (lo == it.lo && i == q.rec_item0[it.rec]) out.r = 1u << (uint32_t)(lo - a0);
        }
    } else if (q.route == RS_FLAT) {
        const uint64_t tile = i * REP_TILE, t_hi = min(q.len, tile + REP_TILE);
        a0 = tile + 16u * t;
        if (t == 0) {
            s_rng[0] = first_ge(q.org, 0u, q.n_org, tile);  // the record starts [s_rng[0], s_rng[1]) inside the tile
            s_rng[1] = first_ge(q.org, s_rng[0], q.n_org, t_hi);
        }
        __syncthreads();
        if (a0 < t_hi) {
            const uint64_t hi = min(a0 + 16u, t_hi);
            valid = rep_bits(0, (uint32_t)(hi - a0));
            if (s_rng[0] < s_rng[1])
                for (uint32_t j = first_ge(q.org, s_rng[0], s_rng[1], a0); j < s_rng[1] && q.org[j] < hi; ++j)
                    out.r |= 1u << (uint32_t)(q.org[j] - a0);
        }
    } else {
        const uint64_t f_tile = q.lo + i * REP_TILE, f_hi = min(q.hi, f_tile + REP_TILE), f0 = f_tile + 16u * t;
        a0 = f0 - q.lo;
        if (t == 0) {
            s_rng[0] = rep_seg_of(q.segs, 0, q.n_segs - 1, f_tile);
            s_rng[1] = rep_seg_of(q.segs, s_rng[0], q.n_segs - 1, f_hi - 1);
        }
        __syncthreads();
        if (f0 < f_hi) {
            const uint64_t e = min(f0 + 16u, f_hi);
            for (uint32_t j = rep_seg_of(q.segs, s_rng[0], s_rng[1], f0); j <= s_rng[1] && q.segs[j].out < e; ++j) {
                const RepSeg sg = q.segs[j];
                const uint64_t s_lo = max(sg.out, f0), s_hi = min(q.segs[j + 1].out, e);
                if (sg.kind == 0u && s_lo < s_hi) valid |= rep_bits((uint32_t)(s_lo - f0), (uint32_t)(s_hi - f0));
                if (sg.kind == 2u && sg.out >= f0) out.r |= 1u << (uint32_t)(sg.out - f0);
            }
        }
    }
    if (valid) {
        const uint4 v = *reinterpret_cast<const uint4 *>(q.text + a0);  // (every source is allocated in whole tiles)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        out.L = seq_lane(w, valid);
    }
    return out;
}

__device__ __forceinline__ uint32_t rep_wave_sum(uint32_t v)
{
    for (uint32_t o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void k_rep_items(const RepSrc q, uint64_t mg, RepItem *__restrict__ items)
{
    REP_LDS(sh);
    __shared__ uint32_t s_rng[2];
    __shared__ uint32_t s_pk[4][4];
    const uint32_t t = threadIdx.x;
    const RepLane ln = rep_fetch(q, blockIdx.x, s_rng);
    const SeqLane &L = ln.L;
    // an N run begins at an N whose byte in front is none, or at a border (in the same wave's bytes; the first lane counts one too
    // many at the most, and so does a line end inside a run)
    uint32_t prev_n = __shfl_up((L.n >> 15) & 1u, 1);
    if ((t & 63u) == 0) prev_n = 0;
    const uint32_t starts = (uint32_t)__popc(L.n & ~(((L.n << 1) | prev_n) & ~ln.r));
    uint32_t pk[4] = {L.cnt[SQ_A] | L.cnt[SQ_C] << 16, L.cnt[SQ_G] | L.cnt[SQ_T] << 16, L.cnt[SQ_N] | L.cnt[SQ_OTHER] << 16,
                      L.cnt[SQ_LOWER] | starts << 16};
    for (uint32_t u = 0; u < 4; ++u) {  // (an item has 4096 bytes at the most: no half overflows)
        pk[u] = rep_wave_sum(pk[u]);
        if ((t & 63u) == 0) s_pk[t >> 6][u] = pk[u];
    }
    const int plain = __syncthreads_and(L.n == 0 && ln.r == 0 ? 1 : 0);  // (block-uniform; s_pk is written)
    for (uint32_t u = 0; u < 4; ++u) pk[u] = s_pk[0][u] + s_pk[1][u] + s_pk[2][u] + s_pk[3][u];
    SeqSum s;
    if (plain) {
        s.p = seq_part_b((uint64_t)(pk[0] & 0xFFFFu) + (pk[0] >> 16) + (pk[1] & 0xFFFFu) + (pk[1] >> 16) + (pk[2] >> 16));
    } else {
        (void)rep_block_inclusive(seq_sum_masks(L.n, L.b, ln.r, mg), sh, mg);
        s = sh[255];
    }
    if (t == 0) {
        RepItem it;
        it.s = s;
        for (uint32_t u = 0; u < 4; ++u) it.pk[u] = pk[u];
        it.plain = plain ? 1u : 0u;
        items[blockIdx.x] = it;
    }
}

// W items a block: their summaries folded, their counts added to the totals
__global__ __launch_bounds__(256) void k_rep_agg(const RepItem *__restrict__ items, uint64_t n_items, uint32_t W, uint64_t mg, SeqSum *__restrict__ agg,
                                                 unsigned long long *__restrict__ tot)
{
    REP_LDS(sh);
    __shared__ uint32_t s_c[4][8];
    const uint32_t t = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * W + t;
    SeqSum v;
    uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (t < W && i < n_items) {
        const RepItem it = items[i];
        v = it.s;
        for (uint32_t u = 0; u < 4; ++u) c[2u * u] = it.pk[u] & 0xFFFFu, c[2u * u + 1u] = it.pk[u] >> 16;
    }
    for (uint32_t u = 0; u < 8; ++u) {  // (256 items of 4096 bytes: 2^20 at the most)
        c[u] = rep_wave_sum(c[u]);
        if ((t & 63u) == 0) s_c[t >> 6][u] = c[u];
    }
    (void)rep_block_inclusive(v, sh, mg);
    if (t == 0) agg[blockIdx.x] = sh[255];
    if (t < 8) {
        const uint32_t sum = s_c[0][t] + s_c[1][t] + s_c[2][t] + s_c[3][t];
        if (sum) atomicAdd(tot + t, (unsigned long long)sum);  // (c[] is in the totals' order: SQ_A .. SQ_LOWER, RT_STARTS)
    }
}

// excl[b] = the state the device keeps, then the blocks in front of block b, folded -- by ONE block, W blocks a round; the state
// behind the last block goes back to where the first came from
__global__ __launch_bounds__(256) void k_rep_tile_scan(const SeqSum *__restrict__ agg, uint32_t n_tiles, uint32_t W, uint64_t mg, SeqSum *__restrict__ excl,
                                                       SeqState *__restrict__ state)
{
    REP_LDS(sh);
    const uint32_t t = threadIdx.x;
    SeqSum carry;
    carry.p = seq_part_of(*state);
    for (uint32_t base = 0; base < n_tiles; base += W) {
        const uint32_t i = base + t;
        SeqSum v;
        if (t < W && i < n_tiles) v = agg[i];
        (void)rep_block_inclusive(v, sh, mg);
        if (t < W && i < n_tiles) excl[i] = t ? seq_combine(carry, sh[t - 1], mg) : carry;
        carry = seq_combine(carry, sh[255], mg);
        __syncthreads();  // (sh is free for the next round)
    }
    if (t == 0) *state = seq_state_of(carry.p, mg, 1u);
}

__global__ __launch_bounds__(256) void k_rep_states(const RepItem *__restrict__ items, uint64_t n_items, uint32_t W, uint64_t mg,
                                                    const SeqSum *__restrict__ excl, SeqState *__restrict__ states)
{
    REP_LDS(sh);
    const uint32_t t = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * W + t;
    SeqSum v;
    if (t < W && i < n_items) v = items[i].s;
    (void)rep_block_inclusive(v, sh, mg);
    if (t >= W || i >= n_items) return;
    const SeqSum e = excl[blockIdx.x];
    states[i] = seq_state_of((t ? seq_combine(e, sh[t - 1], mg) : e).p, mg, 1u);
}

__global__ __launch_bounds__(256) void k_rep_emit(const RepSrc q, uint64_t mg, const RepItem *__restrict__ items, const SeqState *__restrict__ states,
                                                  const RepLists lists)
{
    REP_LDS(sh);
    __shared__ uint32_t s_rng[2];
    const uint32_t t = threadIdx.x;
    if (items[blockIdx.x].plain) {  // (block-uniform) bases that are no N and nothing else: all that can end here is the run it is entered with
        SeqState s = states[blockIdx.x];
        if (t == 0 && s.nrun && !items[blockIdx.x].s.p.all_n) {
            RepSink sink{lists};
            seq_end_run(s, mg, sink);
        }
        return;
    }
    const RepLane ln = rep_fetch(q, blockIdx.x, s_rng);
    (void)rep_block_inclusive(seq_sum_masks(ln.L.n, ln.L.b, ln.r, mg), sh, mg);
    if (!(ln.L.n | ln.L.b | ln.r)) return;
    SeqState s = states[blockIdx.x];
    if (t) s = seq_apply(s, sh[t - 1], mg);
    RepSink sink{lists};
    seq_walk_masks(s, ln.L.n, ln.L.b, ln.r, mg, sink);
}

__global__ void k_rep_close(SeqState *__restrict__ state, uint64_t mg, const RepLists lists)
{
    RepSink sink{lists};
    SeqState s = *state;
    seq_close(s, mg, sink);
    *state = s;
}

// ---- host ----
namespace {

// at least `need` bytes with the first `keep` bytes kept
int rep_grow(mxg_handle *h, DevBuf &b, size_t need, size_t keep)
{
    if (need <= b.bytes) return MXG_OK;
    void *old = b.p;
    const size_t old_bytes = b.bytes;
    b.p = nullptr, b.bytes = 0;
    hipError_t e = b.ensure(need + need / 2);
    if (e == hipSuccess && old && keep) e = hipMemcpyAsync(b.p, old, std::min(keep, old_bytes), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (old) (void)hipFree(old);
    MXG_HIP(h, e);
    return MXG_OK;
}

uint32_t rep_scan_width(mxg_handle *h)
{
    return (uint32_t)std::max<uint64_t>(2, std::min<uint64_t>(knob_u64(h, "MXG_REPORT_SCAN_W", 256), 256));
}

int rep_begin(mxg_handle *h, uint64_t n_records)
{
    DevBuf *B = h->repbuf;
    MXG_HIP(h, hipSetDevice(h->device));
    MXG_HIP(h, B[RB_TOT].ensure(RT_WORDS * 8));
    MXG_HIP(h, B[RB_STATE].ensure(sizeof(SeqState)));
    MXG_HIP(h, hipMemsetAsync(B[RB_TOT].p, 0, RT_WORDS * 8, h->stream));
    MXG_HIP(h, hipMemsetAsync(B[RB_STATE].p, 0, sizeof(SeqState), h->stream));
    h->rep_run = mxg_handle::RepRun();
    h->rep_run.n_records = n_records;
    return MXG_OK;
}

// the two passes over n_items items of q
int rep_pass(mxg_handle *h, const RepSrc &q, uint64_t n_items, const char *who)
{
    if (!n_items) return MXG_OK;
    if (n_items >= 0x7FFFFFFFull) return set_err(h, MXG_ELIMIT, "%s: %llu work items in one pass (fewer than 2^31)", who, (unsigned long long)n_items);
    hipStream_t st = h->stream;
    DevBuf *B = h->repbuf;
    const uint64_t mg = h->rep_min_gap;
    const uint32_t W = rep_scan_width(h);
    const uint32_t n_tiles = (uint32_t)((n_items + W - 1) / W);
    MXG_HIP(h, B[RB_ITEMS].ensure((size_t)n_items * sizeof(RepItem)));
    MXG_HIP(h, B[RB_STATES].ensure((size_t)n_items * sizeof(SeqState)));
    MXG_HIP(h, B[RB_AGG].ensure((size_t)n_tiles * sizeof(SeqSum)));
    MXG_HIP(h, B[RB_EXCL].ensure((size_t)n_tiles * sizeof(SeqSum)));
    RepItem *items = B[RB_ITEMS].as<RepItem>();
    SeqState *states = B[RB_STATES].as<SeqState>();
    unsigned long long *tot = B[RB_TOT].as<unsigned long long>();
    // MXG_DEBUG_IO: one line per pass with the device times of pass 1, the scan and pass 2
    const bool dbg = getenv("MXG_DEBUG_IO") != nullptr;
    hipEvent_t ev[4] = {};
    auto mark = [&](int e) {
        if (dbg && hipEventCreate(&ev[e]) == hipSuccess) (void)hipEventRecord(ev[e], st);
    };
    mark(0);
    hipLaunchKernelGGL(k_rep_items, dim3((uint32_t)n_items), dim3(256), 0, st, q, mg, items);
    mark(1);
    hipLaunchKernelGGL(k_rep_agg, dim3(n_tiles), dim3(256), 0, st, items, n_items, W, mg, B[RB_AGG].as<SeqSum>(), tot);
    hipLaunchKernelGGL(k_rep_tile_scan, dim3(1), dim3(256), 0, st, B[RB_AGG].as<SeqSum>(), n_tiles, W, mg, B[RB_EXCL].as<SeqSum>(),
                       B[RB_STATE].as<SeqState>());
    hipLaunchKernelGGL(k_rep_states, dim3(n_tiles), dim3(256), 0, st, items, n_items, W, mg, B[RB_EXCL].as<SeqSum>(), states);
    mark(2);
    MXG_HIP(h, hipGetLastError());
    // what the lists must hold: every gap is an N run that began somewhere, every contig ends at a gap, a record's end or the text's
    uint64_t starts = 0;
    MXG_HIP(h, hipMemcpyAsync(&starts, tot + RT_STARTS, 8, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    mxg_handle::RepRun &run = h->rep_run;
    run.starts_seen = starts;
    const uint64_t gap_need = starts + 2, ctg_need = starts + run.n_records + 2;
    int rc;
    if ((rc = rep_grow(h, B[RB_GAPS], gap_need * 8, run.gap_cap * 8)) != MXG_OK) return rc;
    if ((rc = rep_grow(h, B[RB_CTGS], ctg_need * 8, run.ctg_cap * 8)) != MXG_OK) return rc;
    run.gap_cap = gap_need, run.ctg_cap = ctg_need;
    const RepLists lists{B[RB_GAPS].as<uint64_t>(), B[RB_CTGS].as<uint64_t>(), run.gap_cap, run.ctg_cap, tot};
    hipEvent_t ev2 = ev[2];
    if (dbg) mark(2);  // (behind the copy of the totals and whatever the lists cost)
    hipLaunchKernelGGL(k_rep_emit, dim3((uint32_t)n_items), dim3(256), 0, st, q, mg, items, states, lists);
    mark(3);
    MXG_HIP(h, hipGetLastError());
    if (dbg) {
        float ms[3] = {0, 0, 0};
        MXG_HIP(h, hipStreamSynchronize(st));
        if (ev[0] && ev[1] && ev2 && ev[2] && ev[3]) {
            (void)hipEventElapsedTime(&ms[0], ev[0], ev[1]);
            (void)hipEventElapsedTime(&ms[1], ev[1], ev2);
            (void)hipEventElapsedTime(&ms[2], ev[2], ev[3]);
        }
        fprintf(stderr, "[mxg] report items=%llu pass1_ms=%.3f scan_ms=%.3f pass2_ms=%.3f run_starts=%llu\n", (unsigned long long)n_items, ms[0], ms[1],
                ms[2], (unsigned long long)starts);
        for (hipEvent_t e : {ev[0], ev[1], ev2, ev[2], ev[3]})
            if (e) (void)hipEventDestroy(e);
    }
    return MXG_OK;
}

// closes the last record; the totals and the lists come to the host
int rep_end(mxg_handle *h, SeqReportHost &out, const char *who)
{
    hipStream_t st = h->stream;
    DevBuf *B = h->repbuf;
    mxg_handle::RepRun &run = h->rep_run;
    int rc;
    if ((rc = rep_grow(h, B[RB_GAPS], (run.starts_seen + 2) * 8, run.gap_cap * 8)) != MXG_OK) return rc;
    if ((rc = rep_grow(h, B[RB_CTGS], (run.starts_seen + run.n_records + 2) * 8, run.ctg_cap * 8)) != MXG_OK) return rc;
    run.gap_cap = run.starts_seen + 2, run.ctg_cap = run.starts_seen + run.n_records + 2;
    unsigned long long *tot = B[RB_TOT].as<unsigned long long>();
    const RepLists lists{B[RB_GAPS].as<uint64_t>(), B[RB_CTGS].as<uint64_t>(), run.gap_cap, run.ctg_cap, tot};
    hipLaunchKernelGGL(k_rep_close, dim3(1), dim3(1), 0, st, B[RB_STATE].as<SeqState>(), h->rep_min_gap, lists);
    MXG_HIP(h, hipGetLastError());
    uint64_t t[RT_WORDS];
    MXG_HIP(h, hipMemcpyAsync(t, tot, sizeof t, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    if (t[RT_OVERFLOW] || t[RT_NGAP] > run.gap_cap || t[RT_NCTG] > run.ctg_cap)
        return set_err(h, MXG_EDEVICE, "internal error: %s: %llu gaps and %llu contigs for lists of %llu and %llu", who, (unsigned long long)t[RT_NGAP],
                       (unsigned long long)t[RT_NCTG], (unsigned long long)run.gap_cap, (unsigned long long)run.ctg_cap);
    out.gap_len.resize(t[RT_NGAP]);
    out.ctg_len.resize(t[RT_NCTG]);
    if (t[RT_NGAP]) MXG_HIP(h, hipMemcpyAsync(out.gap_len.data(), B[RB_GAPS].p, t[RT_NGAP] * 8, hipMemcpyDeviceToHost, st));
    if (t[RT_NCTG]) MXG_HIP(h, hipMemcpyAsync(out.ctg_len.data(), B[RB_CTGS].p, t[RT_NCTG] * 8, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    out.bases = 0;
    for (uint32_t c = 0; c < SQ_COUNTS; ++c) out.cnt[c] = t[c];
    for (uint32_t c = SQ_A; c <= SQ_OTHER; ++c) out.bases += t[c];
    out.min_gap = h->rep_min_gap, out.min_len = h->rep_min_len;
    return MXG_OK;
}

}  // namespace

static mxg_contiguity rep_block(std::vector<uint64_t> &scratch, const std::vector<uint64_t> &len, uint64_t min_len)
{
    scratch = len;
    const SeqContig c = seq_contiguity(scratch.data(), scratch.size(), min_len);
    return mxg_contiguity{c.n, c.n_min, c.sum, c.min, c.max, c.nx[0], c.lx[0], c.nx[1], c.lx[1], c.nx[2], c.lx[2]};
}

void report_fill(const SeqReportHost &r, std::vector<uint64_t> &scratch, mxg_seq_report *out)
{
    const uint32_t size = out->struct_size;
    memset(out, 0, sizeof *out);
    out->struct_size = size;
    out->min_gap = r.min_gap, out->min_len = r.min_len;
    out->n_records = r.n_records, out->bases = r.bases;
    out->a = r.cnt[SQ_A], out->c = r.cnt[SQ_C], out->g = r.cnt[SQ_G], out->t = r.cnt[SQ_T], out->n = r.cnt[SQ_N];
    out->other = r.cnt[SQ_OTHER], out->lower = r.cnt[SQ_LOWER];
    out->n_gaps = r.gap_len.size();
    for (uint64_t g : r.gap_len) out->gap_bases += g, out->max_gap = std::max(out->max_gap, g);
    out->scaffold = rep_block(scratch, r.rec_len, r.min_len);
    out->contig = rep_block(scratch, r.ctg_len, r.min_len);
    out->gap_len = r.gap_len.data(), out->contig_len = r.ctg_len.data();
}

int assembly_report(mxg_handle *h, Assembly *a, int assembly)
{
    const char *who = "mxg_assembly_report";
    h->rep_asm.valid = false;
    if (a->holds_pieces || a->shard_lo != 0 || a->shard_hi < a->recs.size())
        return set_err(h, MXG_EINVAL, "%s: assembly %d holds a shard or pieces of its file, not the whole text", who, assembly);
    const size_t n_rec = a->recs.size();
    const bool indexed = a->text_on_device && a->d_text.p && a->ing_item0.size() == n_rec + 1;
    if (!indexed && !(a->has_text && a->has_bases))
        return set_err(h, MXG_EINVAL, "%s: assembly %d holds no text (a minimizer table from a TSV, side-car or arrays, packed bases handed over on "
                       "the device, text dropped by MXG_FLAG_DROP_SEQ or released by a one-shot handle): the report is made from the text of "
                       "the FASTA", who, assembly);
    if (n_rec >= (1ull << 31)) return set_err(h, MXG_ELIMIT, "%s: %llu records (fewer than 2^31)", who, (unsigned long long)n_rec);
    int rc;
    if ((rc = rep_begin(h, n_rec)) != MXG_OK) return rc;
    hipStream_t st = h->stream;
    DevBuf *B = h->repbuf;
    RepSrc q{};
    uint64_t n_items = 0;
    std::vector<uint64_t> org;
    if (indexed) {
        if (!a->d_ing_item0.p) {
            MXG_HIP(h, a->d_ing_item0.ensure(a->ing_item0.size() * 8));
            MXG_HIP(h, hipMemcpyAsync(a->d_ing_item0.p, a->ing_item0.data(), a->ing_item0.size() * 8, hipMemcpyHostToDevice, st));
        }
        q.route = RS_INDEXED, q.text = a->d_text.as<unsigned char>();
        q.items = a->d_ing_items.as<IngItem>(), q.rec_item0 = a->d_ing_item0.as<uint64_t>();
        n_items = a->ing_item0.back();
    } else {
        org.resize(n_rec);
        uint64_t at = 0;
        for (size_t r = 0; r < n_rec; ++r) {
            if (a->recs[r].text_off != at)
                return set_err(h, MXG_EDEVICE, "internal error: %s: record %llu of assembly %d does not begin where the one before ends", who,
                               (unsigned long long)r, assembly);
            org[r] = at, at += a->recs[r].len;
        }
        if (at != a->text.size())
            return set_err(h, MXG_EDEVICE, "internal error: %s: assembly %d holds %llu bytes of text for %llu bases", who, assembly,
                           (unsigned long long)a->text.size(), (unsigned long long)at);
        if (!a->flat_text_on_device) {  // once per assembly, as the first mxg_write_scaffolds leaves it
            const size_t bytes = (a->text.size() / REP_TILE + 2) * REP_TILE;
            MXG_HIP(h, a->d_text.ensure(bytes));
            MXG_HIP(h, hipMemsetAsync(a->d_text.p, '>', bytes, st));
            if (!a->text.empty()) MXG_HIP(h, hipMemcpyAsync(a->d_text.p, a->text.data(), a->text.size(), hipMemcpyHostToDevice, st));
            a->flat_text_on_device = true;
        }
        MXG_HIP(h, B[RB_ORG].ensure(n_rec * 8 + 16));
        if (n_rec) MXG_HIP(h, hipMemcpyAsync(B[RB_ORG].p, org.data(), n_rec * 8, hipMemcpyHostToDevice, st));
        q.route = RS_FLAT, q.text = a->d_text.as<unsigned char>();
        q.org = B[RB_ORG].as<uint64_t>(), q.n_org = (uint32_t)n_rec, q.len = at;
        n_items = (at + REP_TILE - 1) / REP_TILE;
    }
    if ((rc = rep_pass(h, q, n_items, who)) != MXG_OK) return rc;
    SeqReportHost &out = h->rep_asm;
    if ((rc = rep_end(h, out, who)) != MXG_OK) return rc;  // (waits for the stream: org has left the host)
    out.n_records = n_rec;
    out.rec_len.resize(n_rec);
    uint64_t want = 0;
    for (size_t r = 0; r < n_rec; ++r) out.rec_len[r] = a->recs[r].len, want += a->recs[r].len;
    if (want != out.bases)
        return set_err(h, MXG_EDEVICE, "internal error: %s: assembly %d has %llu bases in its text and %llu in the handle", who, assembly,
                       (unsigned long long)out.bases, (unsigned long long)want);
    out.valid = true;
    return MXG_OK;
}

int report_file_begin(mxg_handle *h, const std::vector<RepSeg> &segs, uint64_t n_records)
{
    int rc;
    if ((rc = rep_begin(h, n_records)) != MXG_OK) return rc;
    if (segs.size() >= 0xFFFFFFFFull) return set_err(h, MXG_ELIMIT, "mxg_write_scaffolds: too many pieces of output for one report");
    DevBuf *B = h->repbuf;
    MXG_HIP(h, B[RB_SEGS].ensure(segs.size() * sizeof(RepSeg) + 16));
    // (pageable memory: the copy returns when the bytes have left the vector)
    if (!segs.empty()) MXG_HIP(h, hipMemcpyAsync(B[RB_SEGS].p, segs.data(), segs.size() * sizeof(RepSeg), hipMemcpyHostToDevice, h->stream));
    MXG_HIP(h, hipStreamSynchronize(h->stream));
    h->rep_run.d_segs = B[RB_SEGS].p;
    h->rep_run.n_segs = segs.empty() ? 0u : (uint32_t)(segs.size() - 1);
    return MXG_OK;
}

int report_file_window(mxg_handle *h, const unsigned char *d_win, uint64_t lo, uint64_t hi)
{
    if (hi <= lo || !h->rep_run.n_segs) return MXG_OK;
    RepSrc q{};
    q.route = RS_WINDOW, q.text = d_win;
    q.segs = static_cast<const RepSeg *>(h->rep_run.d_segs), q.n_segs = h->rep_run.n_segs;
    q.lo = lo, q.hi = hi;
    return rep_pass(h, q, (hi - lo + REP_TILE - 1) / REP_TILE, "mxg_write_scaffolds");
}

int report_file_end(mxg_handle *h, int which, std::vector<uint64_t> &&rec_len, const char *path)
{
    SeqReportHost &out = h->rep_scaf[which];
    out.valid = false;
    int rc;
    if ((rc = rep_end(h, out, "mxg_write_scaffolds")) != MXG_OK) return rc;
    out.rec_len = std::move(rec_len);
    out.n_records = out.rec_len.size();
    uint64_t want = 0;
    for (uint64_t l : out.rec_len) want += l;
    if (want != out.bases)
        return set_err(h, MXG_EDEVICE, "internal error: mxg_write_scaffolds: '%s' has %llu bases in its windows and %llu in its piece table", path,
                       (unsigned long long)out.bases, (unsigned long long)want);
    out.valid = true;
    return MXG_OK;
}

}  // namespace mxg
