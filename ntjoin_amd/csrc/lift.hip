// lift.hip -- mxg_lift_prepare, mxg_lift_intervals, mxg_lift_bed: features of the source records carried through a piece table onto
// the records it spells (include/ntjoin_mx.h, row f15; the rules themselves are lift.h).
// The host checks the table (compose.h's cmp_table, which also gives every piece's record and prefix) and parses BED lines
// (host_io.cpp); everything per piece, feature or part runs on the device:
//   k_lf_flag, scan, k_lf_keys   the sequence pieces compacted, in table order: key (record << 32) | start, payload the piece's index
//   launch_radix_sort            stable, over the 32 bits of `start` and the bits n_source needs of `record` (sort_kernels.h)
//   k_lf_entries                 per sorted piece: what a lookup reads of it in one 16-byte load, and (record << 32) | end
//   launch_max_scan_u64          the running maximum of the latter (scan64_kernels.h)
//   k_lf_count                   per feature: its candidates by two bisections, its parts counted, its status; per block the counts'
//                                64-bit sum, so the host knows the number of parts before anything is scanned in 32 bits
//   scan, k_lf_emit              per feature: its parts, at the scanned place
// The lifted BED is pathtext.hip's shape: one formatter over the two sinks of text_dev.h, a 64-bit scan of the lines' lengths,
// per window the first part by bisection (k_win_bounds), then write_windows (both win_out.hip); MXG_LIFT_WIN sets the bytes per window.
// Plain loads and stores throughout; every write is at an index below the size its array was allocated for (see the launches).
#include <algorithm>
#include <chrono>
#include <string>

#include "compose.h"
#include "lift.h"
#include "mxg_internal.h"
#include "scan64_kernels.h"
#include "scan_kernels.h"
#include "sort_kernels.h"
#include "text_dev.h"

namespace mxg {

enum { LF_PIECES, LF_PREC, LF_PPRE, LF_FLAG, LF_FSCAN, LF_BSUM, LF_K0, LF_V0, LF_K1, LF_V1, LF_COUNTS, LF_RFIRST, LF_RBSUM, LF_ENT, LF_RMAX,
       LF_TMAX, LF_SRCLEN, LF_TOT, LF_FREC, LF_FA, LF_FB, LF_CNT, LF_PSCAN, LF_STATUS, LF_FLO, LF_FHI, LF_BSUM64, LF_PARTS, LF_PFEAT, LF_TEXT,
       LF_REST, LF_NAMES, LF_NAMEOFF, LF_LOFF, LF_TSUM, LF_BOUNDS, LF_BUF_COUNT };
static_assert(LF_BUF_COUNT <= 48, "mxg_handle::lftbuf too small");

// ---- the index -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lf_flag(const mxg_seq_piece *__restrict__ pc, uint32_t n_pc, uint32_t *__restrict__ flag)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_pc) return;
    flag[j] = pc[j].kind != MXG_PIECE_GAP ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_lf_keys(const mxg_seq_piece *__restrict__ pc, const uint32_t *__restrict__ flag,
                                                 const uint32_t *__restrict__ fscan, uint32_t n_pc, uint32_t m, uint64_t *__restrict__ key,
                                                 uint32_t *__restrict__ val)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_pc || !flag[j]) return;
    const uint32_t at = fscan[j];
    if (at >= m) return;  // (cannot be: fscan counts the sequence pieces before j, m is their number)
    const mxg_seq_piece p = pc[j];
    key[at] = lift_key(p.record, p.start);
    val[at] = j;
}

__global__ __launch_bounds__(256) void k_lf_entries(const uint32_t *__restrict__ val, uint32_t m, const mxg_seq_piece *__restrict__ pc,
                                                    const uint32_t *__restrict__ prec, const uint32_t *__restrict__ ppre, uint32_t n_pc,
                                                    LiftEntry *__restrict__ ent, uint64_t *__restrict__ rmax)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    uint32_t j = val[i];
    if (j >= n_pc) j = 0;  // (cannot be: the payloads are indices of sequence pieces)
    const mxg_seq_piece p = pc[j];
    LiftEntry e;
    e.start = p.start, e.end = p.end;
    e.trec = prec[j] | (p.kind == MXG_PIECE_REV ? LFT_REV : 0u);
    e.off = ppre[j];
    ent[i] = e;
    rmax[i] = lift_key(p.record, p.end);
}

int lift_prepare(mxg_handle *h, const mxg_seq_piece *pieces, const uint64_t *first, uint64_t n_records, const uint32_t *source_length,
                 uint64_t n_source)
{
    mxg_handle::Lift &L = h->lift;
    L.valid = false;
    L.m = 0;
    if (n_source >= LFT_MAX) return set_err(h, MXG_ELIMIT, "mxg_lift_prepare: %llu source records (fewer than 2^31)", (unsigned long long)n_source);
    CmpTable tab;
    std::string msg;
    const int rc = cmp_table("table", pieces, first, n_records, n_source, source_length, tab, msg);
    if (rc != MXG_OK) return set_err(h, rc, "mxg_lift_prepare: %s", msg.c_str());
    L.n_records = n_records;
    L.src_len.assign(source_length, source_length + n_source);
    const uint32_t n_pc = (uint32_t)tab.pre.size();
    if (!n_pc) {
        L.valid = true;
        return MXG_OK;
    }
    MXG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    DevBuf *B = h->lftbuf;
    const dim3 b(256);
    auto grid = [](uint64_t n) { return dim3((uint32_t)((n + 255u) / 256u)); };
    const bool dbg = getenv("MXG_DEBUG_IO") != nullptr;
    hipEvent_t ev[2] = {};
    if (dbg && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess) (void)hipEventRecord(ev[0], st);
    MXG_HIP(h, B[LF_PIECES].ensure((size_t)n_pc * sizeof(mxg_seq_piece)));
    for (int id : {LF_PREC, LF_PPRE, LF_FLAG, LF_FSCAN}) MXG_HIP(h, B[id].ensure((size_t)n_pc * 4));
    MXG_HIP(h, B[LF_BSUM].ensure(((size_t)(n_pc + TILE - 1) / TILE) * 4 + 16));
    MXG_HIP(h, B[LF_TOT].ensure(64));
    MXG_HIP(h, B[LF_SRCLEN].ensure((size_t)n_source * 4 + 4));
    MXG_HIP(h, hipMemcpyAsync(B[LF_PIECES].p, pieces, (size_t)n_pc * sizeof(mxg_seq_piece), hipMemcpyHostToDevice, st));
    MXG_HIP(h, hipMemcpyAsync(B[LF_PREC].p, tab.rec.data(), (size_t)n_pc * 4, hipMemcpyHostToDevice, st));
    MXG_HIP(h, hipMemcpyAsync(B[LF_PPRE].p, tab.pre.data(), (size_t)n_pc * 4, hipMemcpyHostToDevice, st));
    if (n_source) MXG_HIP(h, hipMemcpyAsync(B[LF_SRCLEN].p, source_length, (size_t)n_source * 4, hipMemcpyHostToDevice, st));
    const mxg_seq_piece *d_pc = B[LF_PIECES].as<mxg_seq_piece>();
    uint32_t *d_flag = B[LF_FLAG].as<uint32_t>(), *d_fscan = B[LF_FSCAN].as<uint32_t>();
    uint64_t *d_tot = B[LF_TOT].as<uint64_t>();
    // 1: the sequence pieces, counted (every thread j < n_pc writes flag[j])
    hipLaunchKernelGGL(k_lf_flag, grid(n_pc), b, 0, st, d_pc, n_pc, d_flag);
    launch_scan_u32(st, d_flag, n_pc, B[LF_BSUM].as<uint32_t>(), d_fscan, d_tot);
    MXG_HIP(h, hipGetLastError());
    uint64_t m64 = 0;
    MXG_HIP(h, hipMemcpyAsync(&m64, d_tot, 8, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    if (m64 > n_pc) return set_err(h, MXG_EDEVICE, "mxg_lift_prepare: internal error (%llu sequence pieces of %u)", (unsigned long long)m64, n_pc);
    const uint32_t m = (uint32_t)m64;
    if (m) {
        // 2: keys and payloads, compacted (k0 / v0 hold m elements; at < m is checked)
        for (int id : {LF_K0, LF_K1, LF_RMAX}) MXG_HIP(h, B[id].ensure((size_t)m * 8));
        for (int id : {LF_V0, LF_V1}) MXG_HIP(h, B[id].ensure((size_t)m * 4));
        for (int id : {LF_COUNTS, LF_RFIRST}) MXG_HIP(h, B[id].ensure(rs_count_words(m) * 4));
        MXG_HIP(h, B[LF_RBSUM].ensure(rs_bsum_words(m) * 4));
        MXG_HIP(h, B[LF_ENT].ensure((size_t)m * sizeof(LiftEntry)));
        MXG_HIP(h, B[LF_TMAX].ensure(((size_t)(m + PT_TILE - 1) / PT_TILE) * 8));
        hipLaunchKernelGGL(k_lf_keys, grid(n_pc), b, 0, st, d_pc, d_flag, d_fscan, n_pc, m, B[LF_K0].as<uint64_t>(), B[LF_V0].as<uint32_t>());
        // 3: sorted by (record, start); records are below n_source, so the key ends at the highest bit of n_source - 1
        uint32_t key_bits = 32;
        for (uint64_t v = n_source ? n_source - 1 : 0; v; v >>= 1) ++key_bits;
        L.sorted_in = launch_radix_sort(st, B[LF_K0].as<uint64_t>(), B[LF_V0].as<uint32_t>(), B[LF_K1].as<uint64_t>(), B[LF_V1].as<uint32_t>(), m,
                                        key_bits, B[LF_COUNTS].as<uint32_t>(), B[LF_RFIRST].as<uint32_t>(), B[LF_RBSUM].as<uint32_t>(), d_tot + 1);
        // 4: the entries and the running maximum of (record, end) (every thread i < m writes ent[i] and rmax[i])
        hipLaunchKernelGGL(k_lf_entries, grid(m), b, 0, st, B[L.sorted_in ? LF_V1 : LF_V0].as<uint32_t>(), m, d_pc, B[LF_PREC].as<uint32_t>(),
                           B[LF_PPRE].as<uint32_t>(), n_pc, B[LF_ENT].as<LiftEntry>(), B[LF_RMAX].as<uint64_t>());
        launch_max_scan_u64(st, B[LF_RMAX].as<uint64_t>(), m, B[LF_TMAX].as<uint64_t>());
        MXG_HIP(h, hipGetLastError());
    }
    if (dbg && ev[1]) (void)hipEventRecord(ev[1], st);
    MXG_HIP(h, hipStreamSynchronize(st));
    if (dbg) {
        float ms = 0;
        if (ev[0] && ev[1]) (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        fprintf(stderr, "[mxg] lift_prepare pieces=%u sequence_pieces=%u source_records=%llu ms=%.3f\n", n_pc, m, (unsigned long long)n_source, ms);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    L.m = m;
    L.valid = true;
    return MXG_OK;
}

// ---- the lookup ----------------------------------------------------------------------------------------------------------------------
struct LfIndex {
    const uint64_t *key, *rmax;
    const LiftEntry *ent;
    const uint32_t *src_len;
    uint32_t m, n_source;
};

__global__ __launch_bounds__(256) void k_lf_count(const LfIndex x, const uint32_t *__restrict__ frec, const uint32_t *__restrict__ fa,
                                                  const uint32_t *__restrict__ fb, uint32_t n, uint32_t whole_only, uint32_t *__restrict__ cnt,
                                                  uint32_t *__restrict__ status, uint32_t *__restrict__ flo, uint32_t *__restrict__ fhi,
                                                  uint64_t *__restrict__ bsum64)
{
    __shared__ uint64_t sh[256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint64_t c = 0;
    if (i < n) {
        const uint32_t r = frec[i], a = fa[i], b = fb[i];
        uint32_t s = MXG_LIFT_INVALID, lo = 0, hi = 0;
        if (lift_valid(r, a, b, x.n_source, x.src_len)) {
            lift_range(x.key, x.rmax, x.m, r, a, b, lo, hi);
            s = lift_count(x.ent, lo, hi, a, b, c);
            if (whole_only && s != MXG_LIFT_WHOLE) c = 0;
        }
        cnt[i] = (uint32_t)c;  // (c <= m < 2^31)
        status[i] = s;
        flo[i] = lo;
        fhi[i] = hi;
    }
    sh[threadIdx.x] = c;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum64[blockIdx.x] = sh[0];
}

// parts: five arrays of n_parts words (s_record, s_start, s_end, src_start, reverse); pfeat: the feature of every part
__global__ __launch_bounds__(256) void k_lf_emit(const LiftEntry *__restrict__ ent, const uint32_t *__restrict__ fa, const uint32_t *__restrict__ fb,
                                                 uint32_t n, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ pscan,
                                                 const uint32_t *__restrict__ flo, const uint32_t *__restrict__ fhi, uint32_t n_parts,
                                                 uint32_t *__restrict__ parts, uint32_t *__restrict__ pfeat)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cnt[i];
    if (!c) return;
    const uint32_t a = fa[i], b = fb[i], hi = fhi[i], at0 = pscan[i];
    uint32_t t = 0;
    for (uint32_t j = flo[i]; j < hi && t < c; ++j) {
        const LiftEntry e = ent[j];
        if (e.end <= a) continue;
        const uint32_t at = at0 + t;
        if (at >= n_parts) return;  // (cannot be: pscan[i] + cnt[i] <= the scan's total = n_parts)
        const LiftPart p = lift_part(e, a, b);
        parts[at] = p.s_record;
        parts[(size_t)n_parts + at] = p.s_start;
        parts[(size_t)2 * n_parts + at] = p.s_end;
        parts[(size_t)3 * n_parts + at] = p.src_start;
        parts[(size_t)4 * n_parts + at] = p.reverse;
        pfeat[at] = i;
        ++t;
    }
}

static float lf_event_ms(hipEvent_t a, hipEvent_t b)
{
    float ms = 0;
    if (a && b) (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}

// host_parts: the parts come home too (mxg_lift_intervals); statuses and part_first always do.  The parts stay in LF_PARTS / LF_PFEAT
int lift_intervals(mxg_handle *h, const uint32_t *record, const uint32_t *start, const uint32_t *end, uint64_t n64, uint32_t flags, bool host_parts)
{
    mxg_handle::Lift &L = h->lift;
    L.n_parts = 0;
    L.part_first.assign(1, 0);
    L.status.clear(), L.reverse.clear(), L.parts.clear();
    if (n64 >= LFT_MAX) return set_err(h, MXG_ELIMIT, "mxg_lift_intervals: %llu features in one call (fewer than 2^31)", (unsigned long long)n64);
    const uint32_t n = (uint32_t)n64;
    if (!n) return MXG_OK;
    L.part_first.assign((size_t)n + 1, 0);
    L.status.resize(n);
    MXG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    DevBuf *B = h->lftbuf;
    const dim3 b(256);
    const uint32_t blocks = (n + 255u) / 256u;
    const bool dbg = getenv("MXG_DEBUG_IO") != nullptr;
    hipEvent_t ev[2] = {};
    if (dbg && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess) (void)hipEventRecord(ev[0], st);
    for (int id : {LF_FREC, LF_FA, LF_FB, LF_CNT, LF_PSCAN, LF_STATUS, LF_FLO, LF_FHI}) MXG_HIP(h, B[id].ensure((size_t)n * 4));
    MXG_HIP(h, B[LF_BSUM64].ensure((size_t)blocks * 8));
    MXG_HIP(h, B[LF_BSUM].ensure(((size_t)(n + TILE - 1) / TILE) * 4 + 16));
    MXG_HIP(h, B[LF_TOT].ensure(64));
    MXG_HIP(h, B[LF_SRCLEN].ensure(L.src_len.size() * 4 + 4));  // (a table without pieces: prepare uploaded nothing)
    if (!L.m && !L.src_len.empty())
        MXG_HIP(h, hipMemcpyAsync(B[LF_SRCLEN].p, L.src_len.data(), L.src_len.size() * 4, hipMemcpyHostToDevice, st));
    MXG_HIP(h, hipMemcpyAsync(B[LF_FREC].p, record, (size_t)n * 4, hipMemcpyHostToDevice, st));
    MXG_HIP(h, hipMemcpyAsync(B[LF_FA].p, start, (size_t)n * 4, hipMemcpyHostToDevice, st));
    MXG_HIP(h, hipMemcpyAsync(B[LF_FB].p, end, (size_t)n * 4, hipMemcpyHostToDevice, st));
    LfIndex x;
    x.key = B[L.sorted_in ? LF_K1 : LF_K0].as<uint64_t>(), x.rmax = B[LF_RMAX].as<uint64_t>(), x.ent = B[LF_ENT].as<LiftEntry>();
    x.src_len = B[LF_SRCLEN].as<uint32_t>();
    x.m = L.m, x.n_source = (uint32_t)L.src_len.size();
    const uint32_t *d_fa = B[LF_FA].as<uint32_t>(), *d_fb = B[LF_FB].as<uint32_t>();
    uint32_t *d_cnt = B[LF_CNT].as<uint32_t>(), *d_pscan = B[LF_PSCAN].as<uint32_t>(), *d_status = B[LF_STATUS].as<uint32_t>();
    uint32_t *d_flo = B[LF_FLO].as<uint32_t>(), *d_fhi = B[LF_FHI].as<uint32_t>();
    uint64_t *d_tot = B[LF_TOT].as<uint64_t>();
    // 1: count (every thread i < n writes cnt, status, flo, fhi at i; every block its sum).  The number of parts as a 64-bit sum
    hipLaunchKernelGGL(k_lf_count, dim3(blocks), b, 0, st, x, B[LF_FREC].as<uint32_t>(), d_fa, d_fb, n, (flags & MXG_LIFT_WHOLE_ONLY) ? 1u : 0u, d_cnt,
                       d_status, d_flo, d_fhi, B[LF_BSUM64].as<uint64_t>());
    MXG_HIP(h, hipGetLastError());
    std::vector<uint64_t> bsum(blocks);
    std::vector<uint32_t> status32(n), pscan(n);
    MXG_HIP(h, hipMemcpyAsync(bsum.data(), B[LF_BSUM64].p, (size_t)blocks * 8, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipMemcpyAsync(status32.data(), d_status, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    uint64_t n_parts64 = 0;
    for (uint64_t v : bsum) n_parts64 += v;
    if (n_parts64 >= LFT_MAX) {
        L.part_first.assign(1, 0);
        L.status.clear();
        return set_err(h, MXG_ELIMIT, "mxg_lift_intervals: the features have %llu parts (fewer than 2^31)", (unsigned long long)n_parts64);
    }
    const uint32_t n_parts = (uint32_t)n_parts64;
    for (uint32_t i = 0; i < n; ++i) L.status[i] = (uint8_t)status32[i];
    // 2: scan, emit (parts holds 5 n_parts words, pfeat n_parts; at < n_parts is checked)
    launch_scan_u32(st, d_cnt, n, B[LF_BSUM].as<uint32_t>(), d_pscan, d_tot);
    MXG_HIP(h, hipGetLastError());
    uint64_t tot = 0;
    MXG_HIP(h, hipMemcpyAsync(pscan.data(), d_pscan, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipMemcpyAsync(&tot, d_tot, 8, hipMemcpyDeviceToHost, st));
    if (n_parts) {
        MXG_HIP(h, B[LF_PARTS].ensure((size_t)n_parts * 20));
        MXG_HIP(h, B[LF_PFEAT].ensure((size_t)n_parts * 4));
        hipLaunchKernelGGL(k_lf_emit, dim3(blocks), b, 0, st, x.ent, d_fa, d_fb, n, d_cnt, d_pscan, d_flo, d_fhi, n_parts, B[LF_PARTS].as<uint32_t>(),
                           B[LF_PFEAT].as<uint32_t>());
        MXG_HIP(h, hipGetLastError());
        if (host_parts) {
            L.parts.resize((size_t)n_parts * 5);
            MXG_HIP(h, hipMemcpyAsync(L.parts.data(), B[LF_PARTS].p, (size_t)n_parts * 20, hipMemcpyDeviceToHost, st));
        }
    }
    if (dbg && ev[1]) (void)hipEventRecord(ev[1], st);
    MXG_HIP(h, hipStreamSynchronize(st));
    if (tot != n_parts64)
        return set_err(h, MXG_EDEVICE, "mxg_lift_intervals: the scan gives %llu parts, the count gave %llu", (unsigned long long)tot,
                       (unsigned long long)n_parts64);
    for (uint32_t i = 0; i < n; ++i) L.part_first[i] = pscan[i];
    L.part_first[n] = n_parts;
    L.n_parts = n_parts;
    if (host_parts) {
        L.reverse.resize(n_parts);
        for (uint32_t g = 0; g < n_parts; ++g) L.reverse[g] = (uint8_t)L.parts[(size_t)4 * n_parts + g];
    }
    if (dbg) {
        fprintf(stderr, "[mxg] lift_intervals features=%u parts=%u ms=%.3f\n", n, n_parts, lf_event_ms(ev[0], ev[1]));
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    return MXG_OK;
}

// ---- the lifted BED ------------------------------------------------------------------------------------------------------------------
struct LfBed {
    const uint32_t *parts, *pfeat;                      // k_lf_emit's
    const uint32_t *rest_off, *rest_len, *strand;       // per feature, into text
    const char *text;                                   // the batch
    const uint64_t *name_off;                           // [n_names + 1] into names
    const char *names;
    uint64_t *loff;  // [n_parts + 1] bytes of the lines, then their offsets
    uint32_t n_parts, n_names;
};

template <class Sink> __device__ __forceinline__ void lf_bed_line(const LfBed &q, uint32_t g, Sink &o)
{
    uint32_t R = q.parts[g];
    if (R >= q.n_names) R = 0;  // (cannot be: a part's record is a record of the table)
    const uint32_t f = q.pfeat[g];
    o.bytes(q.names + q.name_off[R], q.name_off[R + 1] - q.name_off[R]);
    o.ch('\t');
    o.num(q.parts[(size_t)q.n_parts + g]);
    o.ch('\t');
    o.num(q.parts[(size_t)2 * q.n_parts + g]);
    const uint32_t ro = q.rest_off[f];
    if (ro != LFT_NONE) {
        const uint32_t rl = q.rest_len[f], so = q.strand[f];
        o.ch('\t');
        if (so != LFT_NONE && q.parts[(size_t)4 * q.n_parts + g]) {
            o.bytes(q.text + ro, so - ro);
            o.ch(lift_flip(q.text[so]));
            o.bytes(q.text + so + 1, ro + rl - so - 1u);
        } else {
            o.bytes(q.text + ro, rl);
        }
    }
    o.ch('\n');
}

__global__ __launch_bounds__(256) void k_lf_bed_len(const LfBed q)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g > q.n_parts) return;
    CountSink c;
    if (g < q.n_parts) lf_bed_line(q, g, c);
    q.loff[g] = c.n;  // (entry n_parts: 0, so that the exclusive sums end with the total)
}

// parts [g0, g1): what their lines have inside the window [lo, hi)
__global__ __launch_bounds__(256) void k_lf_bed_emit(const LfBed q, uint32_t g0, uint32_t g1, uint64_t lo, uint64_t hi, char *__restrict__ out)
{
    const uint32_t g = g0 + blockIdx.x * 256u + threadIdx.x;
    if (g >= g1) return;
    const uint64_t f_lo = q.loff[g], f_hi = q.loff[g + 1];
    if (f_hi <= lo || f_lo >= hi) return;
    WinSink w{f_lo, lo, hi, out};
    lf_bed_line(q, g, w);
}

int lift_bed(mxg_handle *h, const char *bed_path, const char *const *source_names, const char *const *scaffold_names, const char *lifted_path,
             const char *unlifted_path, uint32_t flags, mxg_lift_stats *stats)
{
    using clk = std::chrono::steady_clock;
    mxg_handle::Lift &L = h->lift;
    const uint64_t n_source = L.src_len.size(), n_names = L.n_records;
    mxg_lift_stats S{};
    BedFile bf;
    if (!bf.open(bed_path)) return set_err(h, MXG_EIO, "mxg_lift_bed: cannot read '%s'", bed_path);
    struct NamesGuard {
        BedNames *p;
        ~NamesGuard() { bed_names_free(p); }
    } names{bed_names_make(source_names, n_source)};
    const uint64_t BATCH = std::max<uint64_t>(1, knob_u64(h, "MXG_LIFT_BATCH", 256ull << 20));
    const uint64_t WIN = std::max<uint64_t>(1, std::min<uint64_t>(knob_u64(h, "MXG_LIFT_WIN", PIN_HALF), PIN_HALF));
    MXG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    DevBuf *B = h->lftbuf;
    // ---- the scaffolds' names on the device
    std::vector<uint64_t> name_off(n_names + 1, 0);
    std::string ids;
    for (uint64_t r = 0; r < n_names; ++r) {
        ids += scaffold_names[r];
        name_off[r + 1] = ids.size();
    }
    MXG_HIP(h, B[LF_NAMEOFF].ensure(name_off.size() * 8));
    MXG_HIP(h, B[LF_NAMES].ensure(ids.size() + 16));
    MXG_HIP(h, hipMemcpyAsync(B[LF_NAMEOFF].p, name_off.data(), name_off.size() * 8, hipMemcpyHostToDevice, st));
    if (!ids.empty()) MXG_HIP(h, hipMemcpyAsync(B[LF_NAMES].p, ids.data(), ids.size(), hipMemcpyHostToDevice, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    OutFile lf, uf;
    if (!lf.open(lifted_path)) return set_err(h, MXG_EIO, "cannot open '%s' for writing", lifted_path);
    if (unlifted_path && !uf.open(unlifted_path)) return set_err(h, MXG_EIO, "cannot open '%s' for writing", unlifted_path);
    const bool dbg = getenv("MXG_DEBUG_IO") != nullptr;
    double s_parse = 0, s_lift = 0, s_format = 0;
    float ms_format = 0;
    BedBatch bb;
    std::string un;
    for (uint64_t from = 0;; from = bb.hi) {
        auto t0 = clk::now();
        if (!bed_next_batch(bf, from, BATCH, names.p, bb)) break;
        s_parse += std::chrono::duration<double>(clk::now() - t0).count();
        S.lines += bb.lines, S.skipped += bb.skipped;
        const uint64_t n = bb.record.size(), n_bytes = bb.hi - bb.lo;
        S.features += n;
        if (!n) continue;
        if (n_bytes >= LFT_NONE)
            return set_err(h, MXG_ELIMIT, "mxg_lift_bed: a line of %llu bytes at byte %llu of '%s' (fewer than 2^32 - 1)", (unsigned long long)n_bytes,
                           (unsigned long long)bb.lo, bed_path);
        // ---- lift
        t0 = clk::now();
        int rc = lift_intervals(h, bb.record.data(), bb.a.data(), bb.b.data(), n, flags, false);
        if (rc != MXG_OK) return rc;
        s_lift += std::chrono::duration<double>(clk::now() - t0).count();
        for (uint64_t i = 0; i < n; ++i) {
            if (bb.unknown[i]) L.status[i] = MXG_LIFT_UNKNOWN;
            ++S.status[L.status[i]];
        }
        // ---- format and append
        t0 = clk::now();
        const uint32_t n_parts = (uint32_t)L.n_parts;
        S.parts += n_parts;
        if (n_parts) {
            hipEvent_t ev[2] = {};
            if (dbg && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess) (void)hipEventRecord(ev[0], st);
            const size_t cnt = (size_t)n_parts + 1, n_tiles = (cnt + PT_TILE - 1) / PT_TILE;
            MXG_HIP(h, B[LF_TEXT].ensure(n_bytes + 16));
            MXG_HIP(h, B[LF_REST].ensure((size_t)n * 12));
            MXG_HIP(h, B[LF_LOFF].ensure(cnt * 8));
            MXG_HIP(h, B[LF_TSUM].ensure(n_tiles * 8));
            uint32_t *d_rest = B[LF_REST].as<uint32_t>();
            MXG_HIP(h, hipMemcpyAsync(B[LF_TEXT].p, bf.text + bb.lo, n_bytes, hipMemcpyHostToDevice, st));
            MXG_HIP(h, hipMemcpyAsync(d_rest, bb.rest_off.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
            MXG_HIP(h, hipMemcpyAsync(d_rest + n, bb.rest_len.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
            MXG_HIP(h, hipMemcpyAsync(d_rest + 2 * n, bb.strand.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
            LfBed q;
            q.parts = B[LF_PARTS].as<uint32_t>(), q.pfeat = B[LF_PFEAT].as<uint32_t>();
            q.rest_off = d_rest, q.rest_len = d_rest + n, q.strand = d_rest + 2 * n;
            q.text = B[LF_TEXT].as<char>();
            q.name_off = B[LF_NAMEOFF].as<uint64_t>(), q.names = B[LF_NAMES].as<char>();
            q.loff = B[LF_LOFF].as<uint64_t>();
            q.n_parts = n_parts, q.n_names = (uint32_t)n_names;
            // (every thread g <= n_parts writes loff[g]; loff holds n_parts + 1 words)
            hipLaunchKernelGGL(k_lf_bed_len, dim3((uint32_t)((cnt + 255) / 256)), dim3(256), 0, st, q);
            launch_scan_u64(st, q.loff, n_parts + 1, B[LF_TSUM].as<uint64_t>());
            MXG_HIP(h, hipGetLastError());
            uint64_t total = 0;
            MXG_HIP(h, hipMemcpyAsync(&total, q.loff + n_parts, 8, hipMemcpyDeviceToHost, st));
            MXG_HIP(h, hipStreamSynchronize(st));
            const uint64_t n_win = (total + WIN - 1) / WIN;
            if (n_win >= 0xFFFFFFFFull)
                return set_err(h, MXG_ELIMIT, "mxg_lift_bed: %llu windows of MXG_LIFT_WIN bytes for '%s'", (unsigned long long)n_win, lifted_path);
            std::vector<uint32_t> bounds(n_win);
            MXG_HIP(h, B[LF_BOUNDS].ensure(n_win * 4));
            // bounds[c] = the part whose line holds byte c * WIN
            launch_win_bounds(st, q.loff, n_parts, WIN, (uint32_t)n_win, B[LF_BOUNDS].as<uint32_t>());
            MXG_HIP(h, hipGetLastError());
            MXG_HIP(h, hipMemcpyAsync(bounds.data(), B[LF_BOUNDS].p, n_win * 4, hipMemcpyDeviceToHost, st));
            MXG_HIP(h, hipStreamSynchronize(st));
            const WinFill fill = [&](uint64_t c, unsigned char *d_win, uint64_t lo, uint64_t hi) -> int {
                // (the part that holds byte hi holds byte hi - 1 or follows the part that does)
                const uint32_t g0 = bounds[c], g1 = c + 1 < n_win ? std::min(n_parts, bounds[c + 1] + 1) : n_parts;
                hipLaunchKernelGGL(k_lf_bed_emit, dim3((g1 - g0 + 255) / 256), dim3(256), 0, st, q, g0, g1, lo, hi, reinterpret_cast<char *>(d_win));
                MXG_HIP(h, hipGetLastError());
                return MXG_OK;
            };
            rc = write_windows(h, lf, total, WIN, S.lifted_bytes, fill, "mxg_lift_bed");
            if (rc != MXG_OK) return rc;
            S.lifted_bytes += total;
            if (ev[1]) (void)hipEventRecord(ev[1], st);
            MXG_HIP(h, hipStreamSynchronize(st));
            ms_format += lf_event_ms(ev[0], ev[1]);
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
        if (unlifted_path) {
            un.clear();
            for (uint64_t i = 0; i < n; ++i) {
                if (L.status[i] == MXG_LIFT_WHOLE) continue;
                un += '#';
                un += lift_reason(L.status[i]);
                un += '\n';
                un.append(bf.text + bb.line_off[i], bb.line_len[i]);
                un += '\n';
            }
            if (!uf.put(un.data(), un.size(), S.unlifted_bytes, host_threads(h))) return set_err(h, MXG_EIO, "write error on '%s'", unlifted_path);
            S.unlifted_bytes += un.size();
        }
        s_format += std::chrono::duration<double>(clk::now() - t0).count();
    }
    const bool c_lf = lf.close(), c_uf = uf.close();
    if (!(c_lf && c_uf)) return set_err(h, MXG_EIO, "mxg_lift_bed: write error while closing the output files");
    lf.complete = uf.complete = true;
    if (dbg)
        fprintf(stderr, "[mxg] lift_bed lines=%llu features=%llu parts=%llu bytes=%llu parse_s=%.4f lift_s=%.4f format_write_s=%.4f format_dev_ms=%.3f\n",
                (unsigned long long)S.lines, (unsigned long long)S.features, (unsigned long long)S.parts, (unsigned long long)S.lifted_bytes, s_parse,
                s_lift, s_format, ms_format);
    if (stats) *stats = S;
    return MXG_OK;
}

}  // namespace mxg
