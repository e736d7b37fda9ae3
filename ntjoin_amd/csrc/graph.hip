// graph.hip -- the minimizer-graph stage on gfx950: per-assembly uniqueness, cross-assembly intersection,
// adjacency edges with support masks and weights.  Replaces (reference file:line):
//   read_minimizers' duplicate removal      bin/ntjoin_utils.py:182-193  (hash seen >= 2x in an assembly is dropped everywhere in it)
//   filter_minimizers                        bin/ntjoin_utils.py:152-165  (keep hashes present in every assembly)
//   build_graph + calc_total_weight          bin/ntjoin_utils.py:83-115,132-137,54-56
//
// Design (no sort needed): one open-addressing table in HBM keyed by the 64-bit out_hash holds, per key,
// a `seen` and a `dup` bit per assembly.  A hash survives iff seen == all assemblies and dup == 0, i.e. it
// occurs exactly once in every assembly.  Survivors get dense vertex ids (rank in the first assembly's
// order).  Because each survivor occurs once per assembly, a vertex has at most one successor and one
// predecessor per assembly: adjacency is one dense array adj[a][v] = {successor, predecessor}; the support mask of edge
// {u,v} is read off that array and the edge is emitted once, by the first assembly (reference order:
// refs in CLI order, then target) that contains it, in that assembly's first-seen orientation --
// the same (s,t) the reference's `edges[s][t]` dictionary keeps (bin/ntjoin_utils.py:101-108).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <system_error>
#include <thread>

#include "join_verdict.h"
#include "graph_rank.h"
#include "mxg_internal.h"
#include "scan_kernels.h"

namespace mxg {

static constexpr uint64_t HT_EMPTY = 0xFFFFFFFFFFFFFFFFull;
static constexpr uint32_t NONE32 = 0xFFFFFFFFu;

// One table slot (16 B): {key, ~seen mask, ~dup mask}.  The masks are stored INVERTED so that a single 0xFF fill
// initialises a slot completely (key = empty sentinel, nothing seen, nothing duplicated).
struct Slot {
    unsigned long long key;
    uint32_t nseen, ndup;
};

__device__ __forceinline__ uint32_t ht_slot(Slot *tab, uint32_t mask, uint32_t cap, uint64_t key)
{
    if (key == HT_EMPTY) return cap;  // the sentinel value itself lives in the extra slot [cap]
    uint32_t s = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
    while (true) {
        unsigned long long cur = tab[s].key;
        if (cur == key) return s;
        if (cur == HT_EMPTY) {
            unsigned long long old = atomicCAS(&tab[s].key, (unsigned long long)HT_EMPTY, (unsigned long long)key);
            if (old == HT_EMPTY || old == key) return s;
        }
        s = (s + 1) & mask;
    }
}

// all assemblies of the handle in one launch: block b works on 256 minimizers of assembly a, bstart[a] <= b < bstart[a+1]
struct AsmSet {
    uint32_t n_asm;
    uint32_t full;                              // mask with one bit per assembly
    uint32_t n[MXG_MAX_ASSEMBLIES];             // minimizers per assembly (an upper bound when n_ptr[a] is set)
    const uint32_t *n_ptr[MXG_MAX_ASSEMBLIES];  // fused sketch+graph call: the count is still on the device
    uint32_t bstart[MXG_MAX_ASSEMBLIES + 1];    // exclusive prefix of 256-element blocks
    const uint64_t *hash[MXG_MAX_ASSEMBLIES];
    uint32_t *slot[MXG_MAX_ASSEMBLIES];
    uint8_t *flags[MXG_MAX_ASSEMBLIES];
    uint64_t *fol;                              // partitioned join: bit t of word 4 b + q = minimizer 64 q + t of block b is a follower
};

__device__ __forceinline__ uint32_t asm_n(const AsmSet &p, uint32_t a)
{
    return p.n_ptr[a] ? min(*p.n_ptr[a], p.n[a]) : p.n[a];
}
__device__ __forceinline__ uint32_t asm_of_block(const AsmSet &p, uint32_t b)
{
    uint32_t a = 0;
    while (a + 1 < p.n_asm && b >= p.bstart[a + 1]) ++a;  // block-uniform, <= 32 steps
    return a;
}

// insert every minimizer of every assembly; remember its slot
__global__ __launch_bounds__(256) void k_insert(const AsmSet p, Slot *tab, uint32_t mask, uint32_t cap, uint32_t *sup,
                                                uint32_t n_sup)
{
    if (blockIdx.x == 0)  // super-counts of the two counting kernels that follow (scan_kernels.h)
        for (uint32_t i = threadIdx.x; i < n_sup; i += 256) sup[i] = 0;
    const uint32_t a = asm_of_block(p, blockIdx.x);
    const uint32_t i = (blockIdx.x - p.bstart[a]) * 256u + threadIdx.x;
    const bool live = i < asm_n(p, a);
    const uint32_t bit = 1u << a;
    // A key of huge multiplicity (a satellite's minimizer: 10^5-10^6 occurrences) would queue that many atomics on one slot
    // (49 ms for a repeat-rich Gbp).  Two remedies: the bits only ever get cleared, so a (possibly stale) read that shows both
    // cleared proves there is nothing left to record; and runs of equal keys in neighbouring lanes (a satellite array: the same
    // minimizer every 171 bases, for kilobases) are served by the run's first lane -- one probe, and a run of two or more IS
    // "twice in this assembly".
    const uint64_t key = live ? p.hash[a][i] : 0ull;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t prev = ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(key >> 32), 1, 64) << 32) | (uint32_t)__shfl_up((int)(uint32_t)key, 1, 64);
    const bool prev_live = __shfl_up((int)live, 1, 64) != 0;
    const bool start = lane == 0 || !live || !prev_live || key != prev;
    const uint64_t starts = __ballot(start);
    const uint32_t leader = 63u - (uint32_t)__builtin_clzll(starts & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull)));
    const bool followed = lane < 63u && !((starts >> (lane + 1u)) & 1ull);  // (the lane behind belongs to this run)
    uint32_t s = 0;
    if (live && start) {
        s = ht_slot(tab, mask, cap, key);
        const uint32_t ns = __atomic_load_n(&tab[s].nseen, __ATOMIC_RELAXED), nd = __atomic_load_n(&tab[s].ndup, __ATOMIC_RELAXED);
        if ((ns & bit) || (nd & bit)) {
            const uint32_t old = atomicAnd(&tab[s].nseen, ~bit);
            if (!(old & bit) || followed) atomicAnd(&tab[s].ndup, ~bit);  // second occurrence in this assembly
        }
    }
    s = (uint32_t)__shfl((int)s, (int)leader, 64);
    if (live) p.slot[a][i] = s;
}

// flags of every minimizer + number of shared ones per block of 256 (cnt[b], super-counts per assembly at
// sup[sup_start(a)..): scan_kernels.h); k_vertices turns them into offsets
__host__ __device__ __forceinline__ uint32_t sup_start(const AsmSet &p, uint32_t a) { return ((p.bstart[a] >> SUP_SHIFT) + a) * SUP_STRIDE; }

__global__ __launch_bounds__(256) void k_flags(const AsmSet p, const Slot *__restrict__ tab, uint32_t *cnt, uint32_t *sup)
{
    const uint32_t a = asm_of_block(p, blockIdx.x);
    const uint32_t i = (blockIdx.x - p.bstart[a]) * 256u + threadIdx.x;
    bool sh = false;
    if (i < asm_n(p, a)) {
        const uint32_t bit = 1u << a, full = p.full;
        const Slot sl = tab[p.slot[a][i]];
        const uint32_t seen = ~sl.nseen & full, d = ~sl.ndup & full;
        const bool uniq = !(d & bit);
        const bool inall = seen == full;
        sh = inall && d == 0;
        p.flags[a][i] = (uint8_t)((uniq ? MXG_MX_UNIQUE : 0) | (sh ? MXG_MX_SHARED : 0) | (inall ? MXG_MX_INALL : 0));
    }
    const uint32_t c = (uint32_t)__syncthreads_count(sh ? 1 : 0);
    if (threadIdx.x == 0) count_publish(cnt + p.bstart[a], sup + sup_start(p, a), blockIdx.x - p.bstart[a], c);
}

// ---- the same join without far atomics: partition by hash, one LDS table per partition ---------------------------------
// k_insert spends its time in ~2 dependent device-scope atomics per minimizer on a table far larger than L2 (43 us for
// 4 x 10^5 keys).  Here every block of k_pj_bucket takes 4096 minimizers (of all assemblies, in the order of the
// concatenated 256-blocks), sorts them by a hash of their key into P partitions INSIDE ITS OWN 4096-record region
// (LDS histogram, LDS prefix, LDS cursors: no global atomics at all) and writes its row of partition offsets to M.
// One block of k_pj_join per partition then collects the partition's short segments from every region (column of M),
// builds the partition's table in LDS and sends every record's verdict word to the minimizer the record names
// (slot[a][i]), where k_flags_pj reads it in order.  The commonest verdict, "once in its assembly, not in every assembly"
// (a quarter of the records at 3 Gbp + 3 Gbp), is not sent: k_pj_bucket has written it for every minimizer, in order, beside
// its read of the hashes, and the join's scattered store -- 32 bytes of traffic per 4-byte word -- is kept for the words that
// differ (join_verdict.h).
// A partition with more distinct keys than its table holds reports failure through pinned host memory and build_graph
// redoes the stage with the global table.
// (PJ_IPB items per bucketing block, PJ_T slots per table, at most PJ_MAX_P partitions: join_plan.h)

__device__ __forceinline__ uint32_t pj_part(uint64_t key, uint32_t pmask)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 44) & pmask;  // (the slot inside the table uses bits 32..42)
}

// Runs of equal hashes in sketch order -- a tandem array leaves the same minimizer once per unit: tens of thousands of copies of
// one key in a satellite-rich genome, all in one partition, all for one block of k_pj_join -- go through the join as one
// record per wave they touch: the first of the run's minimizers among the wave's 64 (the leader), marked "more than once in
// its assembly" (PJ_REC_DUP in the record's assembly word).  The others (followers) are left out of the records; k_flags_pj
// gives them their verdict (not unique, not shared, in every assembly iff the leader's key is).  A run that crosses into the
// next wave starts again there: its parts meet in the join like any two records of one key.  Called by whole waves (lane = 64
// consecutive minimizers of one block).
constexpr uint32_t PJ_REC_DUP = 0x80000000u;
__device__ __forceinline__ uint32_t pj_run_role(uint32_t i, uint32_t n, uint64_t key, bool live)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t prev = __shfl_up(key, 1), next = __shfl_down(key, 1);
    const bool fol = live && lane > 0 && prev == key;
    const bool lead = live && !fol && lane < 63 && i + 1 < n && next == key;
    return (fol ? 1u : 0u) | (lead ? 2u : 0u);
}

constexpr uint32_t PJ_BT = 1024;   // threads of a bucketing block (4 items each): 16 waves hide the latency of its passes
__global__ __launch_bounds__(PJ_BT) void k_pj_bucket(const AsmSet p, uint32_t nb, uint32_t pmask, uint32_t *M, uint4 *recs,
                                                   uint32_t *sup, uint32_t n_sup)
{
    extern __shared__ uint32_t pj_lds[];
    uint32_t *hist = pj_lds, *start = pj_lds + pmask + 1;
    __shared__ uint32_t sh[256];
    if (blockIdx.x == 0)  // super-counts of the two counting kernels that follow (scan_kernels.h)
        for (uint32_t i = threadIdx.x; i < n_sup; i += PJ_BT) sup[i] = 0;
    constexpr uint32_t U = PJ_IPB / PJ_BT;  // items per thread: item u of thread t = 256-block u * BPU + t / 256, element t % 256
    constexpr uint32_t BPU = PJ_BT / 256;
    const uint32_t j = blockIdx.x, sub = threadIdx.x >> 8, t256 = threadIdx.x & 255u;
    // Almost every block lies inside one assembly: its table entries (scalar loads from the argument block, dependent
    // on one another) are then fetched once, not once per item.
    const uint32_t blk0 = j * (PJ_IPB / 256), a0 = asm_of_block(p, blk0), a1 = asm_of_block(p, min(blk0 + PJ_IPB / 256, nb) - 1u);
    const bool one = a0 == a1;
    const uint64_t *hp0 = p.hash[a0];
    uint32_t *sp0 = p.slot[a0];
    const uint32_t n0 = asm_n(p, a0), ib0 = (blk0 - p.bstart[a0]) * 256u;
    uint64_t key[U];
    uint32_t live = 0, dupm = 0;  // bit u: item u of this thread exists (and is no follower) / leads a run of equal hashes
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t blk = blk0 + u * BPU + sub;
        key[u] = 0;
        if (blk >= nb) continue;
        const uint64_t *hp = hp0;
        uint32_t *sp = sp0;
        uint32_t i = ib0 + (u * BPU + sub) * 256u + t256, n = n0;
        if (!one) {
            const uint32_t a = asm_of_block(p, blk);
            hp = p.hash[a];
            sp = p.slot[a];
            i = (blk - p.bstart[a]) * 256u + t256;
            n = asm_n(p, a);
        }
        const bool lv = i < n;
        if (lv) {
            key[u] = hp[i];
            sp[i] = PJ_VERDICT_PREFILL;  // (followers too; k_pj_join sends only the verdicts that differ)
        }
        const uint32_t role = pj_run_role(i, n, key[u], lv);
        const uint64_t fb = __ballot(role & 1u);
        if ((threadIdx.x & 63u) == 0) p.fol[(size_t)blk * 4u + ((threadIdx.x >> 6) & 3u)] = fb;
        if (lv && !(role & 1u)) live |= 1u << u;
        if (role & 2u) dupm |= 1u << u;
    }
    for (uint32_t b = threadIdx.x; b <= pmask; b += PJ_BT) hist[b] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < U; ++u)
        if ((live >> u) & 1u) atomicAdd(&hist[pj_part(key[u], pmask)], 1u);
    __syncthreads();
    // exclusive prefix of the block's histogram: thread t owns `per` consecutive partitions (none beyond P)
    const uint32_t P = pmask + 1, per = P >= PJ_BT ? P / PJ_BT : 1u, b0 = threadIdx.x * per;
    uint32_t c = 0;
    if (b0 < P)
        for (uint32_t u = 0; u < per; ++u) c += hist[b0 + u];
    uint32_t run = block_exclusive<PJ_BT / 64>(c, sh);
    uint32_t *row = M + (size_t)j * (P + 1);
    if (b0 < P)
        for (uint32_t u = 0; u < per; ++u) {
            const uint32_t cb = hist[b0 + u];
            start[b0 + u] = run;
            row[b0 + u] = run;
            hist[b0 + u] = 0;  // from here on: items already placed in that partition
            run += cb;
        }
    if (threadIdx.x == 0) row[P] = sh[255];
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        if (!((live >> u) & 1u)) continue;
        const uint32_t blk = blk0 + u * BPU + sub;
        uint32_t a = a0, i = ib0 + (u * BPU + sub) * 256u + t256;
        if (!one) {
            a = asm_of_block(p, blk);
            i = (blk - p.bstart[a]) * 256u + t256;
        }
        const uint32_t b = pj_part(key[u], pmask);
        const uint32_t pos = j * PJ_IPB + start[b] + atomicAdd(&hist[b], 1u);
        recs[pos] = make_uint4((uint32_t)key[u], (uint32_t)(key[u] >> 32), i, a | (((dupm >> u) & 1u) ? PJ_REC_DUP : 0u));  // (the record knows whose it is: k_pj_join
                                                                                    //  sends the verdict straight to slot[a][i])
    }
}

// slot of `key` in the partition's LDS table, inserting it if absent; PJ_T + 1: table full
__device__ __forceinline__ uint32_t pj_slot_from(unsigned long long *keys, uint64_t key, uint32_t s)
{
    if (key == HT_EMPTY) return PJ_T;
    for (uint32_t step = 0; step < PJ_T; ++step) {
        const unsigned long long cur = keys[s];
        if (cur == key) return s;
        if (cur == HT_EMPTY) {
            const unsigned long long old = atomicCAS(&keys[s], (unsigned long long)HT_EMPTY, (unsigned long long)key);
            if (old == HT_EMPTY || old == key) return s;
        }
        s = (s + 1u) & (PJ_T - 1u);
    }
    return PJ_T + 1u;
}
__device__ __forceinline__ uint32_t pj_slot(unsigned long long *keys, uint64_t key)
{
    return pj_slot_from(keys, key, (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & (PJ_T - 1u));
}

// The two-level join's records, 16 or 12 bytes (R12: join_plan.h, "the two-level join's 12-byte records"), as the kernels hold
// them: a uint4 whose fourth word is not there in the 12-byte form.  Record r of an array of 12-byte records: words 3 r .. 3 r + 2
// (one dwordx3 access, 4-byte aligned).
struct PjRec3 {
    uint32_t x, y, z;
};
template <bool R12>
__device__ __forceinline__ uint4 pj_rec_load(const uint4 *recs, size_t r)
{
    if (!R12) return recs[r];
    const PjRec3 v = reinterpret_cast<const PjRec3 *>(recs)[r];
    return make_uint4(v.x, v.y, v.z, 0u);
}
template <bool R12>
__device__ __forceinline__ void pj_rec_store(uint4 *recs, size_t r, const uint4 v)
{
    if (!R12) recs[r] = v;
    else reinterpret_cast<PjRec3 *>(recs)[r] = PjRec3{v.x, v.y, v.z};
}

// Two levels (more than PJ_MAX_P x 1280 minimizers): `cursor` != nullptr.  k_pj1_scatter has dealt the minimizers into P1 coarse
// partitions of capacity cap1 (coarse partition c holds cursor[c * PJ1_CS] records from c * cap1 on) and prefilled every
// minimizer's verdict word (PJ_VERDICT_PREFILL: the join sends only the verdicts that differ), k_pj2_bucket has sorted
// every 4096-record region of a coarse partition into P sub-partitions (rows of M: rows2 per coarse partition); block
// blockIdx.x = c * P + b joins sub-partition b of coarse partition c.
// (PJ1_CS words between the coarse partitions' cursors: join_plan.h)
// A coarse partition's cap1 records are ONE run that all assemblies fill through one cursor (n_sub = 1), or -- the fused call that
// partitions every assembly behind its own k_emit, while the others are still being sketched -- one 4096-aligned sub-range per
// assembly, [off, off + cap) of the partition, with a cursor per (coarse partition, assembly): level 2 of an assembly then sorts
// that assembly's rows only, and needs nothing of the others.  The rows of a partition stay its 4096-record pieces in order,
// whosever they are: the join walks them as before.  Cursor of (partition c, sub-range s): word (c * n_sub + s) * PJ1_CS.
struct PjSub {
    uint32_t n_sub, s, off, cap;
};
struct PjSubCaps {  // what the join asks the cursors: did a sub-range outgrow its capacity
    uint32_t n_sub;
    uint32_t cap[MXG_MAX_ASSEMBLIES];
};
// NARROW (at most 16 assemblies): the seen and dup masks share one word per slot (32 KB of LDS per block instead of 44)
template <bool NARROW>
__global__ __launch_bounds__(256) void k_pj_join(uint4 *recs, const uint32_t *__restrict__ M, uint32_t P, uint32_t n_rows,
                                                 uint64_t *host_fail, uint32_t force_fail, const uint32_t *__restrict__ cursor,
                                                 uint32_t cap1, uint32_t rows2, const AsmSet p, const PjSubCaps caps, uint32_t prefill0)
{
    const uint32_t full = p.full;
    __shared__ unsigned long long keys[PJ_T + 1];
    __shared__ uint32_t seen[PJ_T + 1], dup[NARROW ? 1 : PJ_T + 1];
    __shared__ uint32_t item0[PJ_T + 1];  // the key's minimizer in assembly 0 (what the others look their vertex up by)
    __shared__ uint32_t seg_off[257], seg_rec[256], sh[256];
    __shared__ uint32_t failed;
    uint32_t b = blockIdx.x, rec_off = 0;
    if (cursor) {
        const uint32_t c = blockIdx.x / P;
        b = blockIdx.x % P;
        // (sub-ranges: every row of the partition -- k_pj2_bucket leaves an empty row where a sub-range has no records)
        n_rows = caps.n_sub > 1 ? rows2 : (min(cursor[c * PJ1_CS], cap1) + PJ_IPB - 1) / PJ_IPB;
        M += (size_t)c * rows2 * (P + 1);
        rec_off = c * cap1;
        if (threadIdx.x == 0)
            for (uint32_t s = 0; s < caps.n_sub; ++s)
                if (cursor[(c * caps.n_sub + s) * PJ1_CS] > caps.cap[s]) *host_fail = 1;  // the coarse partition overflowed: global table
    }
    for (uint32_t s = threadIdx.x; s <= PJ_T; s += 256) {
        keys[s] = HT_EMPTY;
        seen[s] = 0;
        if (!NARROW) dup[s] = 0;
    }
    if (threadIdx.x == 0) failed = force_fail;
    // The partition's records are short segments, one per region.  Per 256 regions: every thread fetches one segment's
    // bounds, a block scan lays the segments end to end, and the records are dealt out to the threads one by one (binary
    // search in the scan): all loads of a pass are independent.  Pass 0 inserts, pass 1 writes the table state back; with
    // at most 256 regions (10^6 minimizers) pass 1 reuses the layout and the slots of the first QC records per thread.
    constexpr uint32_t QC = 4;
    uint32_t rc[QC], sc[QC], ac[QC], ic[QC];
    const bool single = n_rows <= 256;
    for (uint32_t pass = 0; pass < 2; ++pass) {
        const bool bad = pass == 1 && failed != 0;  // report, and make every key of this partition "seen nowhere"
        if (bad && threadIdx.x == 0) *host_fail = 1;
        for (uint32_t j0 = 0; j0 < n_rows; j0 += 256) {
            if (pass == 0 || !single) {
                const uint32_t j = j0 + threadIdx.x;
                uint32_t lo = 0, len = 0;
                if (j < n_rows) {
                    const uint32_t *row = M + (size_t)j * (P + 1);
                    lo = row[b];
                    len = row[b + 1] - lo;
                }
                const uint32_t off = block_exclusive_256(len, sh);
                seg_off[threadIdx.x] = off;
                seg_rec[threadIdx.x] = rec_off + j * PJ_IPB + lo;
                __syncthreads();
            }
            const uint32_t total = sh[255];
            auto locate = [&](uint32_t q) {  // record number q of the laid-out segments
                uint32_t l = 0, h = 256;     // last segment with seg_off <= q (empty segments share offsets: take the last)
                while (h - l > 1) {
                    const uint32_t m = (l + h) >> 1;
                    if (seg_off[m] <= q) l = m; else h = m;
                }
                return seg_rec[l] + (q - seg_off[l]);
            };
            uint32_t last_a = 0, last_i = 0;  // assembly / item of the record insert() looked at last
            auto insert_rec = [&](const uint4 rec) {   // pass 0; also the lookup of pass 1
                last_a = rec.w & ~PJ_REC_DUP;
                last_i = rec.z;
                const uint32_t s = pj_slot(keys, ((uint64_t)rec.y << 32) | rec.x);
                if (pass == 0) {
                    const uint32_t bit = 1u << last_a;
                    if (s > PJ_T) failed = 1;
                    else {
                        // (a key of huge multiplicity -- a satellite's minimizer -- brings tens of thousands of records to one
                        // slot: once its state says "seen twice here" there is nothing left to record, and no atomic to queue for)
                        const uint32_t cur = seen[s], dcur = NARROW ? cur >> 16 : dup[s];
                        if (!((cur & bit) && (dcur & bit))) {
                            if (rec.w & PJ_REC_DUP) {  // the leader of a run of equal hashes: its followers are not among the records
                                if (NARROW) atomicOr(&seen[s], bit | (bit << 16));
                                else {
                                    atomicOr(&seen[s], bit);
                                    atomicOr(&dup[s], bit);
                                }
                            } else if (atomicOr(&seen[s], bit) & bit) {  // second occurrence in this assembly
                                if (NARROW) atomicOr(&seen[s], bit << 16); else atomicOr(&dup[s], bit);
                            }
                            if (last_a == 0) item0[s] = rec.z;  // (a key that occurs twice in assembly 0 is not shared: never read)
                        }
                    }
                }
                return s;
            };
            auto insert = [&](uint32_t r) { return insert_rec(recs[r]); };
            // the verdict of a record, 4 bytes: (shared: the key's minimizer in assembly 0) << 3 | MXG_MX_* flags, sent straight
            // to the minimizer it stands for (slot[a][i]: the ONE random access per minimizer of the whole join; k_flags_pj
            // then reads the verdicts in order)
            auto finish = [&](uint32_t i, uint32_t s, uint32_t a) {
                uint32_t fl = 0;
                if (!bad) {
                    const uint32_t sn = seen[s] & full, d = (NARROW ? seen[s] >> 16 : dup[s]) & full;
                    const bool inall = sn == full;
                    fl = (!(d & (1u << a)) ? MXG_MX_UNIQUE : 0u) | ((inall && d == 0) ? MXG_MX_SHARED : 0u) | (inall ? MXG_MX_INALL : 0u);
                }
                const uint32_t word = ((fl & MXG_MX_SHARED) ? item0[s] << 3 : 0u) | fl;
                if (word != pj_verdict_prefill(prefill0, a, i)) p.slot[a][i] = word;
            };
#pragma unroll
            for (uint32_t it = 0; it < QC; ++it) {
                const uint32_t q = threadIdx.x + it * 256u;
                if (q >= total) break;
                if (pass == 0) {
                    rc[it] = locate(q);
                    sc[it] = insert(rc[it]);
                    ac[it] = last_a;
                    ic[it] = last_i;
                } else if (single) {
                    finish(ic[it], sc[it], ac[it]);
                } else {
                    const uint32_t r = locate(q);
                    const uint32_t s = insert(r);  // (also reads the record's assembly and item)
                    finish(last_i, s, last_a);
                }
            }
            // beyond QC records per thread (a partition that holds a key of huge multiplicity: hundreds of thousands of records
            // for this one block): eight records per thread are requested before the first is looked at -- one record per
            // iteration made the block wait a memory round trip 1 000 times over (5.7 ms on a repeat-rich 0.3 Gbp genome)
            constexpr uint32_t TU = 8;
            for (uint32_t q0 = threadIdx.x + QC * 256u; q0 < total; q0 += 256u * TU) {
                uint4 rv[TU];
#pragma unroll
                for (uint32_t u = 0; u < TU; ++u) {
                    const uint32_t q = q0 + u * 256u;
                    rv[u] = q < total ? recs[locate(q)] : make_uint4(0u, 0u, 0u, 0u);
                }
#pragma unroll
                for (uint32_t u = 0; u < TU; ++u) {
                    if (q0 + u * 256u >= total) break;
                    const uint32_t s = insert_rec(rv[u]);
                    if (pass == 1) finish(last_i, s, last_a);
                }
            }
            __syncthreads();
        }
    }
}


// The two-level join's partitions by PERSISTENT blocks, three partitions in flight per block: while the records of partition k
// are inserted and judged, the records of partition k + 1 are on their way (requested as soon as its segments were laid out) and
// so are the segment bounds of partition k + 2 -- a block of k_pj_join spends most of its ~16 us waiting for exactly these two
// round trips, one behind the other, and the tables' 32 KB keep more blocks from hiding them.  For partitions of at most 256
// regions (rows2; always, unless a skewed coarse partition was re-sized); same tables, same verdicts as k_pj_join.
// Where a record lies: the thread that owns a region writes the region's number over the records of its segment (seg_of, the
// first QC * 256 records of the partition), so a record finds its segment with one LDS read; only the records beyond
// those (a key of huge multiplicity) are still located by a search in seg_off, as in k_pj_join.
// R12: 12-byte records {product lo, product hi with the tag, item}; the table keeps the product without its tag.
template <bool NARROW, bool R12>
__global__ __launch_bounds__(256) void k_pj_join_pipe(uint4 *recs, const uint32_t *__restrict__ M, uint32_t P, uint32_t n_parts,
                                                      uint64_t *host_fail, uint32_t force_fail, const uint32_t *__restrict__ cursor,
                                                      uint32_t cap1, uint32_t rows2, const AsmSet p, const PjSubCaps caps, uint32_t prefill0)
{
    const uint32_t full = p.full;
    const uint32_t lgP = R12 ? 31u - (uint32_t)__clz(P) : 0u, tag_mask = R12 ? pj12_tag_mask(lgP) : 0u;
    auto rec_a = [&](const uint4 rec) { return R12 ? pj12_unpack_tag(rec.y, lgP) & (PJ12_TAG_DUP - 1u) : rec.w & ~PJ_REC_DUP; };
    auto rec_dup = [&](const uint4 rec) { return R12 ? (pj12_unpack_tag(rec.y, lgP) & PJ12_TAG_DUP) != 0 : (rec.w & PJ_REC_DUP) != 0; };
    auto rec_slot = [&](unsigned long long *tab, const uint4 rec) {
        if (R12) return pj_slot_from(tab, ((uint64_t)(rec.y & ~tag_mask) << 32) | rec.x, rec.y & (PJ_T - 1u));
        return pj_slot(tab, ((uint64_t)rec.y << 32) | rec.x);
    };
    __shared__ unsigned long long keys[PJ_T + 1];
    __shared__ uint32_t seen[PJ_T + 1], dup[NARROW ? 1 : PJ_T + 1];
    __shared__ uint32_t item0[PJ_T + 1];
    __shared__ uint32_t seg_off[2][257], seg_rec[2][256], sh[256];
    __shared__ uint32_t failed;
    constexpr uint32_t QC = 4;
    __shared__ uint8_t seg_of[QC * 256];  // the region whose segment holds record q of the partition laid out last, q < QC * 256
    uint4 rn[QC];                    // the first QC records per thread of the partition whose segments were laid out last
    uint32_t tot_n = 0;              // ... and how many records it has
    uint32_t lo_nn = 0, len_nn = 0;  // segment of this thread's region in the partition after that one
    auto bounds = [&](uint32_t part, uint32_t &lo, uint32_t &len) {  // (requests only: nothing waits here)
        lo = len = 0;
        if (part < n_parts && threadIdx.x < rows2) {
            const uint32_t c = part / P, b = part % P;
            const uint32_t *row = M + ((size_t)c * rows2 + threadIdx.x) * (P + 1);
            lo = row[b];
            len = row[b + 1];  // (the end: the length is taken where the values are used)
        }
    };
    auto lay_out = [&](uint32_t part, uint32_t buf, uint32_t lo, uint32_t end) {  // segments end to end; first records requested
        const uint32_t c = part < n_parts ? part / P : 0u;
        const uint32_t len = end - lo;
        const uint32_t off = block_exclusive_256(len, sh);
        seg_off[buf][threadIdx.x] = off;
        seg_rec[buf][threadIdx.x] = c * cap1 + threadIdx.x * PJ_IPB + lo;
        // the thread that owns a region names it to the records of its segment (about a dozen consecutive ones): each of the
        // first QC records per thread then finds its segment with one LDS read where a search in seg_off took eight in a row
        for (uint32_t q = off, e = min(off + len, QC * 256u); q < e; ++q) seg_of[q] = (uint8_t)threadIdx.x;
        const uint32_t total = sh[255];
        __syncthreads();
#pragma unroll
        for (uint32_t it = 0; it < QC; ++it) {
            const uint32_t q = threadIdx.x + it * 256u;
            rn[it] = make_uint4(0u, 0u, 0u, 0u);
            if (q < total) {
                const uint32_t l = seg_of[q];
                rn[it] = pj_rec_load<R12>(recs, seg_rec[buf][l] + (q - seg_off[buf][l]));
            }
        }
        return total;
    };
    const uint32_t first = blockIdx.x, stride = gridDim.x;
    {
        uint32_t lo, end;
        bounds(first, lo, end);
        bounds(first + stride, lo_nn, len_nn);
        tot_n = lay_out(first, 0u, lo, end);
    }
    uint32_t k = 0;
    for (uint32_t part = first; part < n_parts; part += stride, ++k) {
        // this partition's records are in rn (requested one iteration ago); move on the two prefetches
        uint4 rc[QC];
#pragma unroll
        for (uint32_t it = 0; it < QC; ++it) rc[it] = rn[it];
        const uint32_t total = tot_n, buf = k & 1u;
        {
            const uint32_t lo = lo_nn, end = len_nn;
            bounds(part + 2u * stride, lo_nn, len_nn);
            tot_n = lay_out(part + stride, buf ^ 1u, lo, end);  // (a partition beyond the last: no segments, no requests)
        }
        for (uint32_t s = threadIdx.x; s <= PJ_T; s += 256) {
            keys[s] = HT_EMPTY;
            seen[s] = 0;
            if (!NARROW) dup[s] = 0;
        }
        if (threadIdx.x == 0) {
            failed = force_fail;
            const uint32_t c = part / P;
            if (part % P == 0)
                for (uint32_t s = 0; s < caps.n_sub; ++s)
                    if (cursor[(c * caps.n_sub + s) * PJ1_CS] > caps.cap[s]) *host_fail = 1;  // the coarse partition overflowed: global table
        }
        __syncthreads();
        auto locate = [&](uint32_t q) {
            uint32_t l = 0, h = 256;
            while (h - l > 1) {
                const uint32_t m = (l + h) >> 1;
                if (seg_off[buf][m] <= q) l = m; else h = m;
            }
            return seg_rec[buf][l] + (q - seg_off[buf][l]);
        };
        auto insert_rec = [&](const uint4 rec, bool record) {
            const uint32_t a = rec_a(rec);
            const uint32_t s = rec_slot(keys, rec);
            if (record) {
                const uint32_t bit = 1u << a;
                if (s > PJ_T) failed = 1;
                else {
                    const uint32_t cur = seen[s], dcur = NARROW ? cur >> 16 : dup[s];
                    if (!((cur & bit) && (dcur & bit))) {
                        if (rec_dup(rec)) {
                            if (NARROW) atomicOr(&seen[s], bit | (bit << 16));
                            else {
                                atomicOr(&seen[s], bit);
                                atomicOr(&dup[s], bit);
                            }
                        } else if (atomicOr(&seen[s], bit) & bit) {
                            if (NARROW) atomicOr(&seen[s], bit << 16); else atomicOr(&dup[s], bit);
                        }
                        if (a == 0) item0[s] = rec.z;
                    }
                }
            }
            return s;
        };
        uint32_t sc[QC];
#pragma unroll
        for (uint32_t it = 0; it < QC; ++it)
            if (threadIdx.x + it * 256u < total) sc[it] = insert_rec(rc[it], true);
        constexpr uint32_t TU = 8;
        for (uint32_t q0 = threadIdx.x + QC * 256u; q0 < total; q0 += 256u * TU) {  // (a key of huge multiplicity: see k_pj_join)
            uint4 rv[TU];
#pragma unroll
            for (uint32_t u = 0; u < TU; ++u) {
                const uint32_t q = q0 + u * 256u;
                rv[u] = q < total ? pj_rec_load<R12>(recs, locate(q)) : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (uint32_t u = 0; u < TU; ++u)
                if (q0 + u * 256u < total) insert_rec(rv[u], true);
        }
        __syncthreads();
        const bool bad = failed != 0;
        if (bad && threadIdx.x == 0) *host_fail = 1;
        auto finish = [&](const uint4 rec, uint32_t s) {
            const uint32_t a = rec_a(rec);
            uint32_t fl = 0;
            if (!bad) {
                const uint32_t sn = seen[s] & full, d = (NARROW ? seen[s] >> 16 : dup[s]) & full;
                const bool inall = sn == full;
                fl = (!(d & (1u << a)) ? MXG_MX_UNIQUE : 0u) | ((inall && d == 0) ? MXG_MX_SHARED : 0u) | (inall ? MXG_MX_INALL : 0u);
            }
            const uint32_t word = ((fl & MXG_MX_SHARED) ? item0[s] << 3 : 0u) | fl;
            if (word != pj_verdict_prefill(prefill0, a, rec.z)) p.slot[a][rec.z] = word;
        };
#pragma unroll
        for (uint32_t it = 0; it < QC; ++it)
            if (threadIdx.x + it * 256u < total) finish(rc[it], bad ? 0u : sc[it]);
        for (uint32_t q0 = threadIdx.x + QC * 256u; q0 < total; q0 += 256u * TU) {
            uint4 rv[TU];
#pragma unroll
            for (uint32_t u = 0; u < TU; ++u) {
                const uint32_t q = q0 + u * 256u;
                rv[u] = q < total ? pj_rec_load<R12>(recs, locate(q)) : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (uint32_t u = 0; u < TU; ++u)
                if (q0 + u * 256u < total) finish(rv[u], bad ? 0u : insert_rec(rv[u], false));
        }
        __syncthreads();  // the table is cleared for the next partition
    }
}

// level 1 of the two-level join: 4096 minimizers per block (the same item order as k_pj_bucket), LDS histogram over P1
// coarse partitions (hash bits 52..63), ONE device-scope add per non-empty (block, partition) bin reserves the bin's place
// in the partition (4096 / P1 records per add; the cursors sit on their own lines), then the records are dealt out.
// The launch covers 256-blocks [blk_lo, blk_hi) of the concatenated assemblies: all of them, or (sub.n_sub > 1) those of assembly
// sub.s, whose records go to its own sub-range of every coarse partition.
__device__ __forceinline__ uint32_t pj1_part(uint64_t key, uint32_t p1mask) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 52) & p1mask; }

// R12 (sub-ranges per assembly only): 12-byte records {product lo, product hi, item | PJ12_ITEM_DUP}; key[] then holds the products.
// prefill0: the verdict prefill of assembly 0 (join_verdict.h).
// G: thread block j takes tiles j G .. j G + G - 1 of the launch (the same 256-blocks in the same order as <1>: tile g of the
// block is 256-blocks blk0 + 16 g ..) and a thread keeps 4 G records.  All G tiles' hashes are requested before the first is used;
// the ordered work (prefill, fol ballots) follows per tile as before; there is ONE histogram over the G tiles and ONE add per
// coarse bin and thread block -- G times fewer adds to every cursor -- and a bin's records of all G tiles share its place.
// On the 12-byte route a record's assembly is the sub-range's and its index follows from where it was read, so a thread carries
// the product and two mask bits per record.  G by the launch's tile count: pj1_tiles (join_plan.h, with what was measured:
// one tile at every size; MXG_PJ_TILES=2 forces two on the 12-byte route, the A/B of that finding).
template <bool R12, uint32_t G>
__global__ __launch_bounds__(PJ_BT) void k_pj1_scatter(const AsmSet p, uint32_t blk_lo, uint32_t blk_hi, uint32_t p1mask, uint32_t cap1,
                                                     uint32_t *cursor, uint4 *recs1, uint32_t *sup, uint32_t n_sup, const PjSub subr,
                                                     uint32_t prefill0)
{
    auto part1 = [&](uint64_t k) { return R12 ? (uint32_t)(k >> 52) & p1mask : pj1_part(k, p1mask); };
    extern __shared__ uint32_t pj_lds[];
    uint32_t *hist = pj_lds, *start = pj_lds + p1mask + 1;
    if (blockIdx.x == 0)  // super-counts of the two counting kernels that follow (scan_kernels.h)
        for (uint32_t i = threadIdx.x; i < n_sup; i += PJ_BT) sup[i] = 0;
    constexpr uint32_t U = PJ_IPB / PJ_BT, BPU = PJ_BT / 256, NU = U * G;
    const uint32_t j = blockIdx.x;
    const uint32_t blk0 = blk_lo + j * (G * (PJ_IPB / 256));
    // record u of thread t: item u % U of tile u / U, element t % 256 of its 256-block
    auto blk_of = [&](uint32_t u, uint32_t t) { return blk0 + (u / U) * (PJ_IPB / 256) + (u % U) * BPU + (t >> 8); };
    // Each pass over the records works their 256-blocks and indices out anew from a copy of the thread's number that the compiler
    // cannot see through: it would otherwise keep every record's block, index and predicates from the first pass to the last,
    // five registers per record where the record itself is two.
    auto thread_again = [] {
        uint32_t t = threadIdx.x;
        asm volatile("" : "+v"(t));
        return t;
    };
    const bool own = R12 || subr.n_sub > 1;  // the launch is one assembly's (sub-ranges; the 12-byte route has them)
    const uint32_t bs_own = p.bstart[subr.s], n_own = own ? asm_n(p, subr.s) : 0u;
    // (the records' arrays are written by plain assignments and selects, never under a branch: a conditional store into one of
    // them makes the compiler carry the whole array through the join, 4 G records of copies per record)
    uint64_t key[NU];
    uint32_t ia[R12 ? 1 : NU], ii[R12 ? 1 : NU], live = 0, dupm = 0;
    const uint32_t t_a = thread_again();
#pragma unroll
    for (uint32_t u = 0; u < NU; ++u) {  // every tile's loads, before the first is used
        const uint32_t blk = blk_of(u, t_a), in = blk < blk_hi, t256 = t_a & 255u;
        const uint32_t a = own ? subr.s : asm_of_block(p, min(blk, blk_hi - 1u));
        const uint32_t i = (blk - (own ? bs_own : p.bstart[a])) * 256u + t256, n = own ? n_own : asm_n(p, a);
        const bool lv = in && i < n;
        key[u] = p.hash[a][lv ? i : 0u];  // (a minimizer that is not there reads the first, which the launch has, and drops it below)
        if (lv) p.slot[a][i] = pj_verdict_prefill(prefill0, a, i);  // (followers too; in front of this thread's own store of 0 below)
    }
    const uint32_t t_b = thread_again();
#pragma unroll
    for (uint32_t u = 0; u < NU; ++u) {
        const uint32_t blk = blk_of(u, t_b), in = blk < blk_hi, t256 = t_b & 255u;
        const uint32_t a = own ? subr.s : asm_of_block(p, min(blk, blk_hi - 1u));
        const uint32_t i = (blk - (own ? bs_own : p.bstart[a])) * 256u + t256, n = own ? n_own : asm_n(p, a);
        const bool lv = in && i < n;
        const uint32_t role = pj_run_role(i, n, key[u], lv);  // (followers travel with their run's leader)
        const uint64_t fb = __ballot(role & 1u);
        if (in && (threadIdx.x & 63u) == 0) p.fol[(size_t)blk * 4u + ((threadIdx.x >> 6) & 3u)] = fb;
        if (R12) key[u] *= PJ_MUL;
        const bool rec = lv && !(role & 1u);
        if (!R12) {
            ia[u] = rec ? a | ((role & 2u) ? PJ_REC_DUP : 0u) : 0u;
            ii[u] = rec ? i : 0u;
        }
        dupm |= rec && (role & 2u) ? 1u << u : 0u;
        live |= rec ? 1u << u : 0u;
    }
    // (here, not where they are next read: the compiler would otherwise put off the run test and the product of every record to
    // the last pass and keep the hash, its neighbour's and the index until then)
    asm volatile("" : "+v"(live), "+v"(dupm));
#pragma unroll
    for (uint32_t u = 0; u < NU; ++u) asm volatile("" : "+v"(key[u]));
    for (uint32_t b = threadIdx.x; b <= p1mask; b += PJ_BT) hist[b] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < NU; ++u)
        if ((live >> u) & 1u) atomicAdd(&hist[part1(key[u])], 1u);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b <= p1mask; b += PJ_BT) {
        const uint32_t c = hist[b];
        start[b] = c ? atomicAdd(&cursor[(b * subr.n_sub + subr.s) * PJ1_CS], c) : 0u;
        hist[b] = 0;  // from here on: records of this bin already placed
    }
    __syncthreads();
    const uint32_t t_c = thread_again();
#pragma unroll
    for (uint32_t u = 0; u < NU; ++u) {
        if (!((live >> u) & 1u)) continue;
        const uint32_t b = part1(key[u]);
        const uint32_t pos = start[b] + atomicAdd(&hist[b], 1u);
        // (12 bytes: the item is where its hash was read, the assembly the sub-range's, the mark a bit of dupm)
        const uint32_t i = R12 ? (blk_of(u, t_c) - bs_own) * 256u + (t_c & 255u) : ii[u], aw = R12 ? subr.s : ia[u];
        if (pos < subr.cap)
            pj_rec_store<R12>(recs1, (size_t)b * cap1 + subr.off + pos,
                              make_uint4((uint32_t)key[u], (uint32_t)(key[u] >> 32), R12 && ((dupm >> u) & 1u) ? i | PJ12_ITEM_DUP : i, aw));
        else p.slot[aw & ~PJ_REC_DUP][i] = 0;  // beyond the capacity: no verdict will come (the cursor says so, k_pj_join reports it and
                                        // the host redoes the stage with the global table); leave a harmless one behind
    }
}

// level 2: block (j, c) sorts records [j * 4096, (j + 1) * 4096) of coarse partition c by sub-partition (hash bits 44..) inside
// their region of recs2, writes its row of M and tells every minimizer where its record went (slot[a][i], read by k_flags_pj)
//
// A coarse partition that holds far more records than the mean (skew_lim) holds a key of huge multiplicity (hash partitions of
// distinct keys differ by a fraction of a percent): a satellite's minimizer whose copies are not neighbours in sketch order
// (those travel as one record already, pj_run_role), 10^5 records that would all meet in ONE block of k_pj_join.  The blocks of
// such a partition first collapse what is equal among their 4096 records: records of one (key, assembly) elect one of them,
// which goes on marked PJ_REC_DUP; the others leave a reference to it as their verdict (PJ_VERDICT_REF, followed by k_flags_pj)
// and drop out.
// (PJ_VERDICT_REF, the low bits of a verdict word that is no verdict: join_verdict.h)
// R12: reads level 1's 12-byte records (the assembly is the sub-range's, x and y hold the product), writes {product lo, product
// hi with the tag in implied bits, item}
template <bool R12>
__global__ __launch_bounds__(PJ_BT) void k_pj2_bucket(const AsmSet p, const uint4 *__restrict__ recs1, const uint32_t *__restrict__ cursor,
                                                    uint32_t cap1, uint32_t rows2, uint32_t pmask, uint32_t *M, uint4 *recs2,
                                                    uint32_t skew_lim, const PjSub subr)
{
    extern __shared__ uint32_t pj_lds[];
    uint32_t *hist = pj_lds, *start = pj_lds + pmask + 1;
    __shared__ uint32_t sh[256];
    const uint32_t j = blockIdx.x, c = blockIdx.y;
    const uint32_t lgP = R12 ? 31u - (uint32_t)__clz(pmask + 1u) : 0u;
    auto part2 = [&](const uint4 r) { return R12 ? (r.y >> PJ12_FINE_SHIFT) & pmask : pj_part(((uint64_t)r.y << 32) | r.x, pmask); };
    // (the launch sorts the rows of ONE sub-range of every coarse partition: j counts from the sub-range's first row)
    const uint32_t n_all = cursor[(c * subr.n_sub + subr.s) * PJ1_CS], n_c = min(n_all, subr.cap);
    const uint32_t row_j = subr.off / PJ_IPB + j;
    if (j * PJ_IPB >= n_c) {  // (block-uniform) nothing of this coarse partition in this region: an empty row (k_pj_join_pipe
        uint32_t *row = M + ((size_t)c * rows2 + row_j) * (pmask + 2);  // reads every row of the partition without asking the cursor)
        for (uint32_t b = threadIdx.x; b <= pmask + 1; b += PJ_BT) row[b] = 0;
        return;
    }
    constexpr uint32_t U = PJ_IPB / PJ_BT;
    const size_t base = (size_t)c * cap1 + subr.off + (size_t)j * PJ_IPB;
    uint4 rec[U];
    uint32_t live = 0;
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t q = u * PJ_BT + threadIdx.x;
        rec[u] = make_uint4(0u, 0u, 0u, 0u);
        if (j * PJ_IPB + q < n_c) {
            rec[u] = pj_rec_load<R12>(recs1, base + q);
            if (R12) {
                rec[u].w = subr.s | ((rec[u].z & PJ12_ITEM_DUP) ? PJ_REC_DUP : 0u);
                rec[u].z &= ~PJ12_ITEM_DUP;
            }
            live |= 1u << u;
        }
    }
    if (n_all > skew_lim) {  // (block-uniform)
        __shared__ unsigned long long skey[PJ_IPB];
        __shared__ uint32_t sitem[PJ_IPB];
        __shared__ uint8_t sasm[PJ_IPB];
        __shared__ uint32_t stab[PJ_IPB];      // 2 x 4096 slots of 16 bits: the record number of the slot's (key, assembly)
        __shared__ uint32_t sdup[PJ_IPB / 32];
        for (uint32_t q = threadIdx.x; q < PJ_IPB; q += PJ_BT) stab[q] = 0xFFFFFFFFu;
        for (uint32_t q = threadIdx.x; q < PJ_IPB / 32; q += PJ_BT) sdup[q] = 0;
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t q = u * PJ_BT + threadIdx.x;
            skey[q] = ((unsigned long long)rec[u].y << 32) | rec[u].x;
            sitem[q] = rec[u].z;
            sasm[q] = (uint8_t)(rec[u].w & 0xFFu);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            if (!((live >> u) & 1u)) continue;
            const uint32_t q = u * PJ_BT + threadIdx.x;
            const unsigned long long key = skey[q];
            const uint32_t a = rec[u].w & 0xFFu;
            uint32_t hsl = (uint32_t)(((key + a) * 0x9E3779B97F4A7C15ull) >> 40) & (2u * PJ_IPB - 1u);
            uint32_t rep = q;
            for (;;) {
                const uint32_t sft = (hsl & 1u) * 16u;
                const uint32_t word = stab[hsl >> 1], cur = (word >> sft) & 0xFFFFu;
                if (cur == 0xFFFFu) {
                    const uint32_t want = (word & ~(0xFFFFu << sft)) | (q << sft);
                    if (atomicCAS(&stab[hsl >> 1], word, want) == word) break;  // this record stands for its (key, assembly)
                    continue;                                                    // (the word changed: look again)
                }
                if (skey[cur] == key && sasm[cur] == a) {
                    rep = cur;
                    break;
                }
                hsl = (hsl + 1u) & (2u * PJ_IPB - 1u);
            }
            if (rep != q) {
                atomicOr(&sdup[rep >> 5], 1u << (rep & 31u));
                p.slot[a][rec[u].z] = (sitem[rep] << 3) | PJ_VERDICT_REF;
                live &= ~(1u << u);
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t q = u * PJ_BT + threadIdx.x;
            if ((sdup[q >> 5] >> (q & 31u)) & 1u) rec[u].w |= PJ_REC_DUP;
        }
    }
    for (uint32_t b = threadIdx.x; b <= pmask; b += PJ_BT) hist[b] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < U; ++u)
        if ((live >> u) & 1u) atomicAdd(&hist[part2(rec[u])], 1u);
    __syncthreads();
    const uint32_t P = pmask + 1, per = P >= PJ_BT ? P / PJ_BT : 1u, b0 = threadIdx.x * per;
    uint32_t cn = 0;
    if (b0 < P)
        for (uint32_t u = 0; u < per; ++u) cn += hist[b0 + u];
    uint32_t run = block_exclusive<PJ_BT / 64>(cn, sh);
    uint32_t *row = M + ((size_t)c * rows2 + row_j) * (P + 1);
    if (b0 < P)
        for (uint32_t u = 0; u < per; ++u) {
            const uint32_t cb = hist[b0 + u];
            start[b0 + u] = run;
            row[b0 + u] = run;
            hist[b0 + u] = 0;
            run += cb;
        }
    if (threadIdx.x == 0) row[P] = sh[255];
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        if (!((live >> u) & 1u)) continue;
        const uint32_t b = part2(rec[u]);
        const uint32_t pos = (uint32_t)base + start[b] + atomicAdd(&hist[b], 1u);
        if (R12) rec[u].y = pj12_pack(rec[u].y, lgP, pj12_tag(rec[u].w & ~PJ_REC_DUP, (rec[u].w & PJ_REC_DUP) != 0));
        pj_rec_store<R12>(recs2, pos, rec[u]);
    }
}

// ---- the tail's ordered passes: U consecutive 256-blocks per thread block ---------------------------------------------------
// k_flags_pj, k_vertices_pj, k_adjacency, k_edge_flags and k_edges (and the rank route's k_edge_flags_rank, k_edges_rank, which run
// without k_adjacency) are plain ordered passes, one item per thread.  With one 256-block
// per thread block a CU has 8 KB of loads in flight where an HBM round trip wants tens of KB, and every 256 items pay a block's
// bookkeeping ("The tail's ordered passes").  Thread block j of <U> takes 256-blocks j U .. j U + U - 1
// ("sub-blocks"); thread t keeps item t of each, so a wave still holds 64 consecutive items and the ballots, fol and mask0 words
// and the per-256 counts are what they were.  Every sub-block's loads are requested before the first is used, the dependent
// gathers follow for all U together, and the bookkeeping of sub-block u -- its count_prefix, its count_publish, the "last tile
// reports the total" duty -- is done by wave u (U <= 4 = waves per block).  U by size: graph_tail_u (join_plan.h), MXG_GRAPH_U
// forces it.  The global-table route's own passes (k_flags, k_vertices) stay at one 256-block per thread block.
//
// Ordered ranks of 0/1 flags inside the U sub-blocks with ONE barrier: a wave's ranks are a ballot and a popcount, the four wave
// totals per sub-block go through LDS beside whatever else the caller publishes in front of the same barrier.
template <uint32_t U>
struct TailScan {
    uint32_t tot[U][4];   // flags set per (sub-block, wave)
    uint32_t before[U];   // what precedes the sub-block (count_prefix by wave u)
};
template <uint32_t U>
__device__ __forceinline__ void tail_ballot(TailScan<U> &ts, uint32_t u, bool f, uint64_t &bm)
{
    bm = __ballot(f);
    if ((threadIdx.x & 63u) == 0) ts.tot[u][threadIdx.x >> 6] = (uint32_t)__popcll(bm);
}
// (behind the barrier) rank of this thread's flag of sub-block u among the sub-block's set flags
template <uint32_t U>
__device__ __forceinline__ uint32_t tail_rank(const TailScan<U> &ts, uint32_t u, uint64_t bm)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t r = (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
#pragma unroll
    for (uint32_t q = 0; q < 3; ++q) r += q < wv ? ts.tot[u][q] : 0u;
    return r;
}
template <uint32_t U>
__device__ __forceinline__ uint32_t tail_total(const TailScan<U> &ts, uint32_t u)
{
    return ts.tot[u][0] + ts.tot[u][1] + ts.tot[u][2] + ts.tot[u][3];
}

// The assemblies of a thread block's U sub-blocks [blk0, blk0 + U) of the concatenated 256-blocks: almost always one (its table
// entries -- scalar loads from the argument block, dependent on one another -- are then fetched once, as in k_pj_bucket).
// (The passes request their loads without branches around them -- an item that does not exist reads element 0 of an array that
// does, and drops it -- so that the U sub-blocks' requests stay one run of instructions: behind a branch per sub-block the
// compiler waits for each sub-block's flag before it requests the next one's.)
struct TailAsm {
    uint32_t a, n, b0;  // assembly, its minimizers, its first 256-block
};
__device__ __forceinline__ TailAsm tail_asm(const AsmSet &p, uint32_t a)
{
    return TailAsm{a, asm_n(p, a), p.bstart[a]};
}
template <uint32_t U>
__device__ __forceinline__ bool tail_asms(const AsmSet &p, uint32_t blk0, uint32_t nb, TailAsm (&t)[U])
{
    const uint32_t a_first = asm_of_block(p, blk0), a_last = U > 1 ? asm_of_block(p, min(blk0 + U, nb) - 1u) : a_first;
    t[0] = tail_asm(p, a_first);
#pragma unroll
    for (uint32_t u = 1; u < U; ++u) t[u] = t[0];
    if (a_first != a_last) {
#pragma unroll
        for (uint32_t u = 1; u < U; ++u)
            if (blk0 + u < nb) t[u] = tail_asm(p, asm_of_block(p, blk0 + u));
    }
    return a_first == a_last;
}

// k_flags for the partitioned join: the verdict of minimizer i sits in slot[a][i]
// mask0[w]: which of minimizers 64 w .. 64 w + 63 of assembly 0 are shared (k_vertices_pj ranks by it)
template <uint32_t U>
__global__ __launch_bounds__(256) void k_flags_pj(const AsmSet p, uint32_t nb, uint32_t *cnt, uint32_t *sup, uint64_t *mask0)
{
    __shared__ TailScan<U> ts;
    const uint32_t blk0 = blockIdx.x * U, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    TailAsm t[U];
    tail_asms<U>(p, blk0, nb, t);
    // the verdict k_pj_join left here (k_vertices_pj reads the word's upper part), the prefill of the partitioning kernel where
    // the join had nothing else to say (PJ_VERDICT_PREFILL) -- or a reference to the minimizer that went on for this one
    // (k_pj2_bucket); a follower (pj_run_role) has no verdict of its own: its leader, the last lane in front of it that is no
    // follower, says whether the key is in every assembly
    // (the verdict word is requested beside the follower bits, not behind them: a follower's word -- the prefill, nothing
    // else was written there -- is read and dropped)
    uint64_t fb[U];
    uint32_t v[U], ia[U], ii[U];
    bool in[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const bool there = blk0 + u < nb;  // (a sub-block beyond the last reads the first one's words)
        const uint32_t blk = there ? blk0 + u : blk0;
        ia[u] = t[u].a;
        ii[u] = (blk - t[u].b0) * 256u + threadIdx.x;
        in[u] = there && ii[u] < t[u].n;
        fb[u] = p.fol[(size_t)blk * 4u + wv];
        v[u] = p.slot[t[u].a][in[u] ? ii[u] : 0u];
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        if (blk0 + u >= nb) fb[u] = 0;
        if (!in[u]) v[u] = 0;
    }
    bool other[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {  // (the references, rare, for all U together)
        const bool isf = (fb[u] >> lane) & 1ull;
        if (isf) v[u] = 0u;
        other[u] = isf;
        if ((v[u] & 7u) == PJ_VERDICT_REF) {
            v[u] = p.slot[ia[u]][v[u] >> 3];
            other[u] = true;
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const bool isf = (fb[u] >> lane) & 1ull;
        const uint32_t lead = 63u - (uint32_t)__clzll(~fb[u] & ((2ull << lane) - 1ull));  // (lane 0 follows nobody; lane 63: the
        const uint32_t vl = __shfl(v[u], lead);                                            //  shift wraps to 0, the mask to all ones)
        uint32_t w = isf ? vl : v[u];
        if (other[u]) w &= MXG_MX_INALL;  // more than once in this assembly: neither unique nor shared
        const bool sh = in[u] && (w & MXG_MX_SHARED) != 0;
        if (in[u]) p.flags[ia[u]][ii[u]] = (uint8_t)(w & 7u);
        uint64_t bm;
        tail_ballot(ts, u, sh, bm);
        if (blk0 + u < nb && ia[u] == 0 && lane == 0) mask0[(size_t)(blk0 + u - p.bstart[0]) * 4u + wv] = bm;
    }
    __syncthreads();
    if (wv < U && lane == 0 && blk0 + wv < nb) {  // wave u publishes the count of sub-block u
        const uint32_t blk = blk0 + wv, a = asm_of_block(p, blk);
        count_publish(cnt + p.bstart[a], sup + sup_start(p, a), blk - p.bstart[a], tail_total(ts, wv));
    }
}

struct VertexParams {
    const uint8_t *flags;   // (MXG_MX_SHARED: a vertex)
    const uint32_t *cnt, *sup;  // shared minimizers per 256 elements of this assembly + super-counts (k_flags)
    uint64_t *n_shared;     // ctl[a]: total, written by the last tile
    const uint32_t *slot;
    const uint64_t *hash;
    const uint32_t *pos, *rec;
    uint32_t n;             // (an upper bound when n_ptr is set: fused sketch+graph call)
    const uint32_t *n_ptr;
    uint32_t first;   // 1: this is assembly 0 -> assign vertex ids
    uint32_t *vid;    // [cap+1] slot -> vertex id
    uint64_t *vhash;  // [nv]
    uint32_t *vpos, *vrec;  // this assembly's slice [nv]
    uint32_t *fv, *frec;    // this assembly's filtered order -> vertex id / record
    uint32_t *ivid;         // distributed graph (dgraph.hip): vertex id per ITEM (pre-filled with NONE), else nullptr
};

// ordered compaction of the shared minimizers of one assembly; rank r in filtered order
__global__ __launch_bounds__(256) void k_vertices(const VertexParams p)
{
    // (the global-table route, i.e. the fallback: one 256-block per thread block; the partitioned join's passes take U)
    __shared__ uint32_t sh[256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool f = i < (p.n_ptr ? min(*p.n_ptr, p.n) : p.n) && (p.flags[i] & MXG_MX_SHARED);
    __shared__ uint32_t sh_before;
    if (threadIdx.x < 64) {
        const uint32_t bef = count_prefix(p.cnt, p.sup, blockIdx.x);
        if (threadIdx.x == 0) sh_before = bef;
        if (blockIdx.x + 1 == gridDim.x) {  // the last tile also reports the total
            const uint32_t all = count_prefix(p.cnt, p.sup, (p.n + 255u) / 256u);
            if (threadIdx.x == 0) *p.n_shared = all;
        }
    }
    __syncthreads();
    const uint32_t r = sh_before + block_exclusive_256(f ? 1u : 0u, sh);
    if (!f) return;
    const uint32_t s = p.slot[i];
    uint32_t v;
    if (p.first) {
        v = r;
        p.vid[s] = v;
        p.vhash[v] = p.hash[i];
    } else {
        v = p.vid[s];
    }
    const uint32_t rec = p.rec[i];
    p.vpos[v] = p.pos[i];
    p.vrec[v] = rec;
    if (p.ivid) p.ivid[i] = v;
    p.fv[r] = v;
    p.frec[r] = rec;
}

// out[e] = shared minimizers before 256-block e of assembly 0: every block of this kernel takes 256 entries -- what precedes
// them from the two-level counts, the rest by a scan in LDS (one block scanning all 23 000 entries took 33 us)
__global__ __launch_bounds__(256) void k_block_prefix(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ sup, uint32_t n,
                                                      uint32_t *__restrict__ out)
{
    __shared__ uint32_t sh[256];
    __shared__ uint32_t sh_before;
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    const uint32_t c = e < n ? cnt[e] : 0u;
    if (threadIdx.x < 64) {
        const uint32_t bef = count_prefix(cnt, sup, blockIdx.x * 256u);
        if (threadIdx.x == 0) sh_before = bef;
    }
    __syncthreads();
    const uint32_t r = sh_before + block_exclusive_256(c, sh);
    if (e < n) out[e] = r;
}

// The vertex pass of the partitioned join, ALL assemblies in one launch.  A shared minimizer of assembly a > 0 carries the
// index i0 of its key's minimizer in assembly 0 (k_pj_join); its vertex id is the rank of i0 among assembly 0's shared
// minimizers = shared ones before i0's 256-block (bpref0) + set bits of mask0 before i0 inside the block: two small
// arrays (1 bit and 1/64 word per minimizer) that stay in L2, where the table-slot -> vertex-id array of k_vertices took a
// random 4-byte HBM write per vertex in assembly 0 and a random read per vertex in every other assembly.
struct VertexPjParams {
    AsmSet as;
    const uint32_t *pos[MXG_MAX_ASSEMBLIES], *rec[MXG_MAX_ASSEMBLIES];
    const uint32_t *cnt, *sup;
    uint64_t *n_shared;  // ctl[a]
    const uint64_t *mask0;
    const uint32_t *bpref0;
    uint64_t *vhash;
    uint32_t *vpos, *vrec, *fv, *frec;  // [A][nvs]
    uint32_t *rank;  // [A][nvs], rows 1 .. A - 1: the place of every vertex in the assembly's filtered order (the rank route of the
                     // edge kernels, graph_rank.h; nullptr: not wanted).  Row 0 is never written: assembly 0's vertex ids are its places
    uint32_t nvs;
    uint32_t *ivid[MXG_MAX_ASSEMBLIES];  // (owner of a partitioned graph stage: item -> vertex id, NONE32 for an item that is no vertex)
};

template <uint32_t U>
__global__ __launch_bounds__(256) void k_vertices_pj(const VertexPjParams p, uint32_t nb)
{
    __shared__ TailScan<U> ts;
    const uint32_t blk0 = blockIdx.x * U, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    TailAsm t[U];
    tail_asms<U>(p.as, blk0, nb, t);
    // (what the minimizers bring along first: their loads -- for a > 0 the chain verdict word -> mask words -> vertex id -- do not
    // need their rank, and a sub-block's prefix below is two dependent round trips every thread would otherwise wait for first.
    // The flag byte, the verdict word, record, position and hash of all U sub-blocks are requested together, whether the
    // minimizer is shared or not (three in four are): one round trip where the flag came first and the rest behind it.
    // Assembly 0 needs no verdict word and the others no hash: their threads all read element 0 of it, one line.)
    uint32_t ia[U], ii[U], vw[U], rec[U], pos[U];
    uint64_t hsh[U];
    bool in[U], f[U];
    {
        uint8_t fl[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const bool there = blk0 + u < nb;
            const uint32_t a = ia[u] = t[u].a, i = ii[u] = ((there ? blk0 + u : blk0) - t[u].b0) * 256u + threadIdx.x;
            in[u] = there && i < t[u].n;
            const uint32_t ic = in[u] ? i : 0u;
            fl[u] = p.as.flags[a][ic];
            vw[u] = p.as.slot[a][a ? ic : 0u];  // (the verdict word: flags in its three low bits)
            rec[u] = p.rec[a][ic];
            pos[u] = p.pos[a][ic];
            hsh[u] = p.as.hash[0][a ? 0u : ic];
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) f[u] = in[u] & ((fl[u] & MXG_MX_SHARED) != 0);  // (&: no branch around the flag)
    }
    // a > 0: the vertex id is the rank of the key's minimizer i0 in assembly 0.  The four mask words of i0's 256-block and the
    // block's prefix are requested together (the words in front of i0's own were a loop of dependent length), for two sub-blocks
    // at a time.  (<4> still takes 90 VGPRs, 5 waves per SIMD, and traced no faster than <2> with 58 and 8: by size the pass stops
    // at U = 2, join_plan.h.)
    uint32_t v0[U];
#pragma unroll
    for (uint32_t h = 0; h < U; h += 2) {
        constexpr uint32_t G = U < 2 ? U : 2;
        ulonglong2 mlo[G], mhi[G];
        uint32_t bp[G];
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t u = h + g;
            const uint32_t i0 = f[u] && ia[u] ? vw[u] >> 3 : 0u;  // (no vertex of an assembly > 0: block 0's words, dropped)
            const ulonglong2 *m = reinterpret_cast<const ulonglong2 *>(p.mask0 + ((i0 >> 6) & ~3u));  // (32-byte aligned)
            mlo[g] = m[0];
            mhi[g] = m[1];
            bp[g] = p.bpref0[i0 >> 8];
        }
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t i0 = vw[h + g] >> 3, q = (i0 >> 6) & 3u;
            const uint64_t own = q == 0 ? mlo[g].x : q == 1 ? mlo[g].y : q == 2 ? mhi[g].x : mhi[g].y;
            v0[h + g] = bp[g] + (uint32_t)__popcll(own & ((1ull << (i0 & 63u)) - 1ull)) + (q > 0 ? (uint32_t)__popcll(mlo[g].x) : 0u) +
                        (q > 1 ? (uint32_t)__popcll(mlo[g].y) : 0u) + (q > 2 ? (uint32_t)__popcll(mhi[g].x) : 0u);
        }
        if (U > 2) __builtin_amdgcn_sched_barrier(0);  // (or the scheduler requests the second pair's words beside the first's)
    }
    uint64_t bm[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) tail_ballot(ts, u, f[u], bm[u]);
    if (wv < U && blk0 + wv < nb) {  // wave u: what precedes sub-block u in its assembly
        const uint32_t blk_g = blk0 + wv, a = asm_of_block(p.as, blk_g);
        const uint32_t blk = blk_g - p.as.bstart[a], nblk = p.as.bstart[a + 1] - p.as.bstart[a];
        const uint32_t *cnt = p.cnt + p.as.bstart[a], *sup = p.sup + sup_start(p.as, a);
        const uint32_t bef = count_prefix(cnt, sup, blk);
        if (lane == 0) ts.before[wv] = bef;
        if (blk + 1 == nblk) {  // the assembly's last tile also reports its total
            const uint32_t all = count_prefix(cnt, sup, nblk);
            if (lane == 0) p.n_shared[a] = all;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        if (!in[u]) continue;
        const uint32_t a = ia[u], i = ii[u];
        const uint32_t r = ts.before[u] + tail_rank(ts, u, bm[u]);
        const uint32_t v = a ? v0[u] : r;
        if (p.ivid[a]) p.ivid[a][i] = f[u] ? v : NONE32;
        if (!f[u]) continue;
        if (!a) p.vhash[v] = hsh[u];
        const size_t o = (size_t)a * p.nvs;
        p.vpos[o + v] = pos[u];
        p.vrec[o + v] = rec[u];
        if (a && p.rank) p.rank[o + v] = r;  // (beside the two scattered stores above, at their index)
        p.fv[o + r] = v;
        p.frec[o + r] = rec[u];
    }
}

// blockIdx.y = assembly; all arrays are [A][stride].  adj[a][u] = {successor, predecessor} of vertex u in assembly a's filtered
// order (NONE32: none) -- one 8-byte entry, so that the kernels that ask "is v next to u in assembly b" touch one sector per
// (b, u), not two.  Every vertex occurs exactly once in every assembly's filtered list (a shared minimizer is unique in each
// assembly), so the thread of position r writes the whole entry of its vertex: nothing has to be cleared beforehand.
// (Records and vertices of r and of both neighbours are requested together for all U sub-blocks, inside the rows' `stride`
// words and beside the vertex count, not behind it: what lies beyond the count is read and dropped.)
template <uint32_t U>
__global__ __launch_bounds__(256) void k_adjacency(const uint32_t *__restrict__ fv0, const uint32_t *__restrict__ frec0,
                                                   const uint64_t *__restrict__ nv_ptr, uint2 *__restrict__ adj0, uint32_t stride)
{
    const size_t o = (size_t)blockIdx.y * stride;
    const uint32_t *fv = fv0 + o, *frec = frec0 + o;
    uint32_t rc[U], rn[U], rp[U], vc[U], vn[U], vp[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t r = (blockIdx.x * U + u) * 256u + threadIdx.x;  // (< 2^32: the grid covers `stride` < 2^32 / A positions)
        rc[u] = rn[u] = rp[u] = vc[u] = vn[u] = vp[u] = 0;
        if (r < stride) {
            rc[u] = frec[r];
            vc[u] = fv[r];
            if (r + 1 < stride) {
                rn[u] = frec[r + 1];
                vn[u] = fv[r + 1];
            }
            if (r > 0) {
                rp[u] = frec[r - 1];
                vp[u] = fv[r - 1];
            }
        }
    }
    const uint32_t nv = (uint32_t)*nv_ptr;  // number of shared minimizers, still in HBM (no host sync before this stage)
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t r = (blockIdx.x * U + u) * 256u + threadIdx.x;
        if (r >= nv) continue;  // (nv <= stride)
        // consecutive surviving minimizers of the same contig (ntjoin_utils.py:98-99)
        const uint32_t nx = (r + 1 < nv && rn[u] == rc[u]) ? vn[u] : NONE32;
        const uint32_t pv = (r > 0 && rp[u] == rc[u]) ? vp[u] : NONE32;
        adj0[o + vc[u]] = make_uint2(nx, pv);
    }
}

struct EdgeParams {
    const uint32_t *fv;   // [A][nv]   (nv = stride = upper bound of the vertex count; the count itself is *nv_ptr)
    const uint2 *adj;     // [A][nv]: {successor, predecessor} (k_adjacency); the rank route has none
    const uint32_t *frec, *rank;  // the rank route (k_edge_flags_rank, k_edges_rank): [A][nv] records of the filtered order, places of the vertices
    const uint64_t *nv_ptr;
    uint32_t nv, n_asm;
    uint8_t *eflag;       // [A*nv]
    uint32_t *bsum;       // edges per 256 items + super-counts (scan_kernels.h)
    uint32_t *bsuper;
    uint64_t *n_edges;    // ctl[CTL_EDGES], written by the last tile of k_edges
    uint64_t *host_ctl;   // pinned host copy of the control block, written by that tile too (no copy on the stream)
    uint32_t *eu, *ev, *esup;
    double *ew;
    double weights[MXG_MAX_ASSEMBLIES];
};

__device__ __forceinline__ uint32_t edge_mask(const EdgeParams &p, uint32_t u, uint32_t v)
{
    uint32_t m = 0;
    for (uint32_t b = 0; b < p.n_asm; ++b) {
        const uint2 q = p.adj[(size_t)b * p.nv + u];
        if (q.x == v || q.y == v) m |= 1u << b;
    }
    return m;
}

// item = a*nv + r : the pair (filtered[a][r], filtered[a][r+1]); flagged iff assembly a is the first supporter
// (up to eight assemblies the flag byte IS the edge's support mask: k_edges then has nothing to look up again -- 2 A random
// reads per edge less)
// (n_items = n_asm * nv < 2^32; the row a = item / nv may change anywhere inside a thread block: it is the item's own)
template <uint32_t U>
__global__ __launch_bounds__(256) void k_edge_flags(const EdgeParams p, uint32_t n_items)
{
    __shared__ TailScan<U> ts;
    const uint32_t blk0 = blockIdx.x * U, nblk = (n_items + 255u) / 256u, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    // the vertices of all U sub-blocks, beside the vertex count (what lies beyond it in a row is read and dropped)
    uint32_t uu[U], ia[U];
    bool live[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t item = (blk0 + u) * 256u + threadIdx.x;
        uu[u] = p.fv[blk0 + u < nblk && item < n_items ? item : 0u];
    }
    const uint32_t nvc = (uint32_t)*p.nv_ptr;
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t item = (blk0 + u) * 256u + threadIdx.x;
        const bool in = blk0 + u < nblk && item < n_items;
        ia[u] = in ? item / p.nv : 0u;
        live[u] = in && item - ia[u] * p.nv < nvc;  // (beyond the count: not a vertex)
    }
    uint8_t f[U];
    if (p.n_asm <= 4u) {
        // (up to four assemblies: their entries of u are requested together with this assembly's own -- the successor is
        // then one of them -- instead of behind it; and all U sub-blocks' together)
        uint2 q[U][4];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b)
                q[u][b] = b < p.n_asm ? p.adj[(size_t)b * p.nv + (live[u] ? uu[u] : 0u)] : make_uint2(NONE32, NONE32);
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t a = ia[u];
            const uint32_t v = a == 0 ? q[u][0].x : a == 1 ? q[u][1].x : a == 2 ? q[u][2].x : q[u][3].x;
            uint32_t m = 0;
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b)
                if (b < p.n_asm && (q[u][b].x == v || q[u][b].y == v)) m |= 1u << b;
            f[u] = live[u] && v != NONE32 && (uint32_t)__builtin_ctz(m) == a ? (uint8_t)m : (uint8_t)0;
        }
    } else {
        uint32_t v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) v[u] = p.adj[(size_t)ia[u] * p.nv + (live[u] ? uu[u] : 0u)].x;
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
            if (!live[u]) v[u] = NONE32;
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            f[u] = 0;
            if (v[u] == NONE32) continue;
            const uint32_t m = edge_mask(p, uu[u], v[u]);
            if ((uint32_t)__builtin_ctz(m) == ia[u]) f[u] = p.n_asm <= 8u ? (uint8_t)m : (uint8_t)1;
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t item = (blk0 + u) * 256u + threadIdx.x;
        if (blk0 + u < nblk && item < n_items) p.eflag[item] = f[u];
        uint64_t bm;
        tail_ballot(ts, u, f[u] != 0, bm);
    }
    __syncthreads();
    if (wv < U && lane == 0 && blk0 + wv < nblk) count_publish(p.bsum, p.bsuper, blk0 + wv, tail_total(ts, wv));
}

// (U 256-blocks per thread block, one item per thread of each: see "the tail's ordered passes" above)
template <uint32_t U>
__global__ __launch_bounds__(256) void k_edges(const EdgeParams p, uint32_t n_items)
{
    __shared__ TailScan<U> ts;
    const uint32_t blk0 = blockIdx.x * U, nblk = (n_items + 255u) / 256u, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    // (the edges themselves first: their chain of loads -- flag and vertex, successor, the other assemblies' adjacency -- does not
    // need the edges' places, and a sub-block's prefix below is two dependent round trips every thread would otherwise wait for)
    uint32_t fb[U], uu[U], v[U], m[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t item = (blk0 + u) * 256u + threadIdx.x;
        const bool in = blk0 + u < nblk && item < n_items;
        fb[u] = p.eflag[in ? item : 0u];
        uu[u] = p.fv[in ? item : 0u];  // (fv is [A][nv] like the items; beside the flag, not behind it)
        if (!in) fb[u] = 0;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u)  // (no edge: entry 0, dropped)
        v[u] = p.adj[fb[u] ? (size_t)(((blk0 + u) * 256u + threadIdx.x) / p.nv) * p.nv + uu[u] : (size_t)0].x;
    uint64_t bm[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) tail_ballot(ts, u, fb[u] != 0, bm[u]);
    if (wv < U && blk0 + wv < nblk) {  // wave u: edges in front of sub-block u
        const uint32_t bef = count_prefix(p.bsum, p.bsuper, blk0 + wv);
        if (lane == 0) ts.before[wv] = bef;
        if (blk0 + wv + 1 == nblk) {  // the last tile also reports the total
            const uint32_t all = count_prefix(p.bsum, p.bsuper, nblk);
            if (lane == 0) {
                *p.n_edges = all;
                p.host_ctl[32] = all;  // CTL_EDGES
            }
            if (lane < p.n_asm) p.host_ctl[lane] = p.nv_ptr[lane];  // shared minimizers per assembly
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        m[u] = fb[u];
        if (fb[u] && p.n_asm > 8u) m[u] = edge_mask(p, uu[u], v[u]);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        if (!fb[u]) continue;
        // python: sum(weights[f] for f in support) -- int 0 start, then float adds in support (= assembly) order
        double wsum = 0.0;
        for (uint32_t b = 0; b < p.n_asm; ++b)
            if (m[u] & (1u << b)) wsum = wsum + p.weights[b];
        const uint32_t e = ts.before[u] + tail_rank(ts, u, bm[u]);
        p.eu[e] = uu[u];
        p.ev[e] = v[u];
        p.esup[e] = m[u];
        p.ew[e] = wsum;
    }
}

// ---- the rank route of the two edge passes (GRAPH_FULL behind an LDS join; MXG_GRAPH_RANK=0: k_adjacency and the passes above) ----
// No adjacency table (graph_rank.h).  The successor of item (a, r) is fv[a][r + 1] if frec[a][r + 1] == frec[a][r] and r + 1 is
// below the vertex count: coalesced loads of the item's own row.  v is next to u in another assembly b iff their places there,
// rank[b][u] and rank[b][v] (k_vertices_pj; assembly 0's are the vertex ids themselves), differ by one and lie in one record: two
// neighbouring words of frec[b], fetched only where the places differ by one.  An item of assembly 0 has u = r and v = r + 1, so
// its places in the others are coalesced loads too, requested beside fv and frec.
__device__ __forceinline__ uint32_t edge_mask_rank(const EdgeParams &p, uint32_t u, uint32_t v)
{
    const uint32_t last = p.nv - 1u;  // (a vertex and a place are held against their row: see rank_fetch)
    return rank_support_mask(
        p.n_asm, u, v, [&](uint32_t b, uint32_t x) { return b ? p.rank[(size_t)b * p.nv + min(x, last)] : x; },
        [&](uint32_t b, uint32_t r) { return p.frec[(size_t)b * p.nv + min(r, last)]; });
}

// k_edge_flags from ranks.  NB: how many OTHER assemblies' places and records are requested up front -- 1 (n_asm <= 2), 3
// (n_asm <= 4) -- or 0: more than four assemblies, looked up item by item (edge_mask_rank).  The k-th other assembly of an item of
// assembly a is b = k < a ? k : k + 1.
template <uint32_t U, uint32_t NB>
__global__ __launch_bounds__(256) void k_edge_flags_rank(const EdgeParams p, uint32_t n_items)
{
    __shared__ TailScan<U> ts;
    const uint32_t blk0 = blockIdx.x * U, nblk = (n_items + 255u) / 256u, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    constexpr uint32_t K = NB ? NB : 1u;
    // The rows are strided by an upper bound of the vertex count (the smallest assembly's minimizers; four assemblies at 0.5 to
    // 2 % divergence share one minimizer in six).  A thread block all of whose items lie beyond the count of their row reads
    // nothing: its sub-blocks count no edge, its flag bytes stay unwritten, and k_edges_rank, which decides the same way from the
    // same count, does not read them.  So the count comes first here, not beside the loads.
    const uint32_t nvc = (uint32_t)*p.nv_ptr;
    if (rank_items_unused(blk0 * 256u, U * 256u, n_items, p.nv, nvc)) {
        if (wv < U && lane == 0 && blk0 + wv < nblk) count_publish(p.bsum, p.bsuper, blk0 + wv, 0u);
        return;
    }
    // vertex and record of the item and of the one behind it for all U sub-blocks; and, as if the item
    // were assembly 0's (item = r = u, v = r + 1), its two places in the other assemblies (any other item: word 0, dropped)
    uint32_t uu[U], vv[U], rc[U], rn[U], r0[U][K], r1[U][K];
    bool in[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t item = (blk0 + u) * 256u + threadIdx.x;
        in[u] = blk0 + u < nblk && item < n_items;
        const uint32_t i0 = in[u] ? item : 0u, i1 = in[u] && item + 1u < n_items ? item + 1u : 0u;
        const bool first = item < p.nv;  // assembly 0's row is the identity (k_vertices_pj): its vertices are not fetched
        uu[u] = p.fv[first ? 0u : i0];
        vv[u] = p.fv[first ? 0u : i1];
        if (first) uu[u] = item, vv[u] = item + 1u;
        rc[u] = p.frec[i0];
        rn[u] = p.frec[i1];
        const uint32_t j0 = in[u] && first ? item : 0u, j1 = in[u] && item + 1u < p.nv ? item + 1u : 0u;
#pragma unroll
        for (uint32_t k = 0; k < NB; ++k) {
            const size_t row = k + 1u < p.n_asm ? (size_t)(k + 1u) * p.nv : (size_t)0;
            r0[u][k] = p.rank[row + j0];
            r1[u][k] = p.rank[row + j1];
        }
    }
    uint32_t ia[U];
    bool succ[U];  // the item has a successor: the pair (u, v) exists
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t item = (blk0 + u) * 256u + threadIdx.x;
        ia[u] = in[u] ? item / p.nv : 0u;
        succ[u] = in[u] && item - ia[u] * p.nv + 1u < nvc && rn[u] == rc[u];  // (nvc <= nv: the one behind is in the item's row)
    }
    uint8_t f[U];
    if constexpr (NB > 0) {
        // places of u and v in the other assemblies that are neither assembly 0 nor this item's own: gathers, for all U together
        uint32_t gu[U][K], gv[U][K];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
#pragma unroll
            for (uint32_t k = 1; k < NB; ++k) {
                const uint32_t b = k < ia[u] ? k : k + 1u;
                const bool need = succ[u] && ia[u] != 0u && b < p.n_asm && uu[u] < p.nv && vv[u] < p.nv;  // (held against the row, as the places are)
                const size_t row = need ? (size_t)b * p.nv : (size_t)0;
                gu[u][k] = p.rank[row + (need ? uu[u] : 0u)];
                gv[u][k] = p.rank[row + (need ? vv[u] : 0u)];
            }
        // the two records, where the places differ by one (else word 0 twice, dropped)
        uint32_t x[U][K], y[U][K];
        bool w[U][K];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
#pragma unroll
            for (uint32_t k = 0; k < NB; ++k) {
                const uint32_t b = k < ia[u] ? k : k + 1u;
                const uint32_t ru = ia[u] == 0u ? r0[u][k] : k == 0u ? uu[u] : gu[u][k];
                const uint32_t rv = ia[u] == 0u ? r1[u][k] : k == 0u ? vv[u] : gv[u][k];
                uint32_t lo, hi;
                w[u][k] = rank_fetch(succ[u] && b < p.n_asm, ru, rv, p.nv, lo, hi);
                const size_t row = w[u][k] ? (size_t)b * p.nv : (size_t)0;
                x[u][k] = p.frec[row + lo];
                y[u][k] = p.frec[row + hi];
            }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            uint32_t m = 1u << ia[u];  // (its own assembly: v is its successor there)
#pragma unroll
            for (uint32_t k = 0; k < NB; ++k)
                if (w[u][k] && x[u][k] == y[u][k]) m |= 1u << (k < ia[u] ? k : k + 1u);
            f[u] = succ[u] ? rank_edge_flag(m, ia[u], p.n_asm) : (uint8_t)0;
        }
    } else {
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            f[u] = 0;
            if (!succ[u]) continue;
            f[u] = rank_edge_flag(edge_mask_rank(p, uu[u], vv[u]), ia[u], p.n_asm);
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t item = (blk0 + u) * 256u + threadIdx.x;
        if (in[u]) p.eflag[item] = f[u];
        uint64_t bm;
        tail_ballot(ts, u, f[u] != 0, bm);
    }
    __syncthreads();
    if (wv < U && lane == 0 && blk0 + wv < nblk) count_publish(p.bsum, p.bsuper, blk0 + wv, tail_total(ts, wv));
}

// k_edges from ranks: v is the vertex behind u in the item's own row (a flagged item has one), requested beside the flag
template <uint32_t U>
__global__ __launch_bounds__(256) void k_edges_rank(const EdgeParams p, uint32_t n_items)
{
    __shared__ TailScan<U> ts;
    const uint32_t blk0 = blockIdx.x * U, nblk = (n_items + 255u) / 256u, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    // the last tile also reports the totals (all 64 lanes of the wave that holds it)
    auto report_totals = [&]() {
        const uint32_t all = count_prefix(p.bsum, p.bsuper, nblk);
        if (lane == 0) {
            *p.n_edges = all;
            p.host_ctl[32] = all;  // CTL_EDGES
        }
        if (lane < p.n_asm) p.host_ctl[lane] = p.nv_ptr[lane];  // shared minimizers per assembly
    };
    // a thread block of unused items (see k_edge_flags_rank, which left their flag bytes unwritten) has no edge
    if (rank_items_unused(blk0 * 256u, U * 256u, n_items, p.nv, (uint32_t)*p.nv_ptr)) {
        if (wv < U && blk0 + wv + 1 == nblk) report_totals();
        return;
    }
    uint32_t fb[U], uu[U], v[U], m[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t item = (blk0 + u) * 256u + threadIdx.x;
        const bool in = blk0 + u < nblk && item < n_items;
        const bool first = item < p.nv;  // assembly 0's row is the identity (k_vertices_pj): its vertices are not fetched
        fb[u] = p.eflag[in ? item : 0u];
        uu[u] = p.fv[in && !first ? item : 0u];
        v[u] = p.fv[in && !first && item + 1u < n_items ? item + 1u : 0u];
        if (first) uu[u] = item, v[u] = item + 1u;
        if (!in) fb[u] = 0;
    }
    uint64_t bm[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) tail_ballot(ts, u, fb[u] != 0, bm[u]);
    if (wv < U && blk0 + wv < nblk) {  // wave u: edges in front of sub-block u
        const uint32_t bef = count_prefix(p.bsum, p.bsuper, blk0 + wv);
        if (lane == 0) ts.before[wv] = bef;
        if (blk0 + wv + 1 == nblk) report_totals();
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        m[u] = fb[u];
        if (fb[u] && p.n_asm > 8u) m[u] = edge_mask_rank(p, uu[u], v[u]);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        if (!fb[u]) continue;
        // python: sum(weights[f] for f in support) -- int 0 start, then float adds in support (= assembly) order
        double wsum = 0.0;
        for (uint32_t b = 0; b < p.n_asm; ++b)
            if (m[u] & (1u << b)) wsum = wsum + p.weights[b];
        const uint32_t e = ts.before[u] + tail_rank(ts, u, bm[u]);
        p.eu[e] = uu[u];
        p.ev[e] = v[u];
        p.esup[e] = m[u];
        p.ew[e] = wsum;
    }
}

// distributed graph, owner side (dgraph.hip): adjacency arrives as messages {kind << 8 | assembly, local vertex, other
// vertex (global id), 0}: kind 0 sets the successor, kind 1 the predecessor of adj[a][local] (the array was filled with NONE32)
__global__ __launch_bounds__(256) void k_apply_msgs(const uint4 *__restrict__ msgs, uint64_t n, uint32_t stride, uint32_t *adj)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4 m = msgs[i];
    adj[((size_t)(m.x & 255u) * stride + m.y) * 2u + ((m.x >> 8) ? 1u : 0u)] = m.z;
}

__global__ __launch_bounds__(256) void k_iota_rows(uint32_t *a, uint32_t stride)  // a[row][i] = i
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < stride) a[(size_t)blockIdx.y * stride + i] = i;
}

// ------------------------------------------------------------------------------------------------------
template <class T>
static int d2h(mxg_handle *h, std::vector<T> &dst, const void *src, size_t n)
{
    dst.resize(n);
    if (n) MXG_HIP(h, hipMemcpyAsync(dst.data(), src, n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    return MXG_OK;
}

__global__ __launch_bounds__(256) void k_count_unique(const uint8_t *__restrict__ flags, uint32_t n, unsigned long long *counter)
{
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool u = i < n && (flags[i] & MXG_MX_UNIQUE);
    uint64_t m = __ballot(u);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// The stage's control block (u64 words): g_ctl in HBM, which the kernels count in, and its pinned host copy (pinned_gctl), which
// k_edges and the join kernels write for the host to read behind the stage's one sync.
enum CtlWord : uint32_t {
    CTL_SHARED = 0,    // [0..MXG_MAX_ASSEMBLIES) shared minimizers per assembly (equal by construction): the vertex count
    CTL_EDGES = 32,    // edge count
    CTL_UNIQUE = 33,   // unique count (reserved: mxg_get_stats counts lazily from the flags)
    CTL_PJ_FAIL = 34,  // host copy only: a partition's table or a coarse partition's capacity overflowed (k_pj_join)
    CTL_WORDS = 40,
};
static_assert(CTL_SHARED + MXG_MAX_ASSEMBLIES <= CTL_EDGES, "the per-assembly counts end before the other words");

static int build_graph_impl(mxg_handle *h, const GraphCall &c, bool global_table);

int build_graph(mxg_handle *h, const GraphCall &c)
{
    h->stat_graph_join = 0;
    uint64_t how = 0;
    JoinLearnt &learnt = h->pj_learnt;
    // what the handle learnt from an overflow holds for the sketches it was learnt on.  (The fused call and the owner's slots, c.gb:
    // the sizes are bounds, the sketches' own are not known yet -- the signature is neither compared nor taken.)
    if (!c.gb) {
        uint64_t n_mx[MXG_MAX_ASSEMBLIES];
        const uint32_t n = (uint32_t)std::min<size_t>(h->asms.size(), MXG_MAX_ASSEMBLIES);
        for (uint32_t a = 0; a < n; ++a) n_mx[a] = h->asms[a]->n_mx;
        learnt.sketches_are(JoinLearnt::signature(n, n_mx));
    }
    // (a handle whose minimizers once overflowed a partition -- a key of huge multiplicity: satellite arrays -- goes straight to
    // the global table afterwards: the same assemblies would overflow again)
    int rc = build_graph_impl(h, c, learnt.overflowed);
    // (a coarse partition outgrew its capacity -- hash skew: a key of large multiplicity -- while the tables held: once more with
    // the capacity the cursors ask for, which the handle keeps)
    if (rc == RC_RETRY_PJ) {
        how |= MXG_JOIN_RESIZED;
        rc = build_graph_impl(h, c, false);
    }
    if (rc == RC_RETRY_PJ) rc = RC_RETRY_GLOBAL;
    if (rc == RC_RETRY_GLOBAL) {
        how |= MXG_JOIN_GAVE_UP;
        learnt.gave_up();
        rc = build_graph_impl(h, c, true);
    }
    h->stat_graph_join |= how;
    return rc;
}

// The join's layout: the shape join_shape derives from the assemblies' sizes (the sketches' own, or the bounds gb of the fused
// call) before anything is launched, where every array lies, and the allocations that go with it.  The fused call plans before
// its first filter is launched (graph_plan_early) and hands the plan on.
struct JoinPlan : JoinShape {
    uint32_t pj_force_fail = 0;
    uint64_t *pj_mask0 = nullptr;
    uint32_t *pj_bpref0 = nullptr;
    AsmSet as_all;
    uint32_t n_fsup = 0, n_esup = 0;
    uint32_t *fsup = nullptr, *esup = nullptr, *cnt = nullptr;
    // two-level join
    uint32_t *M = nullptr, *cursor = nullptr;
    uint4 *recs1 = nullptr, *recs2 = nullptr;
    PjSubCaps sc;
    size_t clear_words = 0;  // split: super-counts and cursors are one run of g_cnt, cleared by one fill
};

static int plan_join(mxg_handle *h, int mode, const GraphBounds *gb, bool global_table, bool split, JoinPlan &pl)
{
    const uint32_t A = (uint32_t)h->asms.size();
    if (A == 0) return set_err(h, MXG_EINVAL, "mxg_build_graph: no assemblies");
    if (A > MXG_MAX_ASSEMBLIES) return set_err(h, MXG_ELIMIT, "at most %d assemblies", MXG_MAX_ASSEMBLIES);
    pl = JoinPlan();
    JoinRequest rq;
    rq.A = A;
    for (uint32_t ai = 0; ai < A; ++ai) {
        Assembly *a = h->asms[ai];
        if (!gb && !a->has_sketch) return set_err(h, MXG_EINVAL, "assembly '%s' has no sketch (call mxg_sketch)", a->name.c_str());
        rq.n_of[ai] = gb ? gb->n_bound[ai] : a->n_mx;
    }
    rq.mode = mode;
    rq.bounds = gb != nullptr;
    rq.global_table = global_table;
    rq.split = split;
    // MXG_GRAPH_JOIN=global|lds, MXG_PJ_TWO_LEVEL=1 (two levels on small inputs) and MXG_PJ_FORCE_FAIL=1 are test knobs (knob_*:
    // as the handle first saw them)
    const char *join_env = knob_raw(h, "MXG_GRAPH_JOIN");
    rq.join_global = join_env && !strcmp(join_env, "global");
    rq.force_two_level = knob_u64(h, "MXG_PJ_TWO_LEVEL", 0) != 0;
    rq.graph_u = (uint32_t)std::min<uint64_t>(knob_u64(h, "MXG_GRAPH_U", 0), 8);  // 1 | 2 | 4 forces the tail passes' width
    rq.no_graph_rank = knob_u64(h, "MXG_GRAPH_RANK", 1) == 0;  // 0: k_adjacency and the table's edge passes where the plan takes the rank route (A/B knob)
    rq.pj_tiles = (uint32_t)std::min<uint64_t>(knob_u64(h, "MXG_PJ_TILES", 0), 8);  // 1 | 2 forces level 1's tiles per thread block
    // MXG_PJ_REC12=0 / MXG_PJ_PREFILL0=0: the 16-byte records / the one prefill rule where the plan would choose otherwise (A/B knobs);
    // MXG_PJ_SPLIT=1: sub-ranges per assembly in the stage's own plan too (test knob: the fused call's layout over given minimizers)
    rq.no_rec12 = knob_u64(h, "MXG_PJ_REC12", 1) == 0;
    rq.no_pipe = knob_u64(h, "MXG_PJ_PIPE", 1024) == 0;
    rq.no_prefill0 = knob_u64(h, "MXG_PJ_PREFILL0", 1) == 0;
    if (knob_u64(h, "MXG_PJ_SPLIT", 0) && mode == GRAPH_FULL) rq.split = true;
    switch (join_shape(rq, h->pj_learnt, pl)) {
    case JS_TOO_MANY_MINIMIZERS: return set_err(h, MXG_ELIMIT, "too many minimizers for one table (%llu)", (unsigned long long)pl.N);
    case JS_TOO_MANY_ITEMS: return set_err(h, MXG_ELIMIT, "graph too large for 32-bit item indices");
    case JS_OK: break;
    }
    pl.pj_force_fail = knob_u64(h, "MXG_PJ_FORCE_FAIL", 0) ? 1u : 0u;
    pl.sc.n_sub = pl.n_sub;
    for (uint32_t a = 0; a < MXG_MAX_ASSEMBLIES; ++a) pl.sc.cap[a] = pl.sub_cap[a];
    const uint64_t *const n_of = pl.n_of;
    const uint32_t nb = pl.nb, P = pl.P, P1 = pl.P1;

    if (!pl.pj) MXG_HIP(h, h->g_keys.ensure(((size_t)pl.cap + 1) * sizeof(Slot)));  // (the partitioned join keeps its N records here)
    // global table: slot -> vertex id; partitioned join: assembly 0's shared mask (8 B per 64 minimizers) + block prefix
    // (+ partitioned join: one "follower" bit per minimizer of every assembly, pj_run_role)
    const size_t nb0 = pl.nb0, nb_all = nb;
    MXG_HIP(h, h->g_vid.ensure(pl.pj ? (nb0 + nb_all) * 4 * 8 + nb0 * 4 + 64 : ((size_t)pl.cap + 1) * 4));
    pl.pj_mask0 = h->g_vid.as<uint64_t>();
    uint64_t *const pj_fol = pl.pj_mask0 + nb0 * 4;
    pl.pj_bpref0 = reinterpret_cast<uint32_t *>(pj_fol + nb_all * 4);
    MXG_HIP(h, h->g_ctl.ensure(CTL_WORDS * 8));

    AsmSet &as_all = pl.as_all;
    as_all.n_asm = A;
    as_all.full = pl.full;
    as_all.fol = pl.pj ? pj_fol : nullptr;
    for (uint32_t a = 0; a < A; ++a) {
        Assembly *as = h->asms[a];
        MXG_HIP(h, as->d_slot.ensure(std::max<uint64_t>(n_of[a] * 4, 16)));
        MXG_HIP(h, as->d_flags.ensure(std::max<uint64_t>(n_of[a], 16)));
        as_all.n[a] = (uint32_t)n_of[a];
        as_all.n_ptr[a] = gb ? gb->n_ptr[a] : nullptr;
        as_all.hash[a] = as->d_hash.as<uint64_t>();
        as_all.slot[a] = as->d_slot.as<uint32_t>();
        as_all.flags[a] = as->d_flags.as<uint8_t>();
    }
    for (uint32_t a = A; a < MXG_MAX_ASSEMBLIES; ++a) {
        as_all.n[a] = 0;
        as_all.n_ptr[a] = nullptr;
        as_all.hash[a] = nullptr;
        as_all.slot[a] = nullptr;
        as_all.flags[a] = nullptr;
    }
    std::copy(pl.bstart, pl.bstart + MXG_MAX_ASSEMBLIES + 1, as_all.bstart);
    // per-256 counts of the two counting kernels and their super-counts (scan_kernels.h): [sup of k_flags, one run
    // per assembly | sup of k_edge_flags | cnt of k_flags]; k_insert zeroes the super-counts
    // (split: the cursors of the sub-ranges lie between the super-counts and the counts, so that one fill clears both)
    pl.n_fsup = ((nb >> SUP_SHIFT) + A + 1) * SUP_STRIDE;
    pl.n_esup = sup_words(pl.e_blocks);
    MXG_HIP(h, h->g_cnt.ensure(((size_t)pl.n_fsup + pl.n_esup + pl.n_cur + nb) * 4 + 64));
    pl.fsup = h->g_cnt.as<uint32_t>();
    pl.esup = pl.fsup + pl.n_fsup;
    pl.cnt = pl.esup + pl.n_esup + pl.n_cur;
    pl.clear_words = (size_t)pl.n_fsup + pl.n_esup + pl.n_cur;
    const bool resume = mode == GRAPH_DG_EDGES || mode == GRAPH_DG_EDGES_APPLIED;  // second half on the owner's handle
    if (nb && !resume && pl.pj && pl.two_level) {
        const size_t n_recs = (size_t)P1 * pl.cap1;
        MXG_HIP(h, h->g_part.ensure((size_t)P1 * pl.rows2 * (P + 1) * 4 + (size_t)P1 * PJ1_CS * 4));
        MXG_HIP(h, h->g_keys.ensure(n_recs * sizeof(uint4)));   // level-2 records (what k_flags_pj reads)
        MXG_HIP(h, h->g_recs1.ensure(n_recs * sizeof(uint4)));  // level-1 records
        pl.M = h->g_part.as<uint32_t>();
        pl.cursor = pl.n_cur ? pl.esup + pl.n_esup : pl.M + (size_t)P1 * pl.rows2 * (P + 1);
        pl.recs1 = h->g_recs1.as<uint4>();
        pl.recs2 = h->g_keys.as<uint4>();
    }
    return MXG_OK;
}

// levels 1 and 2 of the two-level join for the 256-blocks of assemblies [a_lo, a_hi) on stream st
static void launch_partition(mxg_handle *h, const JoinPlan &pl, uint32_t a_lo, uint32_t a_hi, hipStream_t st, uint32_t n_sup_clear)
{
    const uint32_t blk_lo = pl.as_all.bstart[a_lo], blk_hi = pl.as_all.bstart[a_hi];
    const uint32_t n_rows1 = (blk_hi - blk_lo + PJ_IPB / 256 - 1) / (PJ_IPB / 256);
    PjSub sub{1u, 0u, 0u, pl.cap1};
    uint32_t skew_lim = (uint32_t)std::min<uint64_t>(pl.N / pl.P1 + pl.N / pl.P1 / 32 + 2048, 0xFFFFFFFFull);  // 3 % above the mean
    if (pl.split) {
        sub = PjSub{pl.A, a_lo, pl.sub_off[a_lo], pl.sub_cap[a_lo]};
        skew_lim = pl.skew_lim[a_lo];
    }
    // level 1's tiles per thread block, by THIS launch's tile count (pj1_launch_tiles: one unless forced)
    const uint32_t g1 = pj1_launch_tiles(pl, a_lo, a_hi);
    auto level1 = pl.rec12 ? (g1 == 2 ? k_pj1_scatter<true, 2> : k_pj1_scatter<true, 1>) : k_pj1_scatter<false, 1>;
    if (n_rows1)
        hipLaunchKernelGGL(level1, dim3(pj_tiles_grid(n_rows1, g1)), dim3(PJ_BT), (size_t)pl.P1 * 8, st, pl.as_all, blk_lo, blk_hi, pl.P1 - 1,
                           pl.cap1, pl.cursor, pl.recs1, pl.fsup, n_sup_clear, sub, pl.prefill0);
    hipLaunchKernelGGL(pl.rec12 ? k_pj2_bucket<true> : k_pj2_bucket<false>, dim3(sub.cap / PJ_IPB, pl.P1), dim3(PJ_BT), (size_t)pl.P * 8, st,
                       pl.as_all, pl.recs1, pl.cursor, pl.cap1, pl.rows2, pl.P - 1, pl.M, pl.recs2,
                       knob_u64(h, "MXG_PJ_SKEW", 0) ? 0u : skew_lim, sub);
}

// A timed span of kind 5 (flush_timers adds it to ms_join and ms_graph).  What ms_join means on the early path, in one place:
// MXG_FLAG_TIMING_FINE puts one such span around each assembly's two partition kernels on that assembly's stream.  A span runs
// from the moment the stream reaches the kernels to their end, so for an assembly whose kernels wait for room beside another
// assembly's filter or slice kernel it holds that wait too (the reference's: ~530 us for ~100 us of work at 3 Gbp + 3 Gbp) and
// ms_join is then an upper bound of the join's work, not its share of the step.  Plain MXG_FLAG_TIMING records nothing here:
// ms_graph is the span of build_graph_impl on the main stream, i.e. the stage from the join kernel on; the last assembly's level
// 1 + 2, which do lie on the critical path behind its k_emit, are in neither ms_hash nor ms_graph (profiles/r07).
// The span is appended to h->ev_spans, where Driver::ev_end() closes ev_spans.back(): callers must have no driver span open
// (graph_partition_early runs behind enqueue_asm, which has closed its spans; k_emit is never held back in the one-call modes).
static int ev_pair(mxg_handle *h, hipEvent_t *a, hipEvent_t *b)
{
    while (h->ev_pool.size() < h->ev_used + 2) {
        hipEvent_t e;
        MXG_HIP(h, hipEventCreate(&e));
        h->ev_pool.push_back(e);
    }
    *a = h->ev_pool[h->ev_used];
    *b = h->ev_pool[h->ev_used + 1];
    h->ev_used += 2;
    h->ev_spans.push_back(TimedSpan{*a, *b, 0, false, 5});
    return MXG_OK;
}

int graph_plan_early(mxg_handle *h, const GraphBounds &gb, bool *early)
{
    *early = false;
    h->pj_early_done = 0;
    if (knob_u64(h, "MXG_PJ_EARLY", 1) == 0) return MXG_OK;
    MXG_HIP(h, hipSetDevice(h->device));
    if (!h->pj_plan) h->pj_plan = new JoinPlan;
    JoinPlan &pl = *h->pj_plan;
    // (a set of sizes the graph stage refuses: build_graph says so behind the sketches, as it always has)
    const std::string err_before = h->err;
    if (plan_join(h, GRAPH_FULL, &gb, h->pj_learnt.overflowed, true, pl) != MXG_OK || !(pl.pj && pl.two_level && pl.split && pl.nb)) {
        pl = JoinPlan();
        h->err = err_before;  // (not this call's error: the stage itself reports it if it still holds then)
        return MXG_OK;
    }
    // the cursors of the sub-ranges and the super-counts of the counting kernels, in front of everything: both streams' partition
    // kernels wait for this fill (ev_plan)
    MXG_HIP(h, hipMemsetAsync(pl.fsup, 0, pl.clear_words * 4, h->stream));
    if (!h->ev_plan) MXG_HIP(h, hipEventCreateWithFlags(&h->ev_plan, hipEventDisableTiming));
    MXG_HIP(h, hipEventRecord(h->ev_plan, h->stream));
    *early = true;
    return MXG_OK;
}

int graph_partition_early(mxg_handle *h, uint32_t a, hipStream_t st)
{
    const JoinPlan *pl = h->pj_plan;
    if (!pl || !pl->split || a != h->pj_early_done || a >= pl->A) return MXG_OK;  // (out of turn: the stage will partition by itself)
    if (h->asms[a]->d_hash.as<uint64_t>() != pl->as_all.hash[a] || h->asms[a]->d_slot.as<uint32_t>() != pl->as_all.slot[a]) return MXG_OK;  // (arrays moved since)
    if (st != h->stream) MXG_HIP(h, hipStreamWaitEvent(st, h->ev_plan, 0));
    const bool fine = (h->cfg.flags & MXG_FLAG_TIMING_FINE) != 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (fine) {
        const int rc = ev_pair(h, &e0, &e1);
        if (rc != MXG_OK) return rc;
        MXG_HIP(h, hipEventRecord(e0, st));
    }
    launch_partition(h, *pl, a, a + 1, st, 0u);
    MXG_HIP(h, hipGetLastError());
    if (fine) MXG_HIP(h, hipEventRecord(e1, st));
    ++h->pj_early_done;
    return MXG_OK;
}

void graph_drop_plan(mxg_handle *h)
{
    delete h->pj_plan;
    h->pj_plan = nullptr;
}

// The fused call's plan, if this is the stage it was made for and every assembly has been partitioned under the sketches; whatever
// comes after (a second attempt, a later call) plans and partitions for itself, into `own`.  Either way nothing of the early
// plan stays in force.
static int take_or_make_plan(mxg_handle *h, const GraphCall &c, bool global_table, JoinPlan &own, const JoinPlan **plan)
{
    const JoinPlan *ep = h->pj_plan;
    bool early = ep && ep->split && h->pj_early_done != 0 && h->pj_early_done == ep->A && c.gb && c.mode == GRAPH_FULL && !global_table &&
                 ep->A == h->asms.size();
    for (uint32_t a = 0; early && a < ep->A; ++a) early = c.gb->n_bound[a] == ep->n_of[a] && c.gb->n_ptr[a] == ep->as_all.n_ptr[a];
    h->pj_early_done = 0;
    *plan = early ? ep : &own;
    if (early) return MXG_OK;
    const int rc = plan_join(h, c.mode, c.gb, global_table, false, own);
    if (rc != MXG_OK && c.mode != GRAPH_DG_EDGES && c.mode != GRAPH_DG_EDGES_APPLIED)
        for (Assembly *a : h->asms) a->flags_valid = a->flags_on_host = false;
    return rc;
}

// a tail pass at its width (U = 1, 2 or 4: graph_tail_u)
#define TAIL_LAUNCH(kernel, U, grid, stream, ...)                                                      \
    do {                                                                                               \
        if ((U) == 4) hipLaunchKernelGGL(kernel<4>, grid, dim3(256), 0, stream, __VA_ARGS__);          \
        else if ((U) == 2) hipLaunchKernelGGL(kernel<2>, grid, dim3(256), 0, stream, __VA_ARGS__);     \
        else hipLaunchKernelGGL(kernel<1>, grid, dim3(256), 0, stream, __VA_ARGS__);                   \
    } while (0)

// ... of a kernel with a second template argument
#define TAIL_LAUNCH2(kernel, U, X, grid, stream, ...)                                                  \
    do {                                                                                               \
        if ((U) == 4) hipLaunchKernelGGL((kernel<4, X>), grid, dim3(256), 0, stream, __VA_ARGS__);     \
        else if ((U) == 2) hipLaunchKernelGGL((kernel<2, X>), grid, dim3(256), 0, stream, __VA_ARGS__); \
        else hipLaunchKernelGGL((kernel<1, X>), grid, dim3(256), 0, stream, __VA_ARGS__);              \
    } while (0)

// One attempt at the stage: the phases of build_graph_impl, in the order it enqueues them.
struct GraphStage {
    mxg_handle *const h;
    const GraphCall &c;
    const JoinPlan &pl;
    const bool early;   // the plan is the fused call's: levels 1 and 2 have run behind every assembly's own k_emit
    const bool resume;  // second half on the owner's handle: flags and vertices are there
    const bool fine, timing;
    Graph &g;
    uint64_t *ctl = nullptr, *hctl = nullptr;  // the control block in HBM and its pinned host copy
    uint64_t *pj_fail = nullptr;               // where the LDS join reports failure

    GraphStage(mxg_handle *h_, const GraphCall &c_, const JoinPlan &pl_, bool early_)
        : h(h_), c(c_), pl(pl_), early(early_), resume(c_.mode == GRAPH_DG_EDGES || c_.mode == GRAPH_DG_EDGES_APPLIED),
          fine((h_->cfg.flags & MXG_FLAG_TIMING_FINE) != 0 && c_.mode == GRAPH_FULL), timing((h_->cfg.flags & MXG_FLAG_TIMING) != 0 || fine),
          g(h_->graph)
    {
    }
    bool joins() const { return pl.nb && !resume; }
    size_t anv() const { return (size_t)pl.A * pl.nvs; }

    // host state, the first timer, the table's fill, the control blocks
    int begin()
    {
        for (uint32_t ai = 0; ai < pl.A; ++ai) {
            Assembly *a = h->asms[ai];
            if (!resume) a->flags_on_host = false;
            a->flags_valid = true;
        }
        if (!resume) g = Graph();
        g.n_asm = pl.A;
        if (fine && !h->ev_g[0]) {
            MXG_HIP(h, hipEventCreate(&h->ev_g[0]));
            MXG_HIP(h, hipEventCreate(&h->ev_g[1]));
        }
        if (timing) MXG_HIP(h, hipEventRecord(h->ev0, h->stream));
        if (!resume)
            h->stat_graph_join = (pl.pj ? (pl.two_level ? MXG_JOIN_LDS_TWO_LEVEL : MXG_JOIN_LDS) : MXG_JOIN_GLOBAL) | (early ? MXG_JOIN_EARLY : 0);
        // MXG_DEBUG_JOIN=1: the plan's choices that mxg_stats::graph_join has no bit for, one line per attempt (tests read it)
        // (tiles1: level 1's tiles per thread block, the widest of the attempt's launches; 0: one level or no LDS join.  Level 2
        // always takes one)
        if (!resume && knob_u64(h, "MXG_DEBUG_JOIN", 0)) {
            uint32_t t1 = 0;
            for (uint32_t a = 0; pl.pj && pl.two_level && a < (pl.split ? pl.A : 1u); ++a)
                t1 = std::max(t1, pj1_launch_tiles(pl, pl.split ? a : 0u, pl.split ? a + 1 : pl.A));
            fprintf(stderr, "[mxg] join pj=%d two_level=%d split=%d early=%d record_bytes=%d prefill0=%u P1=%u rows2=%u tiles1=%u rank=%d\n",
                    (int)pl.pj, (int)pl.two_level, (int)pl.split, (int)early, pl.rec12 ? 12 : 16, pl.prefill0, pl.P1, pl.rows2, t1, (int)pl.graph_rank);
        }
        // (the LDS joins clear nothing: every word of M and of the record regions that is read is written by this call)
        if (!pl.pj && !resume) MXG_HIP(h, hipMemsetAsync(h->g_keys.p, 0xFF, ((size_t)pl.cap + 1) * sizeof(Slot), h->stream));  // one fill: see Slot
        ctl = h->g_ctl.as<uint64_t>();  // every word the host reads of it is written by a kernel of this call
        if (!h->pinned_gctl) MXG_HIP(h, hipHostMalloc((void **)&h->pinned_gctl, CTL_WORDS * 8));
        hctl = h->pinned_gctl;
        memset(hctl, 0, CTL_WORDS * 8);
        pj_fail = pl.dg_pj ? dg_pj_fail_word(h) : hctl + CTL_PJ_FAIL;  // (the device word: cleared by dg_owner_slots)
        return MXG_OK;
    }

    // k_pj_join over the n_parts partitions of `recs`, one block each -- or, behind two levels (cursor: the coarse partitions'),
    // k_pj_join_pipe with MXG_PJ_PIPE blocks that take partitions in turn (0: never) while a partition's rows fit its pipeline
    void launch_join(uint4 *recs, uint32_t *M, uint32_t n_parts, uint32_t n_rows, const uint32_t *cursor)
    {
        const bool narrow = pl.A <= 16;  // the seen and dup masks share one word per slot
        const uint32_t cap1 = cursor ? pl.cap1 : 0u, rows2 = cursor ? pl.rows2 : 0u;
        const uint64_t pipe_blocks = cursor ? knob_u64(h, "MXG_PJ_PIPE", 1024) : 0;
        const uint32_t prefill0 = cursor ? pl.prefill0 : 0u;  // (one level: k_pj_bucket knows the one rule)
        if (pipe_blocks && rows2 <= 256) {
            auto kernel = pl.rec12 ? (narrow ? k_pj_join_pipe<true, true> : k_pj_join_pipe<false, true>)
                                   : (narrow ? k_pj_join_pipe<true, false> : k_pj_join_pipe<false, false>);
            hipLaunchKernelGGL(kernel, dim3((uint32_t)std::min<uint64_t>(pipe_blocks, n_parts)), dim3(256), 0, h->stream, recs, M, pl.P, n_parts,
                               pj_fail, pl.pj_force_fail, cursor, cap1, rows2, pl.as_all, pl.sc, prefill0);
        } else  // (join_shape gives 12-byte records to the pipelined kernel only)
            hipLaunchKernelGGL(narrow ? k_pj_join<true> : k_pj_join<false>, dim3(n_parts), dim3(256), 0, h->stream, recs, M, pl.P, n_rows,
                               pj_fail, pl.pj_force_fail, cursor, cap1, rows2, pl.as_all, pl.sc, prefill0);
    }
    void flags_pj()
    {
        TAIL_LAUNCH(k_flags_pj, pl.u_flags, dim3(graph_tail_grid(pl.nb, pl.u_flags)), h->stream, pl.as_all, pl.nb, pl.cnt, pl.fsup, pl.pj_mask0);
    }
    int join_two_level()
    {
        if (!early && pl.split) {  // (MXG_PJ_SPLIT: the fused call's layout, one assembly after the other)
            MXG_HIP(h, hipMemsetAsync(pl.fsup, 0, pl.clear_words * 4, h->stream));
            for (uint32_t a = 0; a < pl.A; ++a) launch_partition(h, pl, a, a + 1, h->stream, 0u);
        } else if (!early) {  // (else: both levels ran behind every assembly's own k_emit, the cursors were cleared in front of the step)
            MXG_HIP(h, hipMemsetAsync(pl.cursor, 0, (size_t)pl.P1 * PJ1_CS * 4, h->stream));
            launch_partition(h, pl, 0, pl.A, h->stream, pl.n_fsup + pl.n_esup);
        }
        launch_join(pl.recs2, pl.M, pl.P1 * pl.P, 0u, pl.cursor);
        flags_pj();
        return MXG_OK;
    }
    int join_one_level()
    {
        const uint32_t n_rows = (pl.nb + PJ_IPB / 256 - 1) / (PJ_IPB / 256);  // bucketing blocks = record regions = rows of M
        MXG_HIP(h, h->g_part.ensure((size_t)n_rows * (pl.P + 1) * 4));
        MXG_HIP(h, h->g_keys.ensure((size_t)n_rows * PJ_IPB * sizeof(uint4)));
        uint32_t *M = h->g_part.as<uint32_t>();
        uint4 *recs = h->g_keys.as<uint4>();
        hipLaunchKernelGGL(k_pj_bucket, dim3(n_rows), dim3(PJ_BT), (size_t)pl.P * 8, h->stream, pl.as_all, pl.nb, pl.P - 1, M, recs, pl.fsup,
                           pl.n_fsup + pl.n_esup);
        launch_join(recs, M, pl.P, n_rows, nullptr);
        flags_pj();
        return MXG_OK;
    }
    int join_global()
    {
        hipLaunchKernelGGL(k_insert, dim3(pl.nb), dim3(256), 0, h->stream, pl.as_all, h->g_keys.as<Slot>(), pl.mask, pl.cap, pl.fsup,
                           pl.n_fsup + pl.n_esup);
        // flags + shared minimizers per 256 of every assembly (their totals, equal by construction, land in ctl[a])
        hipLaunchKernelGGL(k_flags, dim3(pl.nb), dim3(256), 0, h->stream, pl.as_all, h->g_keys.as<Slot>(), pl.cnt, pl.fsup);
        return MXG_OK;
    }
    // the launches since the last mark went in; fine timing: the span up to here ends at `ev`
    int mark(hipEvent_t ev)
    {
        MXG_HIP(h, hipGetLastError());
        if (fine) MXG_HIP(h, hipEventRecord(ev, h->stream));
        return MXG_OK;
    }

    int vertex_arrays()
    {
        MXG_HIP(h, h->g_vhash.ensure(pl.nvs * 8));
        MXG_HIP(h, h->g_vpos.ensure(anv() * 4));
        MXG_HIP(h, h->g_vrec.ensure(anv() * 4));
        MXG_HIP(h, h->g_fv.ensure(anv() * 4));
        MXG_HIP(h, h->g_frec.ensure(anv() * 4));
        // adj[A][nvs] = {successor, predecessor}: k_adjacency writes every entry that is read -- or, on the rank route, which builds
        // no adj, rank[A][nvs] in the same storage: k_vertices_pj writes every entry below the vertex count of rows 1 .. A - 1
        MXG_HIP(h, h->g_nxt.ensure(2 * anv() * 4));
        if (c.mode == GRAPH_DG_EDGES) MXG_HIP(h, hipMemsetAsync(h->g_nxt.p, 0xFF, 2 * anv() * 4, h->stream));  // messages set single words
        return MXG_OK;
    }
    // GRAPH_DG_VERTICES: where the vertex id of every item of assembly a goes
    int item_vids(uint32_t a, uint32_t **ivid)
    {
        *ivid = nullptr;
        if (c.mode != GRAPH_DG_VERTICES) return MXG_OK;
        MXG_HIP(h, h->asms[a]->d_ivid.ensure((size_t)pl.n_of[a] * 4 + 16));
        *ivid = h->asms[a]->d_ivid.as<uint32_t>();
        return MXG_OK;
    }
    int fill(VertexPjParams &vp)
    {
        vp.as = pl.as_all;
        for (uint32_t a = 0; a < MXG_MAX_ASSEMBLIES; ++a) {
            vp.pos[a] = a < pl.A ? h->asms[a]->d_pos.as<uint32_t>() : nullptr;
            vp.rec[a] = a < pl.A ? h->asms[a]->d_rec.as<uint32_t>() : nullptr;
            vp.ivid[a] = nullptr;
            int rc;
            if (a < pl.A && (rc = item_vids(a, &vp.ivid[a])) != MXG_OK) return rc;
        }
        vp.cnt = pl.cnt;
        vp.sup = pl.fsup;
        vp.n_shared = ctl + CTL_SHARED;
        vp.mask0 = pl.pj_mask0;
        vp.bpref0 = pl.pj_bpref0;
        vp.vhash = h->g_vhash.as<uint64_t>();
        vp.vpos = h->g_vpos.as<uint32_t>();
        vp.vrec = h->g_vrec.as<uint32_t>();
        vp.fv = h->g_fv.as<uint32_t>();
        vp.frec = h->g_frec.as<uint32_t>();
        vp.rank = pl.graph_rank ? h->g_nxt.as<uint32_t>() : nullptr;
        vp.nvs = (uint32_t)pl.nvs;
        return MXG_OK;
    }
    int vertices_pj()  // behind an LDS join
    {
        VertexPjParams vp;
        const int rc = fill(vp);
        if (rc != MXG_OK) return rc;
        hipLaunchKernelGGL(k_block_prefix, dim3((uint32_t)((pl.nb0 + 255) / 256)), dim3(256), 0, h->stream, pl.cnt + pl.as_all.bstart[0],
                           pl.fsup + sup_start(pl.as_all, 0), (uint32_t)pl.nb0, pl.pj_bpref0);
        TAIL_LAUNCH(k_vertices_pj, pl.u_vertices, dim3(graph_tail_grid(pl.nb, pl.u_vertices)), h->stream, vp, pl.nb);
        return MXG_OK;
    }
    int fill(VertexParams &vp, uint32_t a)
    {
        Assembly *as = h->asms[a];
        const size_t row = (size_t)a * pl.nvs;
        vp.flags = as->d_flags.as<uint8_t>();
        vp.cnt = pl.cnt + pl.as_all.bstart[a];
        vp.sup = pl.fsup + sup_start(pl.as_all, a);
        vp.n_shared = ctl + CTL_SHARED + a;
        vp.slot = as->d_slot.as<uint32_t>();
        vp.hash = as->d_hash.as<uint64_t>();
        vp.pos = as->d_pos.as<uint32_t>();
        vp.rec = as->d_rec.as<uint32_t>();
        vp.n = (uint32_t)pl.n_of[a];
        vp.n_ptr = c.gb ? c.gb->n_ptr[a] : nullptr;
        vp.first = a == 0;
        vp.vid = h->g_vid.as<uint32_t>();
        vp.vhash = h->g_vhash.as<uint64_t>();
        vp.vpos = h->g_vpos.as<uint32_t>() + row;
        vp.vrec = h->g_vrec.as<uint32_t>() + row;
        vp.fv = h->g_fv.as<uint32_t>() + row;
        vp.frec = h->g_frec.as<uint32_t>() + row;
        return item_vids(a, &vp.ivid);
    }
    int vertices_global()  // behind the global table: assembly 0 assigns the vertex ids the others look up
    {
        for (uint32_t a = 0; a < pl.A; ++a) {
            VertexParams vp;
            const int rc = fill(vp, a);
            if (rc != MXG_OK) return rc;
            if (vp.ivid) MXG_HIP(h, hipMemsetAsync(vp.ivid, 0xFF, (size_t)vp.n * 4, h->stream));
            hipLaunchKernelGGL(k_vertices, dim3((vp.n + 255) / 256), dim3(256), 0, h->stream, vp);
        }
        return MXG_OK;
    }
    // GRAPH_DG_VERTICES ends here: the caller exchanges vertex ids and adjacency, then calls GRAPH_DG_EDGES.  No host sync: the
    // vertex count stays on the device (ctl[CTL_SHARED]) until then.  (nvs == 0, an assembly without items: no vertex)
    int hand_back_vertices()
    {
        g.nv_stride = pl.nvs;
        if (!c.d_n_vertices) return MXG_OK;
        if (pl.nvs > 0) MXG_HIP(h, hipMemcpyAsync(c.d_n_vertices, ctl + CTL_SHARED, 8, hipMemcpyDeviceToDevice, h->stream));
        else MXG_HIP(h, hipMemsetAsync(c.d_n_vertices, 0, 8, h->stream));
        return MXG_OK;
    }

    void adjacency_own()  // GRAPH_FULL: from the handle's own record order
    {
        TAIL_LAUNCH(k_adjacency, pl.u_edges, dim3(graph_tail_grid((pl.nvs + 255) / 256, pl.u_edges), pl.A), h->stream, h->g_fv.as<uint32_t>(),
                    h->g_frec.as<uint32_t>(), ctl + CTL_SHARED, h->g_nxt.as<uint2>(), (uint32_t)pl.nvs);
    }
    // second half on the owner: every local vertex is an item (fv = identity), adjacency from messages (GRAPH_DG_EDGES) or in place
    void adjacency_of_owner()
    {
        if (c.n_msgs && c.mode == GRAPH_DG_EDGES)
            hipLaunchKernelGGL(k_apply_msgs, dim3((uint32_t)((c.n_msgs + 255) / 256)), dim3(256), 0, h->stream,
                               static_cast<const uint4 *>(c.d_msgs), c.n_msgs, (uint32_t)pl.nvs, h->g_nxt.as<uint32_t>());
        hipLaunchKernelGGL(k_iota_rows, dim3((uint32_t)((pl.nvs + 255) / 256), pl.A), dim3(256), 0, h->stream, h->g_fv.as<uint32_t>(),
                           (uint32_t)pl.nvs);
    }

    void fill(EdgeParams &ep)
    {
        ep.fv = h->g_fv.as<uint32_t>();
        ep.adj = h->g_nxt.as<uint2>();
        ep.frec = h->g_frec.as<uint32_t>();
        ep.rank = h->g_nxt.as<uint32_t>();  // (the rank route: no adj, its storage holds the places)
        ep.nv_ptr = ctl + CTL_SHARED;
        ep.nv = (uint32_t)pl.nvs;
        ep.n_asm = pl.A;
        ep.eflag = h->g_eflag.as<uint8_t>();
        ep.bsum = h->g_ebs.as<uint32_t>();
        ep.bsuper = pl.esup;
        ep.n_edges = ctl + CTL_EDGES;
        ep.host_ctl = hctl;
        ep.eu = h->g_eu.as<uint32_t>();
        ep.ev = h->g_ev.as<uint32_t>();
        ep.esup = h->g_esup.as<uint32_t>();
        ep.ew = h->g_ew.as<double>();
        for (uint32_t a = 0; a < MXG_MAX_ASSEMBLIES; ++a) ep.weights[a] = a < pl.A ? h->asms[a]->weight : 0.0;
    }
    int edges()
    {
        const uint32_t n_items = pl.n_items;
        MXG_HIP(h, h->g_eflag.ensure(n_items));
        MXG_HIP(h, h->g_ebs.ensure((size_t)pl.e_blocks * 4 + 64));
        // every item yields at most one edge: size the edge arrays by that bound
        MXG_HIP(h, h->g_eu.ensure((size_t)n_items * 4));
        MXG_HIP(h, h->g_ev.ensure((size_t)n_items * 4));
        MXG_HIP(h, h->g_esup.ensure((size_t)n_items * 4));
        MXG_HIP(h, h->g_ew.ensure((size_t)n_items * 8));
        EdgeParams ep;
        fill(ep);
        const dim3 grid(graph_tail_grid(pl.e_blocks, pl.u_edges));
        if (pl.graph_rank) {  // from fv, frec and the places k_vertices_pj stored: no k_adjacency in front
            if (pl.A <= 2) TAIL_LAUNCH2(k_edge_flags_rank, pl.u_edges, 1, grid, h->stream, ep, n_items);
            else if (pl.A <= 4) TAIL_LAUNCH2(k_edge_flags_rank, pl.u_edges, 3, grid, h->stream, ep, n_items);
            else TAIL_LAUNCH2(k_edge_flags_rank, pl.u_edges, 0, grid, h->stream, ep, n_items);
            TAIL_LAUNCH(k_edges_rank, pl.u_edges, grid, h->stream, ep, n_items);
        } else {
            TAIL_LAUNCH(k_edge_flags, pl.u_edges, grid, h->stream, ep, n_items);  // + per-256 counts
            TAIL_LAUNCH(k_edges, pl.u_edges, grid, h->stream, ep, n_items);
        }
        MXG_HIP(h, hipGetLastError());
        return MXG_OK;
    }

    // the stage's only sync (results stay in HBM), then: did an LDS join report failure, and what is to be done about it
    int sync_and_verdict()
    {
        if (timing) MXG_HIP(h, hipEventRecord(h->ev1, h->stream));
        MXG_HIP(h, stream_wait(h->stream));
        if (!pl.pj || !hctl[CTL_PJ_FAIL]) return MXG_OK;
        // a partition outgrew its LDS table: redo with the global table ... unless it was a coarse partition's capacity, and only that
        if (!pl.two_level || pl.pj_force_fail) return RC_RETRY_GLOBAL;
        std::vector<uint32_t> cur((size_t)pl.P1 * pl.n_sub * PJ1_CS);
        MXG_HIP(h, hipMemcpy(cur.data(), pl.cursor, cur.size() * 4, hipMemcpyDeviceToHost));
        return join_overflow_verdict(pl, cur.data(), h->pj_learnt);
    }
    int results()
    {
        const uint64_t nv = hctl[CTL_SHARED];
        for (uint32_t a = 1; a < pl.A; ++a)
            if (hctl[CTL_SHARED + a] != nv)
                return set_err(h, MXG_EDEVICE, "internal error: shared-minimizer counts differ between assemblies (%llu vs %llu)",
                               (unsigned long long)hctl[CTL_SHARED + a], (unsigned long long)nv);
        g.nv = nv;
        // (what the next plan for these sizes chooses assembly 0's verdict prefill by)
        if (c.mode == GRAPH_FULL) h->pj_learnt.shared_counted(pl.pre_sig, nv, pl.n_of[0]);
        g.nv_stride = pl.nvs;
        g.ne = pl.nvs > 0 ? hctl[CTL_EDGES] : 0;
        h->stat_unique = ~0ull;  // counted lazily from the flags (mxg_get_stats)
        if (timing) {
            float ms = 0;
            MXG_HIP(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
            h->tm.ms_graph += ms;
            if (fine && pl.nvs > 0) {
                float a = 0, b = 0, c3 = 0;
                MXG_HIP(h, hipEventElapsedTime(&a, h->ev0, h->ev_g[0]));
                MXG_HIP(h, hipEventElapsedTime(&b, h->ev_g[0], h->ev_g[1]));
                MXG_HIP(h, hipEventElapsedTime(&c3, h->ev_g[1], h->ev1));
                h->tm.ms_join += a;
                h->tm.ms_vertices += b;
                h->tm.ms_edges += c3;
            }
        }
        g.valid = true;
        g.own_order = c.mode == GRAPH_FULL;
        g.host_valid = false;
        return MXG_OK;
    }
};

// One attempt.  MXG_OK, an error, or what build_graph is to do about an LDS join that failed (JoinRetry).
static int build_graph_impl(mxg_handle *h, const GraphCall &c, bool global_table)
{
    MXG_HIP(h, hipSetDevice(h->device));
    JoinPlan own;
    const JoinPlan *plan = nullptr;
    int rc = take_or_make_plan(h, c, global_table, own, &plan);
    if (rc != MXG_OK) return rc;
    const JoinPlan &pl = *plan;
    GraphStage s(h, c, pl, plan != &own);
    if ((rc = s.begin()) != MXG_OK) return rc;
    if (s.joins() && (rc = pl.pj ? (pl.two_level ? s.join_two_level() : s.join_one_level()) : s.join_global()) != MXG_OK) return rc;
    if ((rc = s.mark(h->ev_g[0])) != MXG_OK) return rc;
    if (pl.nvs > 0) {
        if ((rc = s.vertex_arrays()) != MXG_OK) return rc;
        if (!s.resume && (rc = pl.pj ? s.vertices_pj() : s.vertices_global()) != MXG_OK) return rc;
    }
    if (c.mode == GRAPH_DG_VERTICES) return s.hand_back_vertices();
    if (pl.nvs > 0) {
        if (c.mode != GRAPH_FULL) s.adjacency_of_owner();
        else if (!pl.graph_rank) s.adjacency_own();  // (the rank route needs no table)
        if ((rc = s.mark(h->ev_g[1])) != MXG_OK) return rc;
        if ((rc = s.edges()) != MXG_OK) return rc;
    }
    if ((rc = s.sync_and_verdict()) != MXG_OK) return rc;
    return s.results();
}

// host mirrors are filled on demand (mxg_get_graph, mxg_write_dot, mxg_get_mx_flags)
int graph_to_host(mxg_handle *h)
{
    Graph &g = h->graph;
    if (!g.valid) return set_err(h, MXG_EINVAL, "call mxg_build_graph first");
    if (g.host_valid) return MXG_OK;
    MXG_HIP(h, hipSetDevice(h->device));
    const size_t anv = (size_t)g.n_asm * g.nv;
    int rc;
    // the host mirrors (a quarter of a gigabyte at 3 Gbp + 3 Gbp) are sized -- zero-filled, i.e. their pages are touched -- by one
    // thread per array before the copies are issued: one thread doing it in front of each copy took 30 of this function's 47 ms
    {
        std::vector<std::thread> th;
        auto sized = [](auto &v, size_t n) {  // (out of memory in a helper: the copy below sizes the array in this thread and reports)
            try {
                v.resize(n);
            } catch (const std::bad_alloc &) {
            }
        };
        try {
            th.emplace_back([&] { sized(g.vhash, g.nv); });
            th.emplace_back([&] { sized(g.vpos, anv); });
            th.emplace_back([&] { sized(g.vrec, anv); });
            th.emplace_back([&] { sized(g.eu, g.ne); });
            th.emplace_back([&] { sized(g.ev, g.ne); });
            th.emplace_back([&] { sized(g.esup, g.ne); });
            sized(g.ew, g.ne);
        } catch (const std::system_error &) {  // (no thread to be had: the copies below size what is left)
        }
        for (auto &t : th) t.join();
    }
    if ((rc = d2h(h, g.vhash, h->g_vhash.p, g.nv)) != MXG_OK) return rc;
    g.vpos.resize(anv);
    g.vrec.resize(anv);
    for (uint32_t a = 0; a < g.n_asm && g.nv; ++a) {  // device arrays are strided by nv_stride, host mirrors are compact
        MXG_HIP(h, hipMemcpyAsync(g.vpos.data() + (size_t)a * g.nv, h->g_vpos.as<uint32_t>() + (size_t)a * g.nv_stride,
                                  g.nv * 4, hipMemcpyDeviceToHost, h->stream));
        MXG_HIP(h, hipMemcpyAsync(g.vrec.data() + (size_t)a * g.nv, h->g_vrec.as<uint32_t>() + (size_t)a * g.nv_stride,
                                  g.nv * 4, hipMemcpyDeviceToHost, h->stream));
    }
    if ((rc = d2h(h, g.eu, h->g_eu.p, g.ne)) != MXG_OK) return rc;
    if ((rc = d2h(h, g.ev, h->g_ev.p, g.ne)) != MXG_OK) return rc;
    if ((rc = d2h(h, g.esup, h->g_esup.p, g.ne)) != MXG_OK) return rc;
    if ((rc = d2h(h, g.ew, h->g_ew.p, g.ne)) != MXG_OK) return rc;
    MXG_HIP(h, hipStreamSynchronize(h->stream));
    g.host_valid = true;
    return MXG_OK;
}

int flags_to_host(mxg_handle *h, Assembly *a)
{
    // (flags also arrive from the owners of the distributed graph stage, without a graph on this handle)
    if (!a->flags_valid) return set_err(h, MXG_EINVAL, "call mxg_build_graph first");
    if (a->flags_on_host) return MXG_OK;
    MXG_HIP(h, hipSetDevice(h->device));
    int rc = d2h(h, a->h_flags, a->d_flags.p, a->n_mx);
    if (rc != MXG_OK) return rc;
    MXG_HIP(h, hipStreamSynchronize(h->stream));
    a->flags_on_host = true;
    return MXG_OK;
}

}  // namespace mxg
