// adjust.hip -- the path adjustment stage (mxg_adjust_paths): what ntJoin does to the paths between format_path and the trimming /
// printing of the scaffolds (reference bin/ntjoin_assemble.py:751-786): merged relocations, --no_cut, overlapping regions.
//
// Seven phases, in the reference's order.  Everything but a few per-path steps depends only on the nodes of ONE
// target contig, taken in (path, node) order: the contig's set of incorporated segments, the merge chains (a chain reads and writes
// only its contig's set), the intersection counts, OverlapRegion.find_non_overlapping, contig_regions and is_best_region.  So the
// node indices are grouped by record (counts -> scan -> scatter, order restored inside each record's short list) and every record
// with at least two nodes gets one wave; records with one node never get one.  Inside the wave the membership, "is a foreign
// segment in the way" and "how many segments does this one intersect" tests run across the lanes (lists longer than 64: strided)
// and are reduced by ballot / popcount; the chain walk and find_non_overlapping's sweeps are sequential and run uniformly (writes by
// lane 0).  The per-path steps (links between the nodes a path still holds, is_subsumed's neighbour test, the gap accumulated onto
// the last kept node, the terminal gap, the final compaction) are one thread per path or node.
//
// Nodes keep their input index throughout: a node that leaves its path (merged into the head of its chain, subsumed, dropped) only
// loses its `alive` flag, and k_adj_link rebuilds the previous / next links of every path from the flags.  One ordered compaction at
// the end (scan_kernels.h) makes the output.  Host syncs: one for the number of records that get a wave, one for the results.
#include <algorithm>

#include "mxg_internal.h"
#include "scan_kernels.h"

namespace mxg {

namespace {

constexpr uint32_t ADJ_NONE = 0xFFFFFFFFu;
constexpr unsigned long long ADJ_NO_ERR = ~0ull;
constexpr uint32_t ADJ_MAX_RECORDS = 1u << 28;
constexpr uint32_t ADJ_MAX_SWEEPS = 1u << 20;  // find_non_overlapping: every sweep that finds an overlap shrinks or drops a region
enum : uint32_t { ADJ_LIMIT_SET = 1, ADJ_LIMIT_SWEEPS = 2, ADJ_LIMIT_COORD = 4 };

enum AdjBuf {
    AJ_NODES, AJ_PATH_FIRST, AJ_PATH_OF, AJ_PRV, AJ_NXT, AJ_POS, AJ_PATH_LEN, AJ_FLAGS, AJ_HEADOF, AJ_REC_CNT, AJ_REC_FIRST, AJ_REC_CURSOR,
    AJ_REC_NODES, AJ_REC_TMP, AJ_CREG_CNT, AJ_ACTIVE, AJ_CTL, AJ_SET, AJ_SET_N, AJ_MAP_B, AJ_MAP_A, AJ_MAP_NONE, AJ_MAP_N, AJ_ORD, AJ_SNAP,
    AJ_BSUM, AJ_OUT_FIRST, AJ_OUT_NODES, AJ_OUT_SRC, AJ_N
};
static_assert(AJ_N <= 32, "mxg_handle::adjbuf");

// everything the kernels read and write, by value
struct Adj {
    mxg_adjust_node *nd;
    uint32_t n_nodes, n_paths, n_rec;
    const uint64_t *path_first;
    uint32_t *path_of, *prv, *nxt, *pos, *path_len;  // links among the nodes a path still holds; pos = index in that path
    uint8_t *alive, *tallied, *creg, *sub, *drop;
    uint32_t *headof;                                // a merged node's chain head (within one merge pass)
    uint32_t *rec_cnt, *rec_first, *rec_cursor, *rec_nodes, *rec_tmp, *creg_cnt;
    uint32_t *active;
    // per record r an area of rec_cnt[r] + 1 entries at rec_first[r] + r in each of these
    uint32_t *set_s, *set_e, *map_bs, *map_be, *ord;
    int64_t *map_as, *map_ae, *snap_s, *snap_e;
    uint8_t *map_none;
    uint32_t *set_n, *map_n;  // per record
    // ctl[0] = first KeyError as (phase << 32 | input node), ctl[1] = ADJ_LIMIT_* bits, ctl[2] = records that get a wave
    unsigned long long *ctl;
    uint32_t no_cut;
    int64_t G;
};

__device__ __forceinline__ bool adj_stop(const Adj &A, uint32_t phase) { return (A.ctl[0] >> 32) < phase || A.ctl[1] != 0; }

// ---- grouping ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_adj_init(Adj A)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= A.n_paths) return;
    const uint32_t lo = (uint32_t)A.path_first[p], hi = (uint32_t)A.path_first[p + 1];
    for (uint32_t i = lo; i < hi; ++i) {
        A.path_of[i] = p;
        A.tallied[i] = hi - lo >= 2u;
    }
}

__global__ __launch_bounds__(256) void k_adj_count(Adj A)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < A.n_nodes) atomicAdd(&A.rec_cnt[A.nd[i].record], 1u);
}

__global__ __launch_bounds__(256) void k_adj_scatter(Adj A)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n_nodes) return;
    const uint32_t r = A.nd[i].record;
    A.rec_nodes[A.rec_first[r] + atomicAdd(&A.rec_cursor[r], 1u)] = i;
}

__global__ __launch_bounds__(256) void k_adj_active(Adj A)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= A.n_rec) return;
    const uint32_t c = A.rec_cnt[r];
    A.creg_cnt[r] = c;
    if (c >= 2u) A.active[(uint32_t)atomicAdd(&A.ctl[2], 1ull)] = r;
}

// ---- per path ----------------------------------------------------------------------------------------------------------------------
// previous / next / position of every node its path still holds; kill (if given): nodes that leave their paths first
__global__ __launch_bounds__(256) void k_adj_link(Adj A, const uint8_t *kill)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= A.n_paths) return;
    const uint32_t lo = (uint32_t)A.path_first[p], hi = (uint32_t)A.path_first[p + 1];
    uint32_t last = ADJ_NONE, n = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        if (kill && kill[i]) A.alive[i] = 0;
        if (!A.alive[i]) continue;
        A.prv[i] = last;
        A.nxt[i] = ADJ_NONE;
        A.pos[i] = n++;
        if (last != ADJ_NONE) A.nxt[last] = i;
        last = i;
    }
    A.path_len[p] = n;
}

// is_subsumed (:253-264): a node between two nodes of one other contig that together span it, that contig being in two nodes overall
__global__ __launch_bounds__(256) void k_adj_subsumed(Adj A)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n_nodes) return;
    uint8_t s = 0;
    if (!adj_stop(A, 3) && A.alive[i] && A.prv[i] != ADJ_NONE && A.nxt[i] != ADJ_NONE) {
        const mxg_adjust_node &a = A.nd[A.prv[i]], &b = A.nd[A.nxt[i]];
        s = a.record == b.record && a.ori == b.ori && min(a.start, b.start) == 0u && max(a.end, b.end) == a.contig_size &&
            A.creg_cnt[a.record] == 2u;
    }
    A.sub[i] = s;
}

// adjust_paths' second loop for the contigs that are in one node overall and never get a wave: widened to the whole contig
__global__ __launch_bounds__(256) void k_adj_single(Adj A)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n_nodes || !A.alive[i] || adj_stop(A, 4)) return;
    mxg_adjust_node &a = A.nd[i];
    if (A.rec_cnt[a.record] != 1u) return;
    if (a.end - a.start < a.contig_size) {
        a.start = 0;
        a.end = a.contig_size;
    }
}

// ... and its gap rule: a node that is not its contig's best region leaves the path; strictly inside the path, and with a kept node in
// front of it, its length goes onto that node's gap (clamped to G at every step)
__global__ __launch_bounds__(256) void k_adj_gap(Adj A)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= A.n_paths || adj_stop(A, 4)) return;
    const uint32_t lo = (uint32_t)A.path_first[p], hi = (uint32_t)A.path_first[p + 1], len = A.path_len[p];
    uint32_t kept = ADJ_NONE;
    for (uint32_t i = lo; i < hi; ++i) {
        if (!A.alive[i]) continue;
        if (!A.drop[i]) {
            kept = i;
            continue;
        }
        const uint32_t at = A.pos[i];
        if (at > 0u && at + 1u < len && kept != ADJ_NONE) {
            int64_t g = A.nd[kept].gap_size + ((int64_t)A.nd[i].end - (int64_t)A.nd[i].start);
            if (A.G > 0) g = min(A.G, g);
            A.nd[kept].gap_size = g;
        }
        A.alive[i] = 0;
    }
}

// remove_overlapping_regions (:451-466): a node whose exact (start, end) is in its contig's table is dropped or takes the replacement
__global__ __launch_bounds__(256) void k_adj_lookup(Adj A)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n_nodes || !A.alive[i] || adj_stop(A, 6)) return;
    mxg_adjust_node &a = A.nd[i];
    const uint32_t r = a.record, m = A.map_n[r];
    if (!m) return;
    const uint32_t base = A.rec_first[r] + r;
    for (uint32_t q = 0; q < m; ++q) {
        if (A.map_bs[base + q] != a.start || A.map_be[base + q] != a.end) continue;
        if (A.map_none[base + q]) {
            A.alive[i] = 0;
        } else {
            const int64_t s = A.map_as[base + q], e = A.map_ae[base + q];
            if (s < 0 || e < 0 || s > 0xFFFFFFFFll || e > 0xFFFFFFFFll) {
                atomicOr(&A.ctl[1], (unsigned long long)ADJ_LIMIT_COORD);
            } else {
                a.start = (uint32_t)s;
                a.end = (uint32_t)e;
            }
        }
        return;
    }
}

// check_terminal_node_gap_zero (:441-448), and how many nodes every path ends with
__global__ __launch_bounds__(256) void k_adj_final(Adj A, uint32_t *out_cnt)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p > A.n_paths) return;
    if (p == A.n_paths) {
        out_cnt[p] = 0;
        return;
    }
    const uint32_t lo = (uint32_t)A.path_first[p], hi = (uint32_t)A.path_first[p + 1];
    uint32_t n = 0, last = ADJ_NONE;
    for (uint32_t i = lo; i < hi; ++i) {
        if (!A.alive[i]) continue;
        ++n;
        if (A.nd[i].ori != 2) last = i;
    }
    if (last != ADJ_NONE && !adj_stop(A, 7)) A.nd[last].gap_size = 0;
    out_cnt[p] = n;
}

__global__ __launch_bounds__(256) void k_adj_emit(Adj A, const uint32_t *out_first, mxg_adjust_node *out_nodes, uint64_t *out_src)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= A.n_paths) return;
    const uint32_t lo = (uint32_t)A.path_first[p], hi = (uint32_t)A.path_first[p + 1];
    uint32_t at = out_first[p];
    for (uint32_t i = lo; i < hi; ++i) {
        if (!A.alive[i]) continue;
        out_nodes[at] = A.nd[i];
        out_src[at++] = i;
    }
}

// ---- per record: one wave ----------------------------------------------------------------------------------------------------------
// a record's view of its areas; every function below is called by all 64 lanes with the same arguments (writes: lane 0, then a barrier)
struct AdjRec {
    uint32_t r, lo, n, base, cap, ns;
};

__device__ __forceinline__ uint32_t adj_set_find(const Adj &A, const AdjRec &R, uint32_t s, uint32_t e)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = 0; c < R.ns; c += 64u) {
        const uint32_t q = c + lane;
        const bool hit = q < R.ns && A.set_s[R.base + q] == s && A.set_e[R.base + q] == e;
        const unsigned long long b = __ballot(hit);
        if (b) return c + (uint32_t)__ffsll((long long)b) - 1u;
    }
    return ADJ_NONE;
}

__device__ __forceinline__ bool adj_set_add(const Adj &A, AdjRec &R, uint32_t s, uint32_t e)
{
    if (adj_set_find(A, R, s, e) != ADJ_NONE) return true;
    if (R.ns >= R.cap) return false;
    if (threadIdx.x == 0) {
        A.set_s[R.base + R.ns] = s;
        A.set_e[R.base + R.ns] = e;
    }
    ++R.ns;
    __syncthreads();
    return true;
}

__device__ __forceinline__ bool adj_set_remove(const Adj &A, AdjRec &R, uint32_t s, uint32_t e)
{
    const uint32_t q = adj_set_find(A, R, s, e);
    if (q == ADJ_NONE) return false;
    --R.ns;
    if (threadIdx.x == 0) {
        A.set_s[R.base + q] = A.set_s[R.base + R.ns];
        A.set_e[R.base + q] = A.set_e[R.base + R.ns];
    }
    __syncthreads();
    return true;
}

// is_new_region_overlapping (:115-123)
__device__ __forceinline__ bool adj_blocked(const Adj &A, const AdjRec &R, uint32_t start, uint32_t end, uint32_t is, uint32_t ie, uint32_t js,
                                            uint32_t je)
{
    bool hit = false;
    for (uint32_t q = threadIdx.x; q < R.ns; q += 64u) {
        const uint32_t s = A.set_s[R.base + q], e = A.set_e[R.base + q];
        hit = hit || (start <= e && s <= end && s != is && e != ie && s != js && e != je);
    }
    return __ballot(hit) != 0ull;
}

// merge_relocations (:126-172) for every chain of the record, in (path, node) order; false: a KeyError (recorded)
__device__ bool adj_merge_pass(const Adj &A, AdjRec &R, uint32_t phase)
{
    const bool w = threadIdx.x == 0;
    for (uint32_t k = 0; k < R.n; ++k) {
        const uint32_t j = A.rec_nodes[R.lo + k];
        if (!A.alive[j]) continue;
        const uint32_t i = A.prv[j];
        if (i == ADJ_NONE || A.nd[i].record != R.r) continue;
        const uint32_t head = A.alive[i] ? i : A.headof[i];
        const uint32_t oi = A.nd[i].ori, oj = A.nd[j].ori;
        const uint32_t is = A.nd[i].start, ie = A.nd[i].end, js = A.nd[j].start, je = A.nd[j].end;
        const uint32_t hs = A.nd[head].start, he = A.nd[head].end;
        const bool plus = oi == 0u && oj == 0u && ie <= js, minus = oi == 1u && oj == 1u && is >= je;
        if (!plus && !minus) continue;
        if (plus ? adj_blocked(A, R, is, je, is, ie, js, je) : adj_blocked(A, R, js, ie, is, ie, js, je)) continue;
        bool ok = plus ? adj_set_add(A, R, hs, je) : adj_set_add(A, R, js, he);
        if (!ok) {
            if (w) atomicOr(&A.ctl[1], (unsigned long long)ADJ_LIMIT_SET);
            return false;
        }
        ok = adj_set_remove(A, R, hs, he) && adj_set_remove(A, R, js, je);
        if (!ok) {
            if (w) atomicMin(&A.ctl[0], ((unsigned long long)phase << 32) | j);
            return false;
        }
        if (w) {
            mxg_adjust_node &h = A.nd[head];
            if (plus) {
                h.end = je;
                h.terminal_mx = A.nd[j].terminal_mx;
            } else {
                h.start = js;
                h.first_mx = A.nd[j].first_mx;
            }
            h.gap_size = A.nd[j].gap_size;
            A.alive[j] = 0;
            A.headof[j] = head;
        }
        __syncthreads();
    }
    return true;
}

__device__ __forceinline__ AdjRec adj_rec(const Adj &A)
{
    AdjRec R;
    R.r = A.active[blockIdx.x];
    R.lo = A.rec_first[R.r];
    R.n = A.rec_cnt[R.r];
    R.base = R.lo + R.r;
    R.cap = R.n + 1u;
    R.ns = A.set_n[R.r];
    return R;
}

// phases 1 and 2: the record's list in node order, its set of incorporated segments, the first merge pass
__global__ __launch_bounds__(64) void k_adj_rec_first(Adj A)
{
    AdjRec R = adj_rec(A);
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = lane; k < R.n; k += 64u) {  // the scatter left the list in any order: rank by counting
        const uint32_t v = A.rec_nodes[R.lo + k];
        uint32_t rank = 0;
        for (uint32_t q = 0; q < R.n; ++q) rank += A.rec_nodes[R.lo + q] < v;
        A.rec_tmp[R.lo + rank] = v;
    }
    __syncthreads();
    for (uint32_t k = lane; k < R.n; k += 64u) A.rec_nodes[R.lo + k] = A.rec_tmp[R.lo + k];
    __syncthreads();
    R.ns = 0;
    for (uint32_t k = 0; k < R.n; ++k) {  // tally_incorporated_segments (:220-230): a set, so equal segments collapse
        const uint32_t i = A.rec_nodes[R.lo + k];
        if (A.tallied[i]) adj_set_add(A, R, A.nd[i].start, A.nd[i].end);  // (at most n entries: never full)
    }
    adj_merge_pass(A, R, 2);
    uint32_t c = 0;
    for (uint32_t k = lane; k < R.n; k += 64u) {  // contig_regions of adjust_paths: the nodes the paths hold now
        const uint32_t i = A.rec_nodes[R.lo + k];
        A.creg[i] = A.alive[i];
        c += A.alive[i];
    }
    c = wave_sum_u32(c);
    if (lane == 0) {
        A.set_n[R.r] = R.ns;
        A.creg_cnt[R.r] = c;
    }
}

// phase 3, first loop: the merge pass over the paths without their subsumed nodes
__global__ __launch_bounds__(64) void k_adj_rec_merge(Adj A, uint32_t phase)
{
    if (adj_stop(A, phase)) return;
    AdjRec R = adj_rec(A);
    adj_merge_pass(A, R, phase);
    if (threadIdx.x == 0) A.set_n[R.r] = R.ns;
}

// phase 3, second loop (:284-304) for the record's nodes in (path, node) order: is_best_region (:233-244) looks at all of
// contig_regions, merged and subsumed nodes included, as they are now -- the widened nodes of earlier steps among them
__global__ __launch_bounds__(64) void k_adj_rec_best(Adj A)
{
    if (adj_stop(A, 4)) return;
    const AdjRec R = adj_rec(A);
    const uint32_t lane = threadIdx.x, c = A.creg_cnt[R.r];
    for (uint32_t k = 0; k < R.n; ++k) {
        const uint32_t i = A.rec_nodes[R.lo + k];
        if (!A.alive[i]) continue;
        const uint32_t len = A.nd[i].end - A.nd[i].start, size = A.nd[i].contig_size;
        bool widen = false, drop = false;
        if (c > 1u) {
            unsigned long long best = 0;  // (length << 32 | ~list index): the first of the longest
            for (uint32_t q = lane; q < R.n; q += 64u) {
                const uint32_t m = A.rec_nodes[R.lo + q];
                if (!A.creg[m]) continue;
                const uint32_t l = A.nd[m].end - A.nd[m].start;
                if (l) best = max(best, ((unsigned long long)l << 32) | (0xFFFFFFFFu - q));
            }
            for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned long long)__shfl_xor((long long)best, o, 64));
            widen = best != 0ull && (uint32_t)(best >> 32) == len &&
                    A.nd[A.rec_nodes[R.lo + (0xFFFFFFFFu - (uint32_t)best)]].terminal_mx == A.nd[i].terminal_mx;
            drop = !widen;
        } else if (c == 1u) {
            widen = len < size;
        }
        if (lane == 0) {
            if (widen) {
                A.nd[i].start = 0;
                A.nd[i].end = size;
            }
            if (drop) A.drop[i] = 1;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ bool adj_closed_overlap(int64_t s1, int64_t e1, int64_t s2, int64_t e2) { return s1 <= e2 && s2 <= e1; }
__device__ __forceinline__ bool adj_inside(int64_t s1, int64_t e1, int64_t s2, int64_t e2) { return s1 >= s2 && e1 <= e2; }

// OverlapRegion.find_non_overlapping (bin/overlap_region.py:32-91) on the m regions of the record's table, ascending: one lane
__device__ void adj_find_non_overlapping(const Adj &A, const AdjRec &R, uint32_t m)
{
    uint32_t *bs = A.map_bs + R.base, *be = A.map_be + R.base, *ord = A.ord + R.base;
    int64_t *as = A.map_as + R.base, *ae = A.map_ae + R.base, *ss = A.snap_s + R.base, *se = A.snap_e + R.base;
    uint8_t *none = A.map_none + R.base;
    uint32_t best = 0;
    for (uint32_t q = 1; q < m; ++q)
        if (be[q] - bs[q] > be[best] - bs[best]) best = q;
    const int64_t b0 = bs[best], b1 = be[best];
    for (uint32_t q = 0; q < m; ++q) {
        const int64_t s = bs[q], e = be[q];
        as[q] = s;
        ae[q] = e;
        none[q] = 0;
        if (q == best) continue;
        if (adj_inside(s, e, b0, b1)) {
            none[q] = 1;
        } else if (adj_closed_overlap(s, e, b0, b1)) {
            if (s <= b0) ae[q] = b0 - 1;
            else as[q] = b1 + 1;
        }
    }
    for (uint32_t sweep = 0;; ++sweep) {
        if (sweep == ADJ_MAX_SWEEPS) {
            atomicOr(&A.ctl[1], (unsigned long long)ADJ_LIMIT_SWEEPS);
            return;
        }
        uint32_t n = 0;
        for (uint32_t q = 0; q < m; ++q) {  // stable insertion sort by the replacement, of the regions that still have one
            if (none[q]) continue;
            uint32_t at = n++;
            while (at > 0u && (as[ord[at - 1]] > as[q] || (as[ord[at - 1]] == as[q] && ae[ord[at - 1]] > ae[q]))) {
                ord[at] = ord[at - 1];
                --at;
            }
            ord[at] = q;
        }
        for (uint32_t u = 0; u < n; ++u) {  // the sweep compares the values it started with
            ss[u] = as[ord[u]];
            se[u] = ae[ord[u]];
        }
        bool again = false;
        for (uint32_t u = 0; u + 1u < n; ++u) {
            const int64_t s1 = ss[u], e1 = se[u], s2 = ss[u + 1], e2 = se[u + 1];
            if (!adj_closed_overlap(s1, e1, s2, e2)) continue;
            again = true;
            const uint32_t q1 = ord[u], q2 = ord[u + 1];
            if (adj_inside(s1, e1, s2, e2)) {
                none[q1] = 1;
            } else if (adj_inside(s2, e2, s1, e1)) {
                none[q2] = 1;
            } else if (e1 - s1 > e2 - s2) {
                none[q2] = 0;
                as[q2] = e1 + 1;
                ae[q2] = e2;
            } else {
                none[q1] = 0;
                as[q1] = s1;
                ae[q1] = s2 - 1;
            }
        }
        if (!again) return;
    }
}

// phases 4 and 5: the segments that intersect another one (bedtools: max(starts) < min(ends)), ascending by (start, end), and what
// becomes of them; then the second merge pass
__global__ __launch_bounds__(64) void k_adj_rec_last(Adj A)
{
    if (adj_stop(A, 4)) return;
    AdjRec R = adj_rec(A);
    const uint32_t lane = threadIdx.x;
    uint32_t m = 0;
    for (uint32_t a = 0; a < R.ns; ++a) {
        const uint32_t s = A.set_s[R.base + a], e = A.set_e[R.base + a];
        uint32_t c = 0;
        for (uint32_t q = lane; q < R.ns; q += 64u) c += max(s, A.set_s[R.base + q]) < min(e, A.set_e[R.base + q]);
        if (wave_sum_u32(c) > 1u) {
            if (lane == 0) {
                A.map_bs[R.base + m] = s;
                A.map_be[R.base + m] = e;
            }
            ++m;
        }
    }
    __syncthreads();
    if (m) {
        if (lane == 0) {
            uint32_t *bs = A.map_bs + R.base, *be = A.map_be + R.base;
            for (uint32_t q = 1; q < m; ++q) {  // the set holds its segments in any order
                const uint32_t s = bs[q], e = be[q];
                uint32_t at = q;
                while (at > 0u && (bs[at - 1] > s || (bs[at - 1] == s && be[at - 1] > e))) {
                    bs[at] = bs[at - 1];
                    be[at] = be[at - 1];
                    --at;
                }
                bs[at] = s;
                be[at] = e;
            }
            adj_find_non_overlapping(A, R, m);
            A.map_n[R.r] = m;
        }
        __syncthreads();
    }
    adj_merge_pass(A, R, 5);
}

uint32_t blocks_of(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, (n + 255) / 256); }

}  // namespace

int adjust_paths(mxg_handle *h, const mxg_adjust_node *nodes, const uint64_t *path_first, uint64_t n_paths, const mxg_adjust_params &p)
{
    h->adj_nodes.clear();
    h->adj_source.clear();
    h->adj_first.assign(n_paths + 1, 0);
    if (n_paths && path_first[0] != 0) return set_err(h, MXG_EINVAL, "mxg_adjust_paths: path_first does not begin with 0");
    const uint64_t n_nodes = n_paths ? path_first[n_paths] : 0;
    if (n_nodes >= 0x7FFFFFFFull || n_paths >= 0x7FFFFFFFull)
        return set_err(h, MXG_ELIMIT, "mxg_adjust_paths: %llu nodes in %llu paths (at most 2^31 - 2 of either)", (unsigned long long)n_nodes,
                       (unsigned long long)n_paths);
    uint32_t max_rec = 0;
    for (uint64_t q = 0; q < n_paths; ++q) {
        const uint64_t lo = path_first[q], hi = path_first[q + 1];
        if (hi < lo || hi > n_nodes) return set_err(h, MXG_EINVAL, "mxg_adjust_paths: path_first is not increasing at path %llu", (unsigned long long)q);
        for (uint64_t i = lo; i < hi; ++i) {
            const mxg_adjust_node &in = nodes[i];
            const unsigned long long up = q, un = i - lo;
            if (in.ori > 2) return set_err(h, MXG_EINVAL, "mxg_adjust_paths: path %llu node %llu: ori %u is none of 0 '+', 1 '-', 2 '?'", up, un, in.ori);
            if (in.start >= in.end)
                return set_err(h, MXG_EINVAL, "mxg_adjust_paths: path %llu node %llu: [%u, %u) holds no base", up, un, in.start, in.end);
            if (in.record >= ADJ_MAX_RECORDS)
                return set_err(h, MXG_ELIMIT, "mxg_adjust_paths: path %llu node %llu: record %u (at most 2^28 - 1)", up, un, in.record);
            max_rec = std::max(max_rec, in.record);
        }
    }
    if (n_nodes == 0) return MXG_OK;
    const uint32_t N = (uint32_t)n_nodes, P = (uint32_t)n_paths, R = max_rec + 1u;
    const size_t area = (size_t)N + R;
    MXG_HIP(h, hipSetDevice(h->device));
    DevBuf *B = h->adjbuf;
    const uint32_t scan_n = std::max(R, P) + 1u, tiles = (scan_n + TILE - 1) / TILE;
    const size_t need[AJ_N] = {
        /*NODES*/ N * sizeof(mxg_adjust_node), /*PATH_FIRST*/ (P + 1ull) * 8, /*PATH_OF*/ N * 4ull, /*PRV*/ N * 4ull, /*NXT*/ N * 4ull,
        /*POS*/ N * 4ull, /*PATH_LEN*/ (P + 1ull) * 4, /*FLAGS*/ N * 5ull, /*HEADOF*/ N * 4ull, /*REC_CNT*/ (R + 1ull) * 4,
        /*REC_FIRST*/ (R + 1ull) * 4, /*REC_CURSOR*/ R * 4ull, /*REC_NODES*/ N * 4ull, /*REC_TMP*/ N * 4ull, /*CREG_CNT*/ R * 4ull,
        /*ACTIVE*/ R * 4ull, /*CTL*/ 32, /*SET*/ area * 8, /*SET_N*/ R * 4ull, /*MAP_B*/ area * 8, /*MAP_A*/ area * 16, /*MAP_NONE*/ area,
        /*MAP_N*/ R * 4ull, /*ORD*/ area * 4, /*SNAP*/ area * 16, /*BSUM*/ (tiles + 1ull) * 4 + 16, /*OUT_FIRST*/ (P + 1ull) * 4,
        /*OUT_NODES*/ N * sizeof(mxg_adjust_node), /*OUT_SRC*/ N * 8ull};
    for (int b = 0; b < AJ_N; ++b) MXG_HIP(h, B[b].ensure(need[b] + 16));
    Adj A{};
    A.nd = B[AJ_NODES].as<mxg_adjust_node>();
    A.n_nodes = N;
    A.n_paths = P;
    A.n_rec = R;
    A.path_first = B[AJ_PATH_FIRST].as<uint64_t>();
    A.path_of = B[AJ_PATH_OF].as<uint32_t>();
    A.prv = B[AJ_PRV].as<uint32_t>();
    A.nxt = B[AJ_NXT].as<uint32_t>();
    A.pos = B[AJ_POS].as<uint32_t>();
    A.path_len = B[AJ_PATH_LEN].as<uint32_t>();
    A.alive = B[AJ_FLAGS].as<uint8_t>();
    A.tallied = A.alive + N;
    A.creg = A.tallied + N;
    A.sub = A.creg + N;
    A.drop = A.sub + N;
    A.headof = B[AJ_HEADOF].as<uint32_t>();
    A.rec_cnt = B[AJ_REC_CNT].as<uint32_t>();
    A.rec_first = B[AJ_REC_FIRST].as<uint32_t>();
    A.rec_cursor = B[AJ_REC_CURSOR].as<uint32_t>();
    A.rec_nodes = B[AJ_REC_NODES].as<uint32_t>();
    A.rec_tmp = B[AJ_REC_TMP].as<uint32_t>();
    A.creg_cnt = B[AJ_CREG_CNT].as<uint32_t>();
    A.active = B[AJ_ACTIVE].as<uint32_t>();
    A.ctl = B[AJ_CTL].as<unsigned long long>();
    A.set_s = B[AJ_SET].as<uint32_t>();
    A.set_e = A.set_s + area;
    A.set_n = B[AJ_SET_N].as<uint32_t>();
    A.map_bs = B[AJ_MAP_B].as<uint32_t>();
    A.map_be = A.map_bs + area;
    A.map_as = B[AJ_MAP_A].as<int64_t>();
    A.map_ae = A.map_as + area;
    A.map_none = B[AJ_MAP_NONE].as<uint8_t>();
    A.map_n = B[AJ_MAP_N].as<uint32_t>();
    A.ord = B[AJ_ORD].as<uint32_t>();
    A.snap_s = B[AJ_SNAP].as<int64_t>();
    A.snap_e = A.snap_s + area;
    A.no_cut = p.no_cut;
    A.G = p.G;
    uint32_t *bsum = B[AJ_BSUM].as<uint32_t>();
    uint64_t *scan_total = reinterpret_cast<uint64_t *>(A.ctl + 3);
    hipStream_t st = h->stream;
    MXG_HIP(h, hipMemcpyAsync(A.nd, nodes, N * sizeof(mxg_adjust_node), hipMemcpyHostToDevice, st));
    MXG_HIP(h, hipMemcpyAsync(B[AJ_PATH_FIRST].p, path_first, (P + 1ull) * 8, hipMemcpyHostToDevice, st));
    const unsigned long long ctl0[4] = {ADJ_NO_ERR, 0, 0, 0};
    MXG_HIP(h, hipMemcpyAsync(A.ctl, ctl0, sizeof ctl0, hipMemcpyHostToDevice, st));
    MXG_HIP(h, hipMemsetAsync(A.alive, 1, N, st));
    MXG_HIP(h, hipMemsetAsync(A.tallied, 0, 4ull * N, st));
    MXG_HIP(h, hipMemsetAsync(A.rec_cnt, 0, (R + 1ull) * 4, st));
    MXG_HIP(h, hipMemsetAsync(A.rec_cursor, 0, R * 4ull, st));
    MXG_HIP(h, hipMemsetAsync(A.set_n, 0, R * 4ull, st));
    MXG_HIP(h, hipMemsetAsync(A.map_n, 0, R * 4ull, st));
    // ---- group the nodes by record; the records with two nodes or more
    hipLaunchKernelGGL(k_adj_init, dim3(blocks_of(P)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_adj_link, dim3(blocks_of(P)), dim3(256), 0, st, A, (const uint8_t *)nullptr);
    hipLaunchKernelGGL(k_adj_count, dim3(blocks_of(N)), dim3(256), 0, st, A);
    launch_scan_u32(st, A.rec_cnt, R + 1u, bsum, A.rec_first, scan_total);  // (R + 1 entries: the last is the total)
    hipLaunchKernelGGL(k_adj_scatter, dim3(blocks_of(N)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_adj_active, dim3(blocks_of(R)), dim3(256), 0, st, A);
    MXG_HIP(h, hipGetLastError());
    // (the two copies into locals below are synchronous for the caller: each is followed by its sync before anything else can fail)
    unsigned long long ctl[3] = {0, 0, 0};
    hipError_t e_copy = hipMemcpyAsync(ctl, A.ctl, sizeof ctl, hipMemcpyDeviceToHost, st);
    const hipError_t e_sync1 = hipStreamSynchronize(st);  // sync 1: how many records get a wave
    MXG_HIP(h, e_copy);
    MXG_HIP(h, e_sync1);
    const uint32_t n_active = (uint32_t)ctl[2];
    // ---- phases 1 and 2
    if (n_active) hipLaunchKernelGGL(k_adj_rec_first, dim3(n_active), dim3(64), 0, st, A);
    hipLaunchKernelGGL(k_adj_link, dim3(blocks_of(P)), dim3(256), 0, st, A, (const uint8_t *)nullptr);
    // ---- phase 3
    if (p.no_cut) {
        hipLaunchKernelGGL(k_adj_subsumed, dim3(blocks_of(N)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(k_adj_link, dim3(blocks_of(P)), dim3(256), 0, st, A, (const uint8_t *)A.sub);
        if (n_active) hipLaunchKernelGGL(k_adj_rec_merge, dim3(n_active), dim3(64), 0, st, A, 3u);
        hipLaunchKernelGGL(k_adj_link, dim3(blocks_of(P)), dim3(256), 0, st, A, (const uint8_t *)nullptr);
        if (n_active) hipLaunchKernelGGL(k_adj_rec_best, dim3(n_active), dim3(64), 0, st, A);
        hipLaunchKernelGGL(k_adj_single, dim3(blocks_of(N)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(k_adj_gap, dim3(blocks_of(P)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(k_adj_link, dim3(blocks_of(P)), dim3(256), 0, st, A, (const uint8_t *)nullptr);
    }
    // ---- phases 4 to 7, the output
    if (n_active) hipLaunchKernelGGL(k_adj_rec_last, dim3(n_active), dim3(64), 0, st, A);
    hipLaunchKernelGGL(k_adj_lookup, dim3(blocks_of(N)), dim3(256), 0, st, A);
    uint32_t *out_cnt = A.path_len, *out_first = B[AJ_OUT_FIRST].as<uint32_t>();
    hipLaunchKernelGGL(k_adj_final, dim3(blocks_of(P + 1ull)), dim3(256), 0, st, A, out_cnt);
    launch_scan_u32(st, out_cnt, P + 1u, bsum, out_first, scan_total);
    hipLaunchKernelGGL(k_adj_emit, dim3(blocks_of(P)), dim3(256), 0, st, A, (const uint32_t *)out_first, B[AJ_OUT_NODES].as<mxg_adjust_node>(),
                       B[AJ_OUT_SRC].as<uint64_t>());
    MXG_HIP(h, hipGetLastError());
    std::vector<uint32_t> first32(P + 1ull);
    h->adj_nodes.resize(N);
    h->adj_source.resize(N);
    // every copy is queued whatever the one before returned, and the stream is drained before any of the errors is returned: no copy
    // into ctl or first32 is left pending when this function's frame goes
    e_copy = hipMemcpyAsync(ctl, A.ctl, sizeof ctl, hipMemcpyDeviceToHost, st);
    const hipError_t e_first = hipMemcpyAsync(first32.data(), out_first, (P + 1ull) * 4, hipMemcpyDeviceToHost, st);
    const hipError_t e_nodes = hipMemcpyAsync(h->adj_nodes.data(), B[AJ_OUT_NODES].p, N * sizeof(mxg_adjust_node), hipMemcpyDeviceToHost, st);
    const hipError_t e_src = hipMemcpyAsync(h->adj_source.data(), B[AJ_OUT_SRC].p, N * 8ull, hipMemcpyDeviceToHost, st);
    const hipError_t e_sync2 = hipStreamSynchronize(st);  // sync 2: the results
    for (const hipError_t e : {e_copy, e_first, e_nodes, e_src, e_sync2}) {
        if (e != hipSuccess) {
            h->adj_nodes.clear();
            h->adj_source.clear();
        }
        MXG_HIP(h, e);
    }
    if (ctl[1] || ctl[0] != ADJ_NO_ERR) {
        h->adj_nodes.clear();
        h->adj_source.clear();
        if (ctl[1] & ADJ_LIMIT_SWEEPS)
            return set_err(h, MXG_ELIMIT, "mxg_adjust_paths: the overlapping regions of a contig were not resolved in %u sweeps", ADJ_MAX_SWEEPS);
        if (ctl[1]) return set_err(h, MXG_ELIMIT, "mxg_adjust_paths: internal limit (%llu)", ctl[1]);
        const uint64_t j = ctl[0] & 0xFFFFFFFFull;
        const uint64_t q = (uint64_t)(std::upper_bound(path_first, path_first + n_paths + 1, j) - path_first) - 1;
        return set_err(h, MXG_EINVAL, "mxg_adjust_paths: path %llu node %llu: its segment or the segment of its chain's head was already taken "
                       "out of the contig's set by an earlier merge (two nodes with the same contig, start and end; phase %llu; the "
                       "reference raises KeyError)", (unsigned long long)q, (unsigned long long)(j - path_first[q]), ctl[0] >> 32);
    }
    const uint32_t n_out = first32[P];
    h->adj_nodes.resize(n_out);
    h->adj_source.resize(n_out);
    for (uint64_t q = 0; q <= n_paths; ++q) h->adj_first[q] = first32[q];
    return MXG_OK;
}

}  // namespace mxg
