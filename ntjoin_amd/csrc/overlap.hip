// overlap.hip -- the cut points of overlapping neighbours of a path (row f5): what the reference's overlap stage computes
// per junction with a segments file, a second indexlr run and one igraph graph per junction (adjust_for_trimming and
// tally_minimizers_overlap, bin/ntjoin_assemble.py:468-516; get_valid_regions, filter_minimizers_position and
// merge_overlapping, bin/ntjoin_overlap.py:13-134), here in two kernels over every node / junction of every path.
//
// A node is a segment [start, end) of a record, reverse-complemented when the node is '-'.  Its text as the reference
// sketches it has the middle [maskL, maskR) replaced by N; of the sketch only the minimizers in the kept ends count:
// positions < keepL = -raw_gap of the node before, and positions >= keepR = len + raw_gap of the node itself.
//
//   ov_node      one work-group per node.  A window is w consecutive VALID k-mers (invalid ones take no slot), so
//                the windows that hold a k-mer of the left end are those over the first nL + w - 1 valid k-mers (nL of them
//                in the end), and likewise from the right.  The group gathers those two lists of (hash, position) from the
//                packed bases chunk by chunk (the left one forwards, the right one backwards; complement = 3 - code on the
//                fly), which is the end plus w - 1 k-mers when nothing is invalid and reaches across N islands and the mask
//                when something is.  Where the two lists meet they are one list and every window counts.  Every window marks
//                its rightmost arg-min; marked k-mers in the kept ends are compacted in order, and a hash that occurs more
//                than once among them is dropped altogether (both ends count together, which is why the node is the work item).
//                Short lists find their duplicates pairwise; lists longer than MXG_OVL_PAIRWISE entries (64) insert their
//                hashes into an open-addressing table in the node's region (expected constant work per entry), which stays
//                for the junction pass.
//   ov_junction  one wave per node whose raw gap is negative: source list = the node's minimizers at positions >= keepR,
//                target list = the next node's at positions < its keepL.  Shared hashes are found pairwise or, where the
//                target node has a table, by probing it; they are ranked in both lists and cut into runs of list neighbours
//                (the components of the reference's weight-2 graph); every lane evaluates the runs that end in its entries,
//                and the largest (mapped, from_end, decimal string of the middle hash) gives the cut.
// The lists live in HBM regions sized per node on the host; a call works through its paths in batches that fit the scratch
// budget (MXG_OVL_BATCH entries), so the scratch does not grow with the number of paths.  Integers only.
#include <algorithm>

#include "bisect.h"
#include "mxg_internal.h"
#include "nthash_dev.h"
#include "text_dev.h"

namespace mxg {

enum { OV_NODES, OV_H0, OV_POS, OV_MARK, OV_OHASH, OV_OPOS, OV_CNT, OV_JS, OV_JP, OV_JT, OV_TAB, OV_OUT, OV_BUF_COUNT };
static_assert(OV_BUF_COUNT <= 16, "mxg_handle::ovbuf too small");

static constexpr uint32_t OV_MAX_K = 256;   // k-mers are hashed base by base
static constexpr uint32_t OV_MAX_W = 4096;  // every window scans its w k-mers
static constexpr uint32_t OV_NONE = 0xFFFFFFFFu;
static constexpr uint32_t OV_MAX_BATCH_NODES = 8u << 20;  // work-groups of one launch

// the node's hash table: 2 cap slots of (index into the node's list before duplicates went) + 1, 0 = empty
__device__ __forceinline__ uint32_t ov_slot(uint64_t hv, uint32_t n_slots) { return (uint32_t)((hv ^ (hv >> 29)) % n_slots); }

struct OvNode {
    uint64_t g0;    // global base index of the segment's first base on the forward strand
    uint64_t off;   // first entry of the node's region in the batch's scratch arrays
    uint32_t len;   // end - start
    uint32_t rev;   // 1: the node reads the reverse complement
    uint32_t keepL, keepR;  // kept ends: positions [0, keepL) and [keepR, len)
    uint32_t maskL, maskR;  // hard-masked middle [maskL, maskR) (equal: none)
    uint32_t inv0, invn;    // the assembly's invalid intervals that touch the segment
    uint32_t cap;   // entries of the region
    uint32_t junction;  // 1: the raw gap to the next node of the path is negative
};

struct OvTab {
    uint4 e[4];  // ntHash warm-up step per incoming base (HashTab entries 16..19, for the call's k)
};

__device__ __forceinline__ uint32_t ov_code(const uint32_t *__restrict__ packed, uint64_t g)
{
    return (packed[g >> 4] >> (((uint32_t)g & 15u) * 2u)) & 3u;
}

// the k-mer at position p of the node's text: false when it holds an invalid or masked base, else its canonical hash
__device__ __forceinline__ bool ov_kmer(const OvNode &nd, const uint32_t *__restrict__ packed, const ulonglong2 *__restrict__ inv,
                                        const OvTab &tab, uint32_t k, uint32_t variant, uint32_t p, uint64_t &h0)
{
    if (nd.maskL < nd.maskR && p + k > nd.maskL && p < nd.maskR) return false;
    const uint64_t a = nd.rev ? nd.g0 + nd.len - p - k : nd.g0 + p, b = a + k;
    if (nd.invn) {  // first interval that ends behind a
        const uint32_t lo = first_where(0u, nd.invn, [&](uint32_t i) { return inv[nd.inv0 + i].y > a; });
        if (lo < nd.invn && inv[nd.inv0 + lo].x < b) return false;
    }
    H2 h = {0u, 0u, 0u, 0u};
    for (uint32_t j = 0; j < k; ++j) {
        const uint32_t c = nd.rev ? 3u - ov_code(packed, b - 1 - j) : ov_code(packed, a + j);
        nt_step(h, tab.e[c]);
    }
    h0 = variant == MXG_VARIANT_V1_MIN ? canonical<MXG_VARIANT_V1_MIN>(h) : canonical<MXG_VARIANT_V2_SUM>(h);
    return true;
}

// ranks of two flags among the group's 256 threads (thread order) and their totals; every thread calls it
__device__ __forceinline__ void ov_scan2(bool f0, bool f1, uint32_t *lds, uint32_t &r0, uint32_t &r1, uint32_t &t0, uint32_t &t1)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t b0 = __ballot(f0), b1 = __ballot(f1), below = (1ull << lane) - 1ull;
    __syncthreads();
    if (lane == 0) {
        lds[wv] = (uint32_t)__popcll(b0);
        lds[4 + wv] = (uint32_t)__popcll(b1);
    }
    __syncthreads();
    r0 = (uint32_t)__popcll(b0 & below);
    r1 = (uint32_t)__popcll(b1 & below);
    t0 = t1 = 0;
    for (uint32_t u = 0; u < 4; ++u) {
        if (u < wv) {
            r0 += lds[u];
            r1 += lds[4 + u];
        }
        t0 += lds[u];
        t1 += lds[4 + u];
    }
}

__global__ __launch_bounds__(256) void ov_node(const OvNode *__restrict__ nodes, const uint32_t *__restrict__ packed,
                                               const ulonglong2 *__restrict__ inv, OvTab tab, uint32_t k, uint32_t w, uint32_t variant,
                                               uint64_t mult, uint32_t pairwise_max, uint64_t *l_h0, uint32_t *l_pos, uint8_t *l_mark,
                                               uint64_t *o_hash, uint32_t *o_pos, uint32_t *o_cnt, uint32_t *tabs)
{
    __shared__ uint32_t sc[8];
    const OvNode nd = nodes[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint32_t nk = nd.len >= k ? nd.len - k + 1 : 0;
    const uint32_t need = w - 1;  // k-mers beyond an end that its windows reach
    // ---- the left list: every valid k-mer in front of keepL and the `need` valid k-mers behind them, forwards
    uint32_t cL = 0, boundL = 0;  // the list holds every valid k-mer at a position < boundL
    if (nd.keepL && nk) {
        uint32_t extras = 0;
        uint32_t c0 = 0;
        for (; c0 < nk; c0 += 256) {
            if (c0 >= nd.keepL && extras >= need) break;
            const uint32_t p = c0 + tid;
            uint64_t h0 = 0;
            const bool ok = p < nk && ov_kmer(nd, packed, inv, tab, k, variant, p, h0);
            const bool extra = ok && p >= nd.keepL;
            uint32_t r_ok, r_ex, t_ok, t_ex;
            ov_scan2(ok, extra, sc, r_ok, r_ex, t_ok, t_ex);
            if (ok && (!extra || extras + r_ex < need)) {
                const uint64_t s = nd.off + cL + r_ok;
                l_h0[s] = h0;
                l_pos[s] = p;
                l_mark[s] = 0;
            }
            const uint32_t room = need - min(need, extras);
            cL += t_ok - (t_ex - min(t_ex, room));
            extras += t_ex;
        }
        __threadfence();
        __syncthreads();
        if (extras >= need) boundL = cL ? l_pos[nd.off + cL - 1] + 1 : min(nd.keepL, nk);
        else boundL = nk;
    }
    // ---- the right list: every valid k-mer from keepR on and the `need` valid k-mers in front of them, backwards down to
    //      boundL; it sits at the end of the region, in position order
    uint32_t cR = 0;
    bool met = false;  // the right list holds every valid k-mer from boundL on
    if (nd.keepR < nd.len && nk > boundL) {
        uint32_t extras = 0;
        uint32_t hi = nk;
        bool cut = false;
        while (hi > boundL) {
            if (hi <= nd.keepR && extras >= need) break;
            const uint32_t n = min(256u, hi - boundL);
            const uint32_t p = hi - 1 - min(tid, n - 1);
            uint64_t h0 = 0;
            const bool ok = tid < n && ov_kmer(nd, packed, inv, tab, k, variant, p, h0);
            const bool extra = ok && p < nd.keepR;
            uint32_t r_ok, r_ex, t_ok, t_ex;
            ov_scan2(ok, extra, sc, r_ok, r_ex, t_ok, t_ex);
            if (ok && (!extra || extras + r_ex < need)) {
                const uint64_t s = nd.off + nd.cap - 1 - (cR + r_ok);
                l_h0[s] = h0;
                l_pos[s] = p;
                l_mark[s] = 0;
            }
            const uint32_t room = need - min(need, extras);
            const uint32_t left_out = t_ex - min(t_ex, room);
            cut = cut || left_out;
            cR += t_ok - left_out;
            extras += t_ex;
            hi -= n;
        }
        met = hi == boundL && !cut;
    }
    __threadfence();
    __syncthreads();
    const uint32_t n_all = cL + cR;
    const uint64_t r_base = nd.off + nd.cap - cR;
#define OV_AT(v) ((v) < cL ? nd.off + (v) : r_base + ((v) - cL))
    // ---- every window marks its rightmost arg-min (<= while scanning left to right); a hash of 2^64 - 1 is never a minimizer
    const bool one_list = met && cL;  // the two lists are neighbours in the text: windows run over both
    for (uint32_t part = 0; part < (one_list ? 1u : 2u); ++part) {
        const uint32_t va = one_list ? 0u : (part ? cL : 0u), n = one_list ? n_all : (part ? cR : cL);
        if (n < w) continue;
        for (uint32_t j = tid; j + w <= n; j += 256) {
            uint64_t best = ~0ull;
            uint32_t arg = 0;
            for (uint32_t u = 0; u < w; ++u) {
                const uint64_t hv = l_h0[OV_AT(va + j + u)];
                if (hv <= best) {
                    best = hv;
                    arg = u;
                }
            }
            if (best != ~0ull) l_mark[OV_AT(va + j + arg)] = 1;
        }
    }
    __threadfence();
    __syncthreads();
    // ---- marked k-mers of the kept ends, in position order
    uint32_t n_out = 0;
    for (uint32_t c0 = 0; c0 < n_all; c0 += 256) {
        const uint32_t v = c0 + tid;
        bool keep = false;
        uint64_t s = 0;
        uint32_t p = 0;
        if (v < n_all) {
            s = OV_AT(v);
            p = l_pos[s];
            keep = l_mark[s] && (p < nd.keepL || p >= nd.keepR);
        }
        uint32_t r0, r1, t0, t1;
        ov_scan2(keep, false, sc, r0, r1, t0, t1);
        if (keep) {
            o_hash[nd.off + n_out + r0] = ext_hash(l_h0[s], mult);
            o_pos[nd.off + n_out + r0] = p;
        }
        n_out += t0;
    }
#undef OV_AT
    __threadfence();
    __syncthreads();
    // ---- a hash seen more than once among them is dropped altogether (tally_minimizers_overlap :510-516)
    const bool use_tab = n_out > pairwise_max;
    uint32_t *tab_n = tabs + 2 * nd.off;
    const uint32_t n_slots = 2 * nd.cap;
    if (use_tab) {
        for (uint32_t i = tid; i < n_slots; i += 256) tab_n[i] = 0;
        for (uint32_t i = tid; i < n_out; i += 256) l_mark[nd.off + i] = 0;
        __threadfence();
        __syncthreads();
        for (uint32_t i = tid; i < n_out; i += 256) {  // the first of equal hashes takes a slot; the others mark it and themselves
            const uint64_t hv = o_hash[nd.off + i];
            for (uint32_t q = ov_slot(hv, n_slots);; q = q + 1 == n_slots ? 0 : q + 1) {
                uint32_t was = atomicCAS(&tab_n[q], 0u, i + 1);
                if (was == 0) break;
                if (o_hash[nd.off + was - 1] == hv) {
                    l_mark[nd.off + was - 1] = 1;
                    l_mark[nd.off + i] = 1;
                    break;
                }
            }
        }
    } else {
        for (uint32_t i = tid; i < n_out; i += 256) {
            const uint64_t hv = o_hash[nd.off + i];
            uint32_t same = 0;
            for (uint32_t j = 0; j < n_out; ++j) same += o_hash[nd.off + j] == hv;
            l_mark[nd.off + i] = same > 1;
        }
    }
    __threadfence();
    __syncthreads();
    uint32_t n_fin = 0;
    for (uint32_t c0 = 0; c0 < n_out; c0 += 256) {
        const uint32_t i = c0 + tid;
        const bool keep = i < n_out && !l_mark[nd.off + i];
        const uint64_t hv = i < n_out ? o_hash[nd.off + i] : 0;
        const uint32_t p = i < n_out ? o_pos[nd.off + i] : 0;
        uint32_t r0, r1, t0, t1;
        ov_scan2(keep, false, sc, r0, r1, t0, t1);  // (its barriers separate the chunk's reads from its writes: n_fin + r0 <= i)
        if (keep) {
            o_hash[nd.off + n_fin + r0] = hv;
            o_pos[nd.off + n_fin + r0] = p;
        }
        if (i < n_out) l_pos[nd.off + i] = keep ? n_fin + r0 : OV_NONE;  // where the table's entry i went (the lists are done with l_pos)
        n_fin += t0;
    }
    if (tid == 0) o_cnt[2 * blockIdx.x + 1] = use_tab;
    if (tid == 0) o_cnt[2 * blockIdx.x] = n_fin;
}

// python's str(a) < str(b) for the decimal strings of two hashes (the reference names vertices by str(out_hash) and
// compares the names: "9" > "10")
__device__ __forceinline__ bool ov_str_less(uint64_t a, uint64_t b)
{
    if (a == b) return false;
    uint32_t da = dec_digits(a), db = dec_digits(b);
    if (da == db) return a < b;
    if (da < db) {
        uint64_t t = b;
        for (; db > da; --db) t /= 10;
        return a <= t;  // (equal: a is a proper prefix of b)
    }
    uint64_t t = a;
    for (; da > db; --da) t /= 10;
    return t < b;
}

// one wave per node with a junction behind it
__global__ __launch_bounds__(64) void ov_junction(const OvNode *__restrict__ nodes, const uint64_t *__restrict__ o_hash,
                                                  const uint32_t *__restrict__ o_pos, const uint32_t *__restrict__ o_cnt,
                                                  const uint32_t *__restrict__ tabs, const uint32_t *__restrict__ remap,
                                                  uint32_t *js, uint32_t *jp, uint32_t *jt, uint32_t *start_adjust,
                                                  uint32_t *end_adjust, uint8_t *cut_found)
{
    const OvNode S = nodes[blockIdx.x];
    if (!S.junction) return;
    const OvNode T = nodes[blockIdx.x + 1];
    const uint32_t lane = threadIdx.x;
    const uint32_t nS = o_cnt[2 * blockIdx.x], nTall = o_cnt[2 * blockIdx.x + 2];
    const bool t_tab = o_cnt[2 * blockIdx.x + 3];
    const uint64_t *sh = o_hash + S.off, *th = o_hash + T.off;
    const uint32_t *sp = o_pos + S.off, *tp = o_pos + T.off;
    // source list: positions >= keepR (a suffix); target list: positions < the next node's keepL (a prefix)
    const uint32_t s0 = first_ge(sp, 0u, nS, S.keepR), nT = first_ge(tp, 0u, nTall, T.keepL);
    uint32_t *ms = js + S.off, *mp = jp + S.off, *mt = jt + T.off;
    for (uint32_t t = lane; t < nT; t += 64) mt[t] = 0;
    __threadfence();
    __syncthreads();
    for (uint32_t s = s0 + lane; s < nS; s += 64) {  // hashes are unique within a node's list: at most one partner
        const uint64_t hv = sh[s];
        uint32_t at = OV_NONE;
        if (t_tab) {
            const uint32_t n_slots = 2 * T.cap;
            const uint32_t *tab_n = tabs + 2 * T.off;
            for (uint32_t q = ov_slot(hv, n_slots); tab_n[q]; q = q + 1 == n_slots ? 0 : q + 1) {
                const uint32_t t = remap[T.off + tab_n[q] - 1];  // (OV_NONE: a duplicate that went)
                if (t < nT && th[t] == hv) {
                    at = t;
                    break;
                }
            }
        } else {
            for (uint32_t t = 0; t < nT; ++t)
                if (th[t] == hv) at = t;
        }
        ms[s] = at;
        if (at != OV_NONE) mt[at] = 1;
    }
    __threadfence();
    __syncthreads();
    // rank of every shared target entry among the shared ones
    uint32_t run = 0;
    for (uint32_t c0 = 0; c0 < nT; c0 += 64) {
        const uint32_t t = c0 + lane;
        const bool f = t < nT && mt[t];
        const uint64_t b = __ballot(f);
        if (t < nT) mt[t] = run + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        run += (uint32_t)__popcll(b);
    }
    // the shared entries in source order: (source index, target index)
    uint32_t m = 0;
    for (uint32_t c0 = s0; c0 < nS; c0 += 64) {
        const uint32_t s = c0 + lane;
        const uint32_t at = s < nS ? ms[s] : OV_NONE;
        const uint64_t b = __ballot(at != OV_NONE);
        __syncthreads();
        if (at != OV_NONE) {
            const uint32_t o = s0 + m + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            ms[o] = at;
            mp[o] = s;
        }
        m += (uint32_t)__popcll(b);
    }
    __threadfence();
    __syncthreads();
    if (m == 0) return;
    // runs of entries that are neighbours in both lists = the components of the reference's graph after its weight filter
    // (merge_overlapping :28-32); the best of (mapped, from_end, str(mid)) wins (:78-79), compared as doubled integers.
    // from_end: get_dist_from_end (:145-149) is handed the node's index where it expects '+' / '-', so it returns -pos for
    // both lists whatever the orientation; that behaviour is what is reproduced.
    // Entry j begins a run when its target rank is no neighbour of entry j - 1's; the lane that holds a run's last entry
    // knows its first one from a running maximum over the beginnings, and evaluates the run.
    __shared__ uint64_t l_map[64], l_hash[64];
    __shared__ int64_t l_end[64];
    __shared__ uint32_t l_sp[64], l_tp[64];
    bool have = false;
    uint64_t b_map = 0, b_hash = 0;
    int64_t b_end = 0;
    uint32_t b_sp = 0, b_tp = 0;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < m; c0 += 64) {
        const uint32_t j = c0 + lane;
        uint32_t rj = 0;
        bool begins = false, ends = false;
        if (j < m) {
            rj = mt[ms[s0 + j]];
            if (j > 0) {
                const uint32_t rp = mt[ms[s0 + j - 1]];
                begins = !(rj == rp + 1 || rp == rj + 1);
            } else {
                begins = true;
            }
            ends = true;
            if (j + 1 < m) {
                const uint32_t rn = mt[ms[s0 + j + 1]];
                ends = !(rn == rj + 1 || rj == rn + 1);
            }
        }
        uint32_t a = begins ? j : 0;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)a, o, 64);
            if (lane >= o) a = max(a, t);
        }
        a = max(a, carry);
        carry = (uint32_t)__shfl((int)a, 63, 64);
        if (!ends) continue;
        // the run [a, j]
        const uint32_t len = j - a + 1, ia = s0 + a, ib = s0 + j;
        uint32_t im = ia;
        uint64_t mapped2 = 2;  // a single vertex: mapped = 1
        if (len > 1) {
            const uint64_t ha = sh[mp[ia]], hb = sh[mp[ib]];
            // the walk starts at the end whose name is the smaller string (:38-41); mid = walk[len / 2] (:52)
            im = ov_str_less(ha, hb) ? ia + len / 2 : ib - len / 2;
            const int64_t ds = (int64_t)sp[mp[ia]] - (int64_t)sp[mp[ib]], dt = (int64_t)tp[ms[ia]] - (int64_t)tp[ms[ib]];
            mapped2 = (uint64_t)(ds < 0 ? -ds : ds) + (uint64_t)(dt < 0 ? -dt : dt);
        }
        const uint32_t c_sp = sp[mp[im]], c_tp = tp[ms[im]];
        const uint64_t c_hash = sh[mp[im]];
        const int64_t c_end = -((int64_t)c_sp + (int64_t)c_tp);
        bool better = !have;
        if (have) {
            if (mapped2 != b_map) better = mapped2 > b_map;
            else if (c_end != b_end) better = c_end > b_end;
            else better = ov_str_less(b_hash, c_hash);
        }
        if (better) {
            have = true;
            b_map = mapped2;
            b_end = c_end;
            b_hash = c_hash;
            b_sp = c_sp;
            b_tp = c_tp;
        }
    }
    l_map[lane] = have ? b_map : 0;  // (a candidate's mapped is at least 2)
    l_end[lane] = b_end;
    l_hash[lane] = b_hash;
    l_sp[lane] = b_sp;
    l_tp[lane] = b_tp;
    __syncthreads();
    if (lane != 0) return;
    for (uint32_t u = 1; u < 64; ++u) {
        if (!l_map[u]) continue;
        bool better = !have;
        if (have) {
            if (l_map[u] != b_map) better = l_map[u] > b_map;
            else if (l_end[u] != b_end) better = l_end[u] > b_end;
            else better = ov_str_less(b_hash, l_hash[u]);
        }
        if (better) {
            have = true;
            b_map = l_map[u];
            b_end = l_end[u];
            b_hash = l_hash[u];
            b_sp = l_sp[u];
            b_tp = l_tp[u];
        }
    }
    end_adjust[blockIdx.x] = b_sp;
    start_adjust[blockIdx.x + 1] = b_tp;
    cut_found[blockIdx.x] = 1;
}

static bool ov_base_invalid(const Assembly *a, uint64_t g)
{
    auto it = std::upper_bound(a->inv.begin(), a->inv.end(), g,
                               [](uint64_t v, const std::pair<uint64_t, uint64_t> &iv) { return v < iv.second; });
    return it != a->inv.end() && it->first <= g;
}

int overlap_cuts(mxg_handle *h, Assembly *a, int assembly, uint32_t k, uint32_t w, const mxg_overlap_node *nodes,
                 const uint64_t *path_first, uint64_t n_paths, uint32_t *start_adjust, uint32_t *end_adjust, uint8_t *cut_found)
{
    if (!a->has_bases || !a->d_packed)
        return set_err(h, MXG_EINVAL, "mxg_overlap_cuts: assembly %d holds no bases (a minimizer table from a TSV, side-car or arrays, or a one-shot "
                       "handle that has released them): the overlap stage sketches the segments' ends from the bases", assembly);
    if (a->holds_pieces)
        return set_err(h, MXG_EINVAL, "mxg_overlap_cuts: assembly %d holds pieces of records (split load), not whole records", assembly);
    if (k == 0 || w == 0 || k > OV_MAX_K || w > OV_MAX_W)
        return set_err(h, MXG_ELIMIT, "mxg_overlap_cuts: k = %u, w = %u; the overlap kernels take 1 <= k <= %u and 1 <= w <= %u", k, w,
                       OV_MAX_K, OV_MAX_W);
    if (n_paths == 0) return MXG_OK;
    const uint64_t n_nodes = path_first[n_paths];
    if (n_nodes >= 0x7FFFFFFFull)
        return set_err(h, MXG_ELIMIT, "mxg_overlap_cuts: %llu nodes (at most 2^31 - 2)", (unsigned long long)n_nodes);
    // ---- the nodes as the kernels read them; everything the reference would assert is checked here, before any launch
    std::vector<OvNode> nd(n_nodes + 1);
    for (uint64_t p = 0; p < n_paths; ++p) {
        const uint64_t lo = path_first[p], hi = path_first[p + 1];
        if (hi < lo || hi > n_nodes) return set_err(h, MXG_EINVAL, "mxg_overlap_cuts: path_first is not increasing at path %llu", (unsigned long long)p);
        if (hi - lo < 2)
            return set_err(h, MXG_EINVAL, "mxg_overlap_cuts: path %llu has %llu node(s); a path has at least two (the reference leaves "
                           "shorter ones out)", (unsigned long long)p, (unsigned long long)(hi - lo));
        for (uint64_t i = lo; i < hi; ++i) {
            const mxg_overlap_node &in = nodes[i];
            const unsigned long long up = p, un = i - lo;
            if (in.record >= a->recs.size() || in.record < a->shard_lo || in.record >= a->shard_hi)
                return set_err(h, MXG_EINVAL, "mxg_overlap_cuts: path %llu node %llu: record %u is not one this handle holds bases of", up, un,
                               in.record);
            const Record &rec = a->recs[in.record];
            if (in.start >= in.end || in.end > rec.len)
                return set_err(h, MXG_EINVAL, "mxg_overlap_cuts: path %llu node %llu: [%u, %u) is not a segment of record '%s' (%llu bases)", up,
                               un, in.start, in.end, rec.id.c_str(), (unsigned long long)rec.len);
            if (ov_base_invalid(a, rec.base_off + in.start) || ov_base_invalid(a, rec.base_off + in.end - 1))
                return set_err(h, MXG_EINVAL, "mxg_overlap_cuts: path %llu node %llu: the segment [%u, %u) of '%s' begins or ends with an invalid "
                               "base (the reference strips N there and asserts the length)", up, un, in.start, in.end, rec.id.c_str());
            OvNode &o = nd[i];
            o.g0 = rec.base_off + in.start;
            o.len = in.end - in.start;
            o.rev = in.reverse ? 1u : 0u;
            const int64_t len = o.len, g_prev = i > lo ? (int64_t)nodes[i - 1].raw_gap : 0, g_own = in.raw_gap;
            o.keepL = (uint32_t)std::min<int64_t>(len, std::max<int64_t>(0, -g_prev));
            o.keepR = (uint32_t)std::min<int64_t>(len, std::max<int64_t>(0, len + g_own));
            int64_t ml = g_prev < 0 ? -g_prev + (int64_t)k + w : 0, mr = g_own < 0 ? len + g_own - (int64_t)k - w : len;
            if (ml > mr) mr = ml;  // (get_valid_regions :111-112: nothing is masked)
            o.maskL = (uint32_t)std::min<int64_t>(ml, len);
            o.maskR = (uint32_t)std::min<int64_t>(mr, len);
            o.junction = (i + 1 < hi && in.raw_gap < 0) ? 1u : 0u;
            const uint64_t g1 = o.g0 + o.len;
            auto first = std::upper_bound(a->inv.begin(), a->inv.end(), o.g0,
                                          [](uint64_t v, const std::pair<uint64_t, uint64_t> &iv) { return v < iv.second; });
            auto last = first;
            while (last != a->inv.end() && last->first < g1) ++last;
            o.inv0 = (uint32_t)(first - a->inv.begin());
            o.invn = (uint32_t)(last - first);
            const uint64_t nk = o.len >= k ? o.len - k + 1 : 0;
            const uint64_t capL = o.keepL ? std::min<uint64_t>(nk, (uint64_t)o.keepL + w - 1) : 0;
            const uint64_t capR = o.keepR < o.len ? std::min<uint64_t>(nk, (uint64_t)(o.len - o.keepR) + w - 1) : 0;
            o.cap = (uint32_t)std::min<uint64_t>(nk, capL + capR);
        }
    }
    if (a->inv.size() >= 0xFFFFFFFFull) return set_err(h, MXG_ELIMIT, "mxg_overlap_cuts: more than 2^32 - 2 stretches of invalid bases");
    MXG_HIP(h, hipSetDevice(h->device));
    DevBuf *B = h->ovbuf;
    if (!a->inv_on_device) {
        MXG_HIP(h, a->d_inv.ensure(a->inv.size() * 16 + 16));
        if (!a->inv.empty())
            MXG_HIP(h, hipMemcpyAsync(a->d_inv.p, a->inv.data(), a->inv.size() * 16, hipMemcpyHostToDevice, h->stream));
        a->inv_on_device = true;
    }
    static_assert(sizeof(std::pair<uint64_t, uint64_t>) == 16, "invalid-interval table layout");
    HashTab full;
    make_hash_tab(k, &full);
    OvTab tab;
    for (int c = 0; c < 4; ++c) tab.e[c] = full.e[16 + c];
    const uint64_t mult = 1ull ^ ((uint64_t)k * 0x90b45d39fb6da1faull);
    // ---- whole paths in batches whose regions fit the scratch budget (a path larger than the budget is a batch of its own)
    const uint64_t budget = std::max<uint64_t>(1, knob_u64(h, "MXG_OVL_BATCH", 32ull << 20));
    const uint32_t pairwise_max = (uint32_t)std::min<uint64_t>(knob_u64(h, "MXG_OVL_PAIRWISE", 64), 0xFFFFFFFFull);
    MXG_HIP(h, B[OV_OUT].ensure(n_nodes * 9 + 16));
    uint32_t *d_sa = B[OV_OUT].as<uint32_t>(), *d_ea = d_sa + n_nodes;
    uint8_t *d_cf = reinterpret_cast<uint8_t *>(d_ea + n_nodes);
    MXG_HIP(h, hipMemsetAsync(B[OV_OUT].p, 0, n_nodes * 9, h->stream));
    for (uint64_t p0 = 0; p0 < n_paths;) {
        uint64_t p1 = p0, entries = 0;
        while (p1 < n_paths) {
            uint64_t e = 0;
            for (uint64_t i = path_first[p1]; i < path_first[p1 + 1]; ++i) e += nd[i].cap;
            if (p1 > p0 && (entries + e > budget || path_first[p1 + 1] - path_first[p0] > OV_MAX_BATCH_NODES)) break;
            for (uint64_t i = path_first[p1]; i < path_first[p1 + 1]; ++i) {
                nd[i].off = entries;
                entries += nd[i].cap;
            }
            ++p1;
        }
        const uint64_t n0 = path_first[p0], nb = path_first[p1] - n0;
        const size_t ne = (size_t)entries + 16;
        MXG_HIP(h, B[OV_NODES].ensure((nb + 1) * sizeof(OvNode)));
        MXG_HIP(h, B[OV_H0].ensure(ne * 8));
        MXG_HIP(h, B[OV_POS].ensure(ne * 4));
        MXG_HIP(h, B[OV_MARK].ensure(ne));
        MXG_HIP(h, B[OV_OHASH].ensure(ne * 8));
        MXG_HIP(h, B[OV_OPOS].ensure(ne * 4));
        MXG_HIP(h, B[OV_CNT].ensure((nb + 1) * 8));
        MXG_HIP(h, B[OV_TAB].ensure(2 * ne * 4));
        MXG_HIP(h, B[OV_JS].ensure(ne * 4));
        MXG_HIP(h, B[OV_JP].ensure(ne * 4));
        MXG_HIP(h, B[OV_JT].ensure(ne * 4));
        // (the copy is synchronous for pageable memory: nd may be rewritten for the next batch right away)
        MXG_HIP(h, hipMemcpyAsync(B[OV_NODES].p, nd.data() + n0, (nb + 1) * sizeof(OvNode), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(ov_node, dim3((uint32_t)nb), dim3(256), 0, h->stream, B[OV_NODES].as<OvNode>(), a->d_packed,
                           a->d_inv.as<ulonglong2>(), tab, k, w, (uint32_t)h->cfg.variant, mult, pairwise_max, B[OV_H0].as<uint64_t>(),
                           B[OV_POS].as<uint32_t>(), B[OV_MARK].as<uint8_t>(), B[OV_OHASH].as<uint64_t>(), B[OV_OPOS].as<uint32_t>(),
                           B[OV_CNT].as<uint32_t>(), B[OV_TAB].as<uint32_t>());
        hipLaunchKernelGGL(ov_junction, dim3((uint32_t)nb), dim3(64), 0, h->stream, B[OV_NODES].as<OvNode>(), B[OV_OHASH].as<uint64_t>(),
                           B[OV_OPOS].as<uint32_t>(), B[OV_CNT].as<uint32_t>(), B[OV_TAB].as<uint32_t>(), B[OV_POS].as<uint32_t>(),
                           B[OV_JS].as<uint32_t>(), B[OV_JP].as<uint32_t>(),
                           B[OV_JT].as<uint32_t>(), d_sa + n0, d_ea + n0, d_cf + n0);
        MXG_HIP(h, hipGetLastError());
        MXG_HIP(h, hipStreamSynchronize(h->stream));  // the next batch reuses the regions (and the scratch may be re-allocated)
        p0 = p1;
    }
    MXG_HIP(h, hipMemcpyAsync(start_adjust, d_sa, n_nodes * 4, hipMemcpyDeviceToHost, h->stream));
    MXG_HIP(h, hipMemcpyAsync(end_adjust, d_ea, n_nodes * 4, hipMemcpyDeviceToHost, h->stream));
    MXG_HIP(h, hipMemcpyAsync(cut_found, d_cf, n_nodes, hipMemcpyDeviceToHost, h->stream));
    MXG_HIP(h, hipStreamSynchronize(h->stream));
    return MXG_OK;
}

}  // namespace mxg
