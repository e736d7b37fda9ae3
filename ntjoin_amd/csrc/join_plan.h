// The arithmetic of the graph stage's join, the one place that knows it: from the assemblies' sizes to which join runs and how its
// partitions are sized (join_shape), what a handle has learnt from overflows (JoinLearnt), and what the cursors of an overflowed
// two-level join ask for (join_overflow_verdict), and the bits of the two-level join's 12-byte records (pj12_*).  No device, no
// handle: graph.hip's plan_join reads the knobs, calls join_shape and lays the arrays out; tests/test_join_plan_cpu.py and
// tests/test_join_records_cpu.py compile this header on their own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "ntjoin_mx.h"

#if defined(__HIPCC__)
#define PJP_HD __host__ __device__ inline
#else
#define PJP_HD inline
#endif

namespace mxg {

enum { GRAPH_FULL = 0, GRAPH_DG_VERTICES = 1, GRAPH_DG_EDGES = 2, GRAPH_DG_EDGES_APPLIED = 3 /* nxt/prv already filled */ };

constexpr uint32_t PJ_IPB = 4096;  // items per bucketing block = 16 blocks of 256
constexpr uint32_t PJ_T = 2048;    // slots of a partition's table (+1: the slot of the key that equals the empty mark)
constexpr uint32_t PJ_MAX_P = 4096;
constexpr uint32_t PJ1_CS = 32;  // words between the coarse partitions' cursors (own 128-byte lines: same-line atomics serialise)
constexpr uint32_t PJ_CAP_LIMIT = 0xFFFFF000u;  // a coarse partition's records are counted in 32 bits, in whole bucketing blocks

// What a handle has learnt from the overflows of its LDS joins.  It holds for the sketches it was learnt on (`sig`).
struct JoinLearnt {
    bool overflowed = false;  // the partitioned join overflowed once (build_graph then starts with the global table)
    uint32_t cap1_P1 = 0;     // two-level join: coarse partitions and the records one of them must hold, as an earlier call's
    uint64_t cap1_need = 0;   // cursors reported them (a key of large multiplicity skews the partitions)
    uint64_t sig = 0;         // the sketches (count and sizes) the fields above were learnt on
    uint32_t sub_P1 = 0;      // fused call: what the sub-ranges of a coarse partition must hold per assembly (cap1_need's counterpart)
    uint64_t sub_need[MXG_MAX_ASSEMBLIES] = {};
    bool dg_off = false;      // owner of a partitioned graph stage: the LDS join failed once over the slots (global table from then on)
    // the verdict prefill of assembly 0 (join_verdict.h): how many of its minimizers the last build found shared, of how many, and
    // for which sizes (prefill_signature: the fused call's bounds have one too)
    bool pre_known = false;
    uint64_t pre_sig = 0, pre_shared0 = 0, pre_n0 = 0;

    static uint64_t signature(uint32_t n_asm, const uint64_t *n_mx)
    {
        uint64_t s = 0x9E3779B97F4A7C15ull * ((uint64_t)n_asm + 1);
        for (uint32_t a = 0; a < n_asm; ++a) s = (s ^ n_mx[a]) * 0x100000001B3ull;
        return s;
    }
    // build_graph over finished sketches (not the fused call, whose sizes are still bounds): other sketches -- new assemblies, a
    // borrowed buffer refilled and sketched again -- start with the defaults.  sub_need[] stays as it is (nothing reads it while
    // sub_P1 is 0, and the verdict clears it when it sets sub_P1 anew); so does dg_off.
    void sketches_are(uint64_t s)
    {
        if ((overflowed || cap1_P1) && sig != s) {
            overflowed = false;
            cap1_P1 = 0;
            cap1_need = 0;
            sub_P1 = 0;
        }
        sig = s;
    }
    // an assembly was added to the handle.  Leaves sub_P1 / sub_need[], sig and dg_off alone.
    void assembly_added()
    {
        pre_known = false;
        overflowed = false;
        cap1_P1 = 0;
        cap1_need = 0;
    }
    void gave_up() { overflowed = true; }  // the LDS join fell to the global table
    // mxg_set_sketch_device put other minimizers in an assembly's place.  What overflowed was the data that left, and the sizes
    // alone (sketches_are) cannot tell: the next build tries the LDS join again.  The verdict prefill's count stays (pre_known):
    // a guess that no longer fits costs bytes, never the result (prefill_own0 below), and sub_P1 / sub_need[] only ever widen.
    // (mxg_set_sketch_gathered does not call this: the exchange installs the same union again every step, and the lesson holds.)
    void sketch_replaced()
    {
        overflowed = false;
        cap1_P1 = 0;
        cap1_need = 0;
    }

    // The sizes a plan was made for, as one word: the sketches' own sizes or the fused call's bounds (which settle from the second
    // call on: they follow the counts of the call before).
    static uint64_t prefill_signature(uint32_t n_asm, const uint64_t *n_of, bool bounds)
    {
        return signature(n_asm, n_of) ^ (bounds ? 0xB0B0B0B0B0B0B0B0ull : 0ull);
    }
    // a build ended: `shared0` of the n0 minimizers the plan counted for assembly 0 are shared (= the graph's vertices)
    void shared_counted(uint64_t plan_sig, uint64_t shared0, uint64_t n0)
    {
        pre_known = true;
        pre_sig = plan_sig;
        pre_shared0 = shared0;
        pre_n0 = n0;
    }
    // Assembly 0's verdicts are prefilled "shared, own index" (PJ_PREFILL_OWN0) only where the previous build, of the same sizes,
    // found more than half of assembly 0 shared: the join then sends assembly 0's other words instead of its shared ones, which
    // are fewer.  The first build, a build after other sizes or after an added assembly: PJ_PREFILL_UNIQUE.
    // "The same sizes" is all the guess knows, and a sketch can be replaced on a live handle without changing them:
    // mxg_set_sketch_device and mxg_set_sketch_gathered with as many minimizers as before, a borrowed packed buffer that is
    // refilled and sketched again (the fused call's key is its bounds, which follow the record layout alone).  The guess may then
    // be wrong, by design: the join sends every word that differs from the prefill, word 1 included, so a wrong guess moves more
    // bytes and gives the same flags, vertices and edges (tests/test_gpu_join_prefill_stale.py).
    bool prefill_own0(uint64_t plan_sig) const { return pre_known && pre_sig == plan_sig && 2 * pre_shared0 > pre_n0; }
};

// ---- the two-level join's 12-byte records -------------------------------------------------------------------------------------
// A record is {key lo, key hi, item, assembly | PJ_REC_DUP}: 16 bytes, written by k_pj1_scatter, read and rewritten by
// k_pj2_bucket, read by the join.  The fourth word holds 6 bits (5 of the assembly, MXG_MAX_ASSEMBLIES = 32, and the mark
// "more than once in its assembly"), and the place of a record says as much already:
//   level 1 (sub-ranges per assembly): the record lies in ITS assembly's sub-range.  {product lo, product hi, item | mark << 31}
//       (items are below 2^29, join_shape), product = key * 0x9E3779B97F4A7C15.
//   level 2: the record lies in fine partition b of coarse partition c, so bits 44 .. 44 + lg P - 1 (b) and 52 .. 52 + lg P1 - 1
//       (c) of its product are known.  The 6-bit tag (assembly | mark << 5) takes the lowest 6 of those bits: the fine
//       partition's first, then the coarse one's.  {product lo, product hi with the tag, item}.
// The multiplier is odd, so the product is a bijection of the key: two records of one fine partition have equal keys exactly when
// their products agree in every bit that is not implied, i.e. when pj12_key() of both is equal.  The table slot of the join
// (bits 32..42 of the product) lies below the tag.  pj12_key() is never the table's empty mark (all ones): the tag's bits are 0.
constexpr uint64_t PJ_MUL = 0x9E3779B97F4A7C15ull;
constexpr uint32_t PJ12_TAG_BITS = 6, PJ12_TAG_DUP = 32u, PJ12_ITEM_DUP = 0x80000000u;
constexpr uint32_t PJ12_FINE_SHIFT = 44 - 32, PJ12_COARSE_SHIFT = 52 - 32;  // in the product's high word

PJP_HD uint32_t pj12_lg(uint32_t x)  // x = 2^n
{
    uint32_t n = 0;
    while ((1u << n) < x && n < 31) ++n;
    return n;
}
// do the partitions imply 6 bits?  (P1 = 0: one level)
PJP_HD bool pj12_fits(uint32_t P1, uint32_t P) { return P1 != 0 && P != 0 && (uint64_t)P1 * P >= (1u << PJ12_TAG_BITS); }
// tag bits taken from the fine partition's field (the rest come from the coarse one's)
PJP_HD uint32_t pj12_fine_bits(uint32_t lgP) { return lgP < PJ12_TAG_BITS ? lgP : PJ12_TAG_BITS; }
// the bits of the product's high word that hold the tag
PJP_HD uint32_t pj12_tag_mask(uint32_t lgP)
{
    const uint32_t f = pj12_fine_bits(lgP);
    return (((1u << f) - 1u) << PJ12_FINE_SHIFT) | (((1u << (PJ12_TAG_BITS - f)) - 1u) << PJ12_COARSE_SHIFT);
}
PJP_HD uint32_t pj12_tag(uint32_t assembly, bool dup) { return assembly | (dup ? PJ12_TAG_DUP : 0u); }
PJP_HD uint32_t pj12_pack(uint32_t prod_hi, uint32_t lgP, uint32_t tag)
{
    const uint32_t f = pj12_fine_bits(lgP);
    return (prod_hi & ~pj12_tag_mask(lgP)) | ((tag & ((1u << f) - 1u)) << PJ12_FINE_SHIFT) | ((tag >> f) << PJ12_COARSE_SHIFT);
}
PJP_HD uint32_t pj12_unpack_tag(uint32_t word, uint32_t lgP)
{
    const uint32_t f = pj12_fine_bits(lgP);
    return ((word >> PJ12_FINE_SHIFT) & ((1u << f) - 1u)) | (((word >> PJ12_COARSE_SHIFT) & ((1u << (PJ12_TAG_BITS - f)) - 1u)) << f);
}
// what two records of one fine partition compare (and the join's table keeps)
PJP_HD uint64_t pj12_key(uint32_t lo, uint32_t word, uint32_t lgP) { return ((uint64_t)(word & ~pj12_tag_mask(lgP)) << 32) | lo; }
PJP_HD bool pj12_same_key(uint32_t lo_a, uint32_t word_a, uint32_t lo_b, uint32_t word_b, uint32_t lgP)
{
    return pj12_key(lo_a, word_a, lgP) == pj12_key(lo_b, word_b, lgP);
}
// the partitions of a product (what pj1_part / pj_part of graph.hip take of key * PJ_MUL)
PJP_HD uint32_t pj12_coarse(uint64_t prod, uint32_t P1) { return (uint32_t)(prod >> 52) & (P1 - 1u); }
PJP_HD uint32_t pj12_fine(uint64_t prod, uint32_t P) { return (uint32_t)(prod >> 44) & (P - 1u); }

struct JoinRequest {
    uint32_t A = 0;                          // assemblies, 1..MXG_MAX_ASSEMBLIES
    uint64_t n_of[MXG_MAX_ASSEMBLIES] = {};  // minimizers per assembly (the sketches' own sizes, or the bounds of the fused call)
    int mode = GRAPH_FULL;
    bool bounds = false;           // the sizes are bounds, the counts are still on the device
    bool global_table = false;     // the caller asks for the global table (an earlier attempt overflowed)
    bool split = false;            // a sub-range of every coarse partition per assembly (the fused call's early partition)
    bool force_two_level = false;  // MXG_PJ_TWO_LEVEL
    bool join_global = false;      // MXG_GRAPH_JOIN=global
    bool no_rec12 = false;         // MXG_PJ_REC12=0: 16-byte records everywhere
    bool no_pipe = false;          // MXG_PJ_PIPE=0: k_pj_join behind two levels too (it reads 16-byte records only)
    bool no_prefill0 = false;      // MXG_PJ_PREFILL0=0: assembly 0 keeps PJ_PREFILL_UNIQUE whatever was learnt
    bool no_graph_rank = false;    // MXG_GRAPH_RANK=0: the adjacency table and its edge passes where the rank route would run
    uint32_t graph_u = 0;          // MXG_GRAPH_U: 1, 2 or 4 forces the width of the tail's ordered passes (anything else: by size)
    uint32_t pj_tiles = 0;         // MXG_PJ_TILES: 1 or 2 forces level 1's tiles per thread block on the 12-byte route (anything else: by size)
};

enum JoinShapeError { JS_OK = 0, JS_TOO_MANY_MINIMIZERS, JS_TOO_MANY_ITEMS };

// Everything the stage derives from the sizes before it launches anything: which join, how many partitions of what capacity.
struct JoinShape {
    uint32_t A = 0;
    uint64_t N = 0, nvs = 0;  // minimizers of all assemblies; stride of the vertex arrays (the smallest assembly)
    uint64_t n_of[MXG_MAX_ASSEMBLIES] = {};
    uint32_t cap = 0, mask = 0, full = 0;  // global table: slots, slots - 1; one bit per assembly
    uint32_t P = 0, P1 = 0, cap1 = 0, rows2 = 0;
    bool two_level = false, pj = false, dg_pj = false;
    bool split = false;  // a sub-range of every coarse partition per assembly (PjSub)
    uint32_t n_sub = 1;  // sub-ranges (cursors) per coarse partition, and what each holds
    uint32_t sub_cap[MXG_MAX_ASSEMBLIES] = {}, sub_off[MXG_MAX_ASSEMBLIES] = {}, skew_lim[MXG_MAX_ASSEMBLIES] = {};
    uint32_t bstart[MXG_MAX_ASSEMBLIES + 1] = {};  // exclusive prefix of the assemblies' 256-element blocks
    uint32_t nb = 0;                               // ... and their number
    size_t nb0 = 0;                                // assembly 0's
    uint32_t n_items = 0, e_blocks = 0;            // A * nvs items of the edge kernels, in blocks of 256
    bool rec12 = false;        // 12-byte records (two levels, sub-ranges per assembly, the pipelined join kernel)
    uint32_t prefill0 = 0;     // assembly 0's verdict prefill (PjPrefillRule of join_verdict.h: 0 unless learnt otherwise)
    uint64_t pre_sig = 0;      // JoinLearnt::prefill_signature of these sizes
    size_t n_cur = 0;  // split: words of the sub-ranges' cursors that lie between the super-counts and the counts
    // 256-blocks per thread block of the ordered passes (graph_tail_u): k_flags_pj and k_vertices_pj over nb, the adjacency and
    // edge passes over e_blocks
    uint32_t u_flags = 1, u_vertices = 1, u_edges = 1;
    // the edge passes work from rank arrays, no adjacency table (graph_rank.h): the whole stage behind an LDS join.  The global
    // table's route and both distributed modes (adjacency arrives as messages) keep k_adjacency / the table.
    bool graph_rank = false;
    uint32_t pj_tiles_forced = 0;  // level 1's tiles per thread block as forced (0: pj1_tiles decides per launch)
};

// The tail's ordered passes (k_flags_pj, k_vertices_pj over nb 256-blocks; k_adjacency, k_edge_flags, k_edges or, on the rank route,
// k_edge_flags_rank, k_edges_rank over e_blocks) give
// every thread block U consecutive 256-blocks whose loads are all requested before the first is used: a pass of one 256-block per
// thread block keeps 8 KB of loads in flight per CU, where an HBM round trip wants tens of KB ("The tail's
// ordered passes").  Wider blocks are fewer blocks: the pass must still fill the chip's 256 CUs x 8 resident thread blocks several
// times over, or its last round of blocks runs on a half-empty chip.  The thresholds lie between the sizes measured at forced
// U = 1 / 2 / 4 (profiles/r08/graph_tail_ab.txt; traced time of the five passes together, us):
//   100 + 100 Mbp    (nb ~ 1 560, e_blocks ~ 1 170)    27.8 / 29.4 / 31.3   the wider, the slower
//   300 + 300 Mbp    (nb ~ 4 670, e_blocks ~ 3 520)    45.5 / 44.2 / 42.9   U = 2 not slower than 1; 4 against 2 inside the spread
//   1000 + 1000 Mbp  (nb ~ 15 560, e_blocks ~ 11 720)  105.5 / 97.3 / 92.6  U = 4 fastest
//   3000 + 3000 Mbp  (nb = 46 700, e_blocks ~ 35 200)  298.9 / 255.5 / 237.2
// The vertex pass stops at U = 2 by size: <4> takes 90 VGPRs (5 waves per SIMD where <2> keeps 8) and traced 91.9 us against
// <2>'s 91.8 at 3 Gbp + 3 Gbp, 31.0 against 30.9 at 1 Gbp + 1 Gbp.
constexpr uint32_t GRAPH_TAIL_U2 = 3072, GRAPH_TAIL_U4 = 8192;
constexpr uint32_t GRAPH_TAIL_U_VERTICES = 2;  // the widest vertex pass the size rule picks
inline uint32_t graph_tail_u(uint64_t blocks, uint32_t forced = 0)
{
    if (forced == 1 || forced == 2 || forced == 4) return forced;
    return blocks >= GRAPH_TAIL_U4 ? 4u : blocks >= GRAPH_TAIL_U2 ? 2u : 1u;
}
// thread blocks of a pass over `blocks` 256-blocks, U to each
inline uint32_t graph_tail_grid(uint64_t blocks, uint32_t U) { return (uint32_t)((blocks + U - 1) / U); }

// Level 1 of the two-level join (k_pj1_scatter) can give a thread block G consecutive 4096-minimizer tiles of its launch: one
// histogram and one add per coarse bin for all of them, G times fewer adds to every cursor.  A 1024-thread block has two places
// per CU, 512 on the chip, and a launch of the two-level route has about a thousand tiles (1 465 per assembly at 3 Gbp + 3 Gbp):
// wider blocks are fewer rounds of blocks, and their last round runs on a part of the chip.  Traced minimum of the kernel, the
// target's launch alone on the GPU, at forced G = 1 / 2 / 4, two runs each (profiles/r13/join_tiles_ab.txt; us; in brackets the
// kernel before it asked for a tile's four hashes ahead of their first use, which is where the time went):
//   1.4 + 1.4 Gbp    (684 tiles per launch)      21.4 21.2 / 23.1 24.0 / 25.3 24.2   [28.7]   the wider, the slower
//   2 + 2 Gbp        (977 tiles)                 34.0 32.8 / 31.2 32.0 / 37.4 37.9   [39.7]
//   3 + 3 Gbp        (1 465 tiles)               42.1 41.9 / 40.7 40.5 / 47.8 48.1   [53.4 52.5]
// (below 1.3 + 1.3 Gbp the join has one level).  G = 4 takes 92 VGPRs, one block per CU, and is slower at every size: it is not
// built.  G = 2 (52 VGPRs, two blocks per CU as G = 1) is 1 to 2 us ahead from about 900 tiles on and buys nothing in the step:
// at 3 Gbp + 3 Gbp the step's median is 2.2219 ms with it and 2.2208 without, and with four assemblies (2 930 tiles a launch, the
// reference's launches beside the others' filters) every run with it is slower, 6.68-6.71 against 6.63-6.67 ms.  So NO size takes
// it: the rule below answers 1 unless MXG_PJ_TILES=2 forces the 12-byte route's launches to two, which is how the figures above
// can be had again.  The 16-byte route (one launch for all assemblies, the block looks every tile's assembly up) was slower with
// wider blocks (189 / 247 / 275 us on 4.5 + 4.5 Gbp) and has one width; so has level 2 (39.3 / 46.9 / 56.0 us at 3 Gbp + 3 Gbp).
// The rule is PER LAUNCH (on the fused route every assembly has its own), so that a threshold, should a later chip want one,
// leaves a small assembly beside a large one at G = 1.
constexpr uint32_t PJ1_TILES_G2 = 0xFFFFFFFFu;  // tiles per launch from which G = 2 is taken: never

inline uint32_t pj1_tiles(uint64_t tiles, bool rec12, uint32_t forced = 0)
{
    if (!rec12) return 1u;
    if (forced == 1 || forced == 2) return forced;
    return tiles >= PJ1_TILES_G2 ? 2u : 1u;
}
// thread blocks of a launch over `tiles` tiles, G to each
inline uint32_t pj_tiles_grid(uint64_t tiles, uint32_t G) { return (uint32_t)((tiles + G - 1) / G); }

inline JoinShapeError join_shape(const JoinRequest &rq, const JoinLearnt &learnt, JoinShape &pl)
{
    pl = JoinShape();
    const uint32_t A = pl.A = rq.A;
    uint64_t N = 0, nmin = ~0ull, n_max = 0;
    for (uint32_t a = 0; a < A; ++a) {
        pl.n_of[a] = rq.n_of[a];
        N += rq.n_of[a];
        nmin = std::min(nmin, rq.n_of[a]);
        n_max = std::max(n_max, rq.n_of[a]);
    }
    pl.N = N;
    if (N >= (1ull << 30)) return JS_TOO_MANY_MINIMIZERS;
    pl.cap = 1024;
    while (pl.cap < 2 * N) pl.cap <<= 1;
    pl.mask = pl.cap - 1;
    pl.full = (A == 32) ? 0xFFFFFFFFu : ((1u << A) - 1u);
    // the join: LDS tables per hash partition (the whole-stage call, up to PJ_MAX_P partitions of <= 1280 records), else
    // the global table
    uint32_t P = 256;
    while ((uint64_t)P * 1280 < N) P <<= 1;
    // beyond PJ_MAX_P partitions of <= 1280 records: two levels -- P1 coarse partitions, each sorted into 256 sub-partitions
    uint32_t P1 = 0, cap1 = 0;
    bool fits32 = true;
    if (P > PJ_MAX_P || rq.force_two_level) {
        P = 256;
        P1 = 2;
        while ((uint64_t)P1 * P * 1000 < N) P1 <<= 1;
        if (rq.split) {  // a sub-range per assembly, each with the slack of the whole: 25 % above ITS mean
            uint64_t c_all = 0;
            for (uint32_t a = 0; a < A; ++a) {
                const uint64_t mean = rq.n_of[a] / P1;
                uint64_t c1 = mean + mean / 4 + 4096;
                if (learnt.sub_P1 == P1) c1 = std::max<uint64_t>(c1, learnt.sub_need[a]);  // (what an earlier call's cursors asked for)
                c1 = (c1 + PJ_IPB - 1) / PJ_IPB * PJ_IPB;
                pl.sub_off[a] = (uint32_t)std::min<uint64_t>(c_all, PJ_CAP_LIMIT);
                pl.sub_cap[a] = (uint32_t)std::min<uint64_t>(c1, PJ_CAP_LIMIT);
                pl.skew_lim[a] = (uint32_t)std::min<uint64_t>(mean + mean / 32 + 2048, 0xFFFFFFFFull);  // 3 % above the mean
                c_all += c1;
            }
            pl.n_sub = A;
            pl.split = true;
            cap1 = (uint32_t)std::min<uint64_t>(c_all, PJ_CAP_LIMIT);
            fits32 = c_all <= PJ_CAP_LIMIT;
        } else {
            uint64_t c1 = (N / P1) + (N / P1) / 4 + 4096;  // 25 % above the mean (hash skew: keys of large multiplicity)
            if (learnt.cap1_P1 == P1) c1 = std::max<uint64_t>(c1, learnt.cap1_need);  // (what an earlier call's cursors asked for)
            cap1 = (uint32_t)((c1 + PJ_IPB - 1) / PJ_IPB * PJ_IPB);
            pl.sub_cap[0] = cap1;
        }
        pl.rows2 = cap1 / PJ_IPB;
    }
    pl.P = P;
    pl.P1 = P1;
    pl.cap1 = cap1;
    pl.two_level = P1 != 0 && P1 <= 4096 && fits32 && (uint64_t)P1 * cap1 < (1ull << 32) && (uint64_t)P1 * P * (PJ_T + 1) < (1ull << 29);
    // (the owner's half of the partitioned graph stage takes the LDS join too when it runs over fixed slots -- bounds: the counts on
    // the device, nobody waits for the host before the verdicts leave -- and says "failed" through a DEVICE word)
    pl.dg_pj = rq.mode == GRAPH_DG_VERTICES && rq.bounds && !learnt.dg_off;
    // (k_pj_join's verdict word carries the index of the key's minimizer in assembly 0 above three flag bits, k_pj2_bucket's
    // reference that of a minimizer of the same assembly: n_max < 2^29)
    pl.pj = (rq.mode == GRAPH_FULL || pl.dg_pj) && !rq.global_table && (P1 == 0 || pl.two_level) && P <= PJ_MAX_P && n_max < (1ull << 29) &&
            !rq.join_global;
    for (uint32_t a = 0; a < A; ++a) {
        pl.bstart[a] = pl.nb;
        pl.nb += (uint32_t)((rq.n_of[a] + 255) / 256);
    }
    for (uint32_t a = A; a <= MXG_MAX_ASSEMBLIES; ++a) pl.bstart[a] = pl.nb;
    pl.nb0 = (size_t)((rq.n_of[0] + 255) / 256);
    // vertex arrays are strided by an upper bound of the vertex count (every vertex occurs once in every assembly), so
    // the stage needs no host sync before its kernels: they read the counts from the control block in HBM
    pl.nvs = nmin;
    if (pl.nvs > 0 && (uint64_t)A * pl.nvs >= (1ull << 32)) return JS_TOO_MANY_ITEMS;  // (cannot happen below 2^30 minimizers)
    pl.n_items = (uint32_t)((size_t)A * pl.nvs);
    pl.e_blocks = (pl.n_items + 255) / 256;
    if (pl.split && pl.pj && pl.two_level) pl.n_cur = (size_t)P1 * A * PJ1_CS;
    // 12-byte records: where the record's place implies its fourth word.  Level 1 needs the sub-ranges per assembly, level 2 six
    // implied bits; k_pj_join_pipe reads them (partitions of at most 256 rows), k_pj_join and every other route keep 16 bytes.
    pl.rec12 = pl.split && pl.pj && pl.two_level && pj12_fits(P1, P) && pl.rows2 <= 256 && !rq.no_rec12 && !rq.no_pipe;
    pl.pre_sig = JoinLearnt::prefill_signature(A, rq.n_of, rq.bounds);
    pl.prefill0 = pl.pj && pl.two_level && !rq.no_prefill0 && learnt.prefill_own0(pl.pre_sig) ? 1u : 0u;
    pl.u_flags = graph_tail_u(pl.nb, rq.graph_u);
    // (by size the vertex pass stops at GRAPH_TAIL_U_VERTICES; MXG_GRAPH_U=4 still runs it at 4)
    pl.u_vertices = graph_tail_u(0, rq.graph_u) == rq.graph_u ? rq.graph_u : std::min(pl.u_flags, GRAPH_TAIL_U_VERTICES);
    pl.u_edges = graph_tail_u(pl.e_blocks, rq.graph_u);
    pl.graph_rank = rq.mode == GRAPH_FULL && pl.pj && !rq.no_graph_rank;
    pl.pj_tiles_forced = rq.pj_tiles == 1 || rq.pj_tiles == 2 ? rq.pj_tiles : 0u;
    return JS_OK;
}

// Level 1's tiles per thread block for the launch over assemblies [a_lo, a_hi) of a two-level plan (sub-ranges: one assembly per
// launch; else one launch for all)
inline uint32_t pj1_launch_tiles(const JoinShape &pl, uint32_t a_lo, uint32_t a_hi)
{
    const uint32_t tiles = (pl.bstart[a_hi] - pl.bstart[a_lo] + PJ_IPB / 256 - 1) / (PJ_IPB / 256);
    return pj1_tiles(tiles, pl.rec12, pl.pj_tiles_forced);
}

// build_graph_impl's answer to an LDS join that reported failure
enum JoinRetry { RC_RETRY_GLOBAL = 1, RC_RETRY_PJ = 2 };

// A two-level join failed and no table was forced to: was it a coarse partition's (sub-range's) capacity, and only that?  `cur`
// is the cursor table as the device left it (P1 * n_sub cursors, PJ1_CS words apart).  RC_RETRY_PJ: `learnt` now holds what the
// cursors ask for, and a plan made with it has room.  RC_RETRY_GLOBAL: a partition's LDS table overflowed, or the capacities
// were learnt from these very counts already.
inline JoinRetry join_overflow_verdict(const JoinShape &pl, const uint32_t *cur, JoinLearnt &learnt)
{
    const uint32_t P1 = pl.P1, n_sub = pl.n_sub;
    uint64_t mx = 0;  // the fullest coarse partition, all assemblies together: what the one-cursor layout must hold
    for (uint32_t c = 0; c < P1; ++c) {
        uint64_t all = 0;
        for (uint32_t s = 0; s < n_sub; ++s) all += cur[((size_t)c * n_sub + s) * PJ1_CS];
        mx = std::max(mx, all);
    }
    if (pl.split) {
        // a sub-range outgrew its capacity: the next fused call sizes that assembly's sub-ranges by what the cursors counted,
        // and the attempt that follows this one (one cursor per coarse partition) by the partitions' totals
        bool grew = false;
        if (learnt.sub_P1 != P1) std::fill_n(learnt.sub_need, MXG_MAX_ASSEMBLIES, 0ull);
        learnt.sub_P1 = P1;
        for (uint32_t s = 0; s < n_sub; ++s) {
            uint64_t ms = 0;
            for (uint32_t c = 0; c < P1; ++c) ms = std::max<uint64_t>(ms, cur[((size_t)c * n_sub + s) * PJ1_CS]);
            if (ms > pl.sub_cap[s] && learnt.sub_need[s] < ms) {
                learnt.sub_need[s] = ms + ms / 8 + 4096;
                grew = true;
            }
        }
        if (grew) {
            if (learnt.cap1_P1 != P1) learnt.cap1_need = 0;
            learnt.cap1_P1 = P1;
            learnt.cap1_need = std::max<uint64_t>(learnt.cap1_need, mx + mx / 8 + 4096);
            return RC_RETRY_PJ;
        }
    } else if (mx > pl.cap1 && (learnt.cap1_P1 != P1 || learnt.cap1_need < mx)) {
        learnt.cap1_P1 = P1;
        learnt.cap1_need = mx + mx / 8 + 4096;
        return RC_RETRY_PJ;
    }
    return RC_RETRY_GLOBAL;
}

}  // namespace mxg
