// The control words of a sketch batch, the one place that knows their layout, that of SC_CTRL behind them, and the launch
// arithmetic that goes with them.  A batch has two blocks of 16 words:
// - the DEVICE block: the first CTRL_WORDS words of the batch's SC_CTRL scratch, zeroed before its first kernel; the batch's
//   kernels count and raise flags in it, the pack kernels (sketch.hip, dgraph.hip) read it;
// - the HOST REPORT: the batch's slot of pinned host memory (mxg_handle::pinned_ctrl), which k_emit's reporting tile writes,
//   all 16 words at once, at the end of the batch.  The host reads it after the stream has drained.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

namespace mxg {

// ---- device block
enum CtrlWord : uint32_t {
    CW_ARENA_NEED = 0,       // arena overflow: the largest wave's candidate count where it exceeds the wave's slice (0: none)
    CW_STRETCHES = 1,        // candidate-free stretches pushed (k_resolve, k_bs_select, k_sel_stretch)
    CW_SELECTED = 2,         // [2..3] selected candidates, 64 bit
    CW_CAND = 4,             // [4..5] candidates, 64 bit
    CW_REDO = 6,             // "the host must redo the batch" (the stretch kernels, k_bs_select)
    CW_STRETCH_MX = 7,       // minimizers found in the stretches (k_gap_post)
    CW_GAP_KMERS = 10,       // k-mers of the stretches hashed on the device (k_gap_fix)
    CW_DEFERRED = 11,        // stretches deferred to the host (defer_stretch)
    CW_REGION_TICKET = 12,   // the next of k_bs_select's global-memory regions for slices beyond their queue
    CW_SLICE_GAVE_UP = 13,   // k_bs_select gave up on a slice (it raises CW_REDO too)
    CW_REGION_ENTRIES = 14,  // entries of the stretches' minimizer pool handed out (k_gap_fix)
    CW_SEL_REQS = 15,        // requests for k_sel_stretch
};
constexpr uint32_t CTRL_WORDS = 16;  // (words 8 and 9 are unused)

// ---- host report.  Its words derive from the device block's as k_emit finds it: a batch with an arena overflow or without any
// candidate reports RW_ARENA_NEED and RW_STRETCHES only, every other word 0.  Words 13 and 14 are always 0.
enum ReportWord : uint32_t {
    RW_ARENA_NEED = 0,       // CW_ARENA_NEED
    RW_STRETCHES = 1,        // CW_STRETCHES
    RW_SELECTED = 2,         // CW_SELECTED (32 bit)
    RW_REDO = 3,             // CW_REDO (device route, k_bs_select), or: more stretches than k_emit's launch had placing blocks for
    RW_CAND = 4,             // CW_CAND (32 bit)
    RW_STRETCH_MX = 5,       // CW_STRETCH_MX if k_emit placed the stretches' minimizers, else 0
    RW_TOTAL = 6,            // [6..7] minimizers of the batch, RW_SELECTED + RW_STRETCH_MX, 64 bit
    RW_OUT_BASE = 8,         // [8..9] where the batch starts in the assembly's sketch, 64 bit
    RW_GAP_KMERS = 10,       // CW_GAP_KMERS on the device route, else 0
    RW_DEFERRED = 11,        // CW_DEFERRED on the device route unless RW_REDO, else 0
    RW_SLICE_GAVE_UP = 12,   // CW_SLICE_GAVE_UP
    RW_SEL_REQS = 15,        // CW_SEL_REQS behind k_bs_select, else 0
};
constexpr uint32_t REPORT_WORDS = 16, REPORT_BYTES = 64;  // a pinned slot
static_assert(REPORT_WORDS * sizeof(uint32_t) == REPORT_BYTES, "a report fills its pinned slot");
static_assert(RW_SEL_REQS < REPORT_WORDS && CW_SEL_REQS < CTRL_WORDS, "every word lies in its block");
// the host fills a slot with this before it enqueues the batch: a report still unset after the stream has drained was never
// written (no tile held the batch's last candidate: more candidates than the launch's grid covered)
constexpr uint32_t REPORT_UNSET = 0xFFFFFFFFu;

// A report as the host reads it.  Counts that a batch may leave unset read as 0.
struct BatchReport {
    const uint32_t *w;
    bool reported() const { return w[RW_CAND] != REPORT_UNSET; }
    uint32_t arena_need() const { return w[RW_ARENA_NEED]; }
    uint32_t n_stretches() const { return w[RW_STRETCHES]; }
    uint32_t n_selected() const { return w[RW_SELECTED]; }
    uint32_t n_cand() const { return w[RW_CAND]; }
    uint64_t total() const { return (uint64_t)w[RW_TOTAL] | ((uint64_t)w[RW_TOTAL + 1] << 32); }
    uint64_t out_base() const { return (uint64_t)w[RW_OUT_BASE] | ((uint64_t)w[RW_OUT_BASE + 1] << 32); }
    uint32_t gap_kmers() const { return w[RW_GAP_KMERS] == REPORT_UNSET ? 0u : w[RW_GAP_KMERS]; }
    uint32_t n_deferred() const { return w[RW_DEFERRED] == REPORT_UNSET ? 0u : w[RW_DEFERRED]; }
    uint32_t sel_requests() const { return w[RW_SEL_REQS] == REPORT_UNSET ? 0u : w[RW_SEL_REQS]; }
    // Did the batch end the common way: reported, no arena overflow, nothing raised, at least one candidate unless `empty_ok`,
    // and its stretches, if any, placed by the device route (`dev_route`) -- where the stretches it deferred to the host are
    // acceptable only if `deferred_ok` (the host merges them in later; a caller that has already used the device's counts
    // cannot).  k_bs_select reports the contigs of a batch without candidates as stretches, so that route may pass
    // `empty_ok`; the other route leaves such a batch to the host.
    bool ended_well(bool dev_route, bool deferred_ok, bool empty_ok) const
    {
        return reported() && arena_need() == 0 && w[RW_REDO] == 0 && w[RW_SLICE_GAVE_UP] == 0 && (n_cand() != 0 || empty_ok) &&
               ((dev_route && (deferred_ok || n_deferred() == 0)) || n_stretches() == 0);
    }
};

// ---- SC_CTRL behind the device block.  One memset zeroes `bytes()` of it before the batch's first kernel; every part below is
// a word offset into SC_CTRL.  The super-count arrays are those of scan_kernels.h: the callers pass sup_words(...) of them, so
// that this header needs no HIP type.
// A row of counters that many waves add to at once: SPREAD_COUNTERS of them, SPREAD_STRIDE words apart (a wave takes one by
// its number), SPREAD_WORDS in all
constexpr uint32_t SPREAD_COUNTERS = 64, SPREAD_STRIDE = 32, SPREAD_WORDS = SPREAD_COUNTERS * SPREAD_STRIDE;
// candidate-array route: the super-counts per hash-kernel wave, sup_words(n_waves), then per k_resolve block,
// sup_words(ceil(n_cap / RK))
struct CandCtrlLayout {
    uint32_t wave_sup, sel_sup, words;
    size_t bytes() const { return (size_t)words * 4; }
};
constexpr CandCtrlLayout cand_ctrl_layout(uint32_t wave_sup_words, uint32_t sel_sup_words)
{
    return {CTRL_WORDS, CTRL_WORDS + wave_sup_words, CTRL_WORDS + wave_sup_words + sel_sup_words};
}
// slice route: the super-counts per slice, sup_words(n_slices), then k_bs_select's candidate counters (BsSelParams::cand_spread),
// then k_sel_stretch's request tickets (SelStretchParams::tickets), a row of SPREAD_WORDS each
struct SliceCtrlLayout {
    uint32_t sup, cand_spread, tickets, words;
    size_t bytes() const { return (size_t)words * 4; }
};
constexpr SliceCtrlLayout slice_ctrl_layout(uint32_t sup_words)
{
    return {CTRL_WORDS, CTRL_WORDS + sup_words, CTRL_WORDS + sup_words + SPREAD_WORDS, CTRL_WORDS + sup_words + 2 * SPREAD_WORDS};
}

// ---- launch arithmetic of a batch that is enqueued without a host sync
// The blocks at the front of k_emit's grid that place the stretches' minimizers, four stretches each: for twice the stretches
// the plan expects of the batch (`gap_rate` per k-mer, `nk` k-mers) + 256, at most for all the per-stretch arrays hold (`gcap`)
// -- once earlier sketches of the assembly have met stretches (`rate_hint` > 0), until then for all of them.  `forced` != 0
// (MXG_GAP_PLACE, a test knob): blocks for that many stretches.  gap_expect: the stretches expected, for the stretch kernels'
// grids (< 0: not known).  place4 = 4 * n_place: the stretches the launch can place (batch_ended_well).
struct GapPlacing {
    uint32_t n_place;
    double gap_expect;
    uint32_t place4;
};
inline GapPlacing gap_placing(uint32_t gcap, double gap_rate, uint64_t nk, double rate_hint, uint64_t forced)
{
    const double expect = gap_rate * (double)nk;
    const uint32_t want = (uint32_t)std::min<double>((double)gcap, 2.0 * expect + 256.0);
    GapPlacing p{rate_hint > 0 ? (want + 3u) / 4u : gcap / 4u, rate_hint > 0 ? expect : -1.0, 0};
    if (forced) p = GapPlacing{(uint32_t)std::min<uint64_t>((forced + 3u) / 4u, gcap / 4u), -1.0, 0};
    p.place4 = 4u * p.n_place;
    return p;
}
// The candidates k_resolve and k_emit are launched for: the EXPECTED number (`nk` k-mers below the filter's threshold `tau_hi`,
// either strand with `min_variant`; `hint`: what the batch held last time) + 30 % + 16384 instead of the arrays' capacity `n_cap`,
// a whole number of k_emit tiles (`tile` = EMIT_COMPACT_BLOCKS * `rk` candidates), so that k_resolve (`rk` candidates per
// block) and k_emit cover the same candidates: a tile that reports must have had all its blocks resolved.  0: the capacity
// (`knob` = MXG_GRID_BY_ESTIMATE is 0).  knob 2 (a test value): too small on purpose.
inline uint32_t grid_by_estimate(uint64_t knob, uint64_t nk, uint32_t tau_hi, bool min_variant, uint64_t hint, uint32_t n_cap,
                                 uint32_t rk, uint32_t tile)
{
    if (!knob) return 0;
    const uint64_t expect = (uint64_t)((double)nk * (double)tau_hi / 4294967296.0) * (min_variant ? 2u : 1u);
    uint64_t gc = std::max(expect, hint) * 13 / 10 + 16384;
    if (knob == 2) gc = std::max<uint64_t>(rk, expect / 2);
    return (uint32_t)std::min<uint64_t>(n_cap, (gc + tile - 1) / tile * tile);
}

#ifdef __HIPCC__
// What is decided about a batch before anything of it is enqueued.  The caller builds one per batch (a default one: a batch the
// host waits for, on its own in the assembly's sketch); the driver only reads it.
struct BatchShape {
    // stretches the device route's per-stretch arrays hold for the batch, the blocks at the front of k_emit's grid that place
    // them, four stretches each (see gap_capacity, gap_placing), and the stretches the plan expects for the stretch kernels
    // (< 0: not known)
    uint32_t gcap = 0, n_place = 0;  // (0: the batch does not take the device route)
    double gap_expect = -1.0;
    uint32_t *n_out = nullptr;  // see EmitParams::n_out (the calls with a stage behind the sketches)
    bool few_cand = false;      // <= 12 candidates per window: smaller k_reorder blocks and k_resolve halos
    // Batches enqueued without a host sync: k_resolve and k_emit are launched for the EXPECTED number of candidates (+ 30 %)
    // instead of the arrays' capacity (about 2.7 x the expectation), so that half their blocks do not start just to find
    // nothing to do -- blocks that each hold a wave slot for a memory round trip beside the other stream's hash kernel.  A batch
    // with more candidates than that never reports (no tile holds its last candidate): the host redoes the assembly.
    uint32_t grid_cand = 0;     // 0: the capacity (grid_by_estimate)
    bool may_hold_emit = false;  // the slice route may hold the batch's k_emit back (Driver::flush_emit)
    // how the batch hangs together with the batches before it and with the device-side stretch fix-up (see EmitParams)
    bool chained = false;  // enqueued without a host sync, by SketchStep
    const uint64_t *base_in = nullptr;
    uint64_t *base_out = nullptr;
    bool dev_gaps = false;  // candidate-free stretches are sketched on the device
    hipEvent_t wait = nullptr;  // recorded behind the previous batch of the assembly when that ran on the other stream
    uint32_t ecb = 0;           // slices per k_emit tile behind k_bs_select (0: the default)
};

// Which route left the selection that k_emit places, and where in the driver's scratch
struct EmitSource {
    enum Route { TILE_SUMS, RESOLVE, SLICES } route;
    uint32_t sup;          // RESOLVE, SLICES: the word of SC_CTRL where the selection's super-counts start
    uint32_t rk;           // candidates per counted block: k_resolve's threads, or a slice's entries
    uint32_t n_fixed;      // SLICES: the entries the grid covers (every slice's), else 0
    uint32_t cand_spread;  // SLICES: the word of SC_CTRL where k_bs_select's candidate counters start, else 0
    // per 1024-tile sums in SC_BSUM (resolve_and_count)
    static EmitSource tile_sums(uint32_t rk) { return {TILE_SUMS, 0, rk, 0, 0}; }
    // k_resolve's two-level counts and per-block layout (resolve_count)
    static EmitSource resolve(const CandCtrlLayout &l, uint32_t rk) { return {RESOLVE, l.sel_sup, rk, 0, 0}; }
    // k_bs_select's, one 16-byte entry per selected candidate
    static EmitSource slices(const SliceCtrlLayout &l, uint32_t rk, uint32_t n_ent) { return {SLICES, l.sup, rk, n_ent, l.cand_spread}; }
};

// BatchReport::ended_well(dev_gaps, false, false) read from the device block while the batch may still be in flight on the
// stream, for the pack kernels.  k_emit has not folded "more stretches than its launch had placing blocks for" into a report
// here, so that test is made directly: `place4` = 4 x k_emit's placing blocks.
__device__ __forceinline__ bool batch_ended_well(const uint32_t *ctrl, uint32_t dev_gaps, uint32_t place4)
{
    return ctrl[CW_ARENA_NEED] == 0 && ctrl[CW_REDO] == 0 && ctrl[CW_SLICE_GAVE_UP] == 0 &&
           (dev_gaps ? (ctrl[CW_DEFERRED] == 0 && ctrl[CW_STRETCHES] <= place4) : ctrl[CW_STRETCHES] == 0) &&
           (ctrl[CW_CAND] | ctrl[CW_CAND + 1]) != 0;
}
#endif

}  // namespace mxg
