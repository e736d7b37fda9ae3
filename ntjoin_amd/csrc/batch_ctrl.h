// The control words of a sketch batch, the one place that knows their layout.  A batch has two blocks of 16 words:
// - the DEVICE block: the first CTRL_WORDS words of the batch's SC_CTRL scratch, zeroed before its first kernel; the batch's
//   kernels count and raise flags in it, the pack kernels (sketch.hip, dgraph.hip) read it;
// - the HOST REPORT: the batch's slot of pinned host memory (mxg_handle::pinned_ctrl), which k_emit's reporting tile writes,
//   all 16 words at once, at the end of the batch.  The host reads it after the stream has drained.
#pragma once
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

#ifdef __HIPCC__
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
