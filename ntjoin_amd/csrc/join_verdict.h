// The words the partitioned join leaves in slot[a][i], the one place that knows them: the kernels that partition the minimizers
// (k_pj1_scatter, k_pj_bucket) write the prefill, the join kernels skip every verdict that equals it, k_flags_pj reads whichever
// is there.  No device, no handle: tests/test_join_verdict_cpu.py compiles this header on its own.
#pragma once
#include <cstdint>

#include "ntjoin_mx.h"

#if defined(__HIPCC__)
#define PJV_HD __host__ __device__ inline
#else
#define PJV_HD inline
#endif

namespace mxg {

// A verdict word: (shared: the key's minimizer in assembly 0) << 3 | MXG_MX_* flags.  The commonest word that carries nothing
// above its flags is "once in its assembly, not in every assembly": the partitioning kernels write it for every minimizer, in
// order, and the join sends only the words that differ.
constexpr uint32_t PJ_VERDICT_PREFILL = MXG_MX_UNIQUE;
// low bits of a verdict word that is no verdict (SHARED without UNIQUE cannot be): the upper bits name a minimizer of the same
// assembly whose verdict holds for this one (k_pj2_bucket's skew path)
constexpr uint32_t PJ_VERDICT_REF = 2u;

PJV_HD bool pj_verdict_is_prefill(uint32_t word) { return word == PJ_VERDICT_PREFILL; }

// The second prefill rule (two-level join).  Where most of assembly 0's minimizers are shared, the commonest word of assembly 0 is
// "shared, and the key's minimizer in assembly 0 is this very one": (i << 3) | UNIQUE | SHARED | INALL, which k_pj1_scatter can
// write in order as well.  The other assemblies keep PJ_VERDICT_PREFILL.  Which rule a build takes is decided on the host from
// what an earlier build of the same sketches counted (JoinLearnt::prefill_own0, join_plan.h).
// Neither prefill can be taken for one of the other words a partitioning kernel leaves: 0 (a record beyond its sub-range's
// capacity) has no flag, a reference has the low bits PJ_VERDICT_REF; the prefills' low bits are 1 and 7.
enum PjPrefillRule : uint32_t { PJ_PREFILL_UNIQUE = 0, PJ_PREFILL_OWN0 = 1 };
constexpr uint32_t PJ_VERDICT_SHARED = MXG_MX_UNIQUE | MXG_MX_SHARED | MXG_MX_INALL;

// the word the partitioning kernel writes for minimizer i of assembly a, and the join does not send
PJV_HD uint32_t pj_verdict_prefill(uint32_t rule, uint32_t a, uint32_t i)
{
    return rule == PJ_PREFILL_OWN0 && a == 0 ? (i << 3) | PJ_VERDICT_SHARED : PJ_VERDICT_PREFILL;
}

}  // namespace mxg
