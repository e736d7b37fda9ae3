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

}  // namespace mxg
