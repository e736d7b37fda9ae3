// The request array between k_bs_select and k_sel_stretch (sketch_bs.hip), the one place that knows what happens at its capacity.
// Plain C++: the kernels and a CPU test (tests/test_sel_requests_cpu.py) share one statement of it.
//
// A slice with n_i <= SEL_REQ stretches between two of its candidates reserves n_i consecutive entries with ONE add to the batch's
// counter (CW_SEL_REQS) and lane q < n_i fills entry base + q: {contig, first k-mer, last k-mer, sel_req_word(slice, q, n_i)}.
// Reservations are handed out back to back from 0 on, so entry e < the counter's end value belongs to exactly one of them.
// k_sel_stretch walks the entries [0, min(counter, cap)): the wave that meets a slice's FIRST entry (q = 0) takes all n_i of the
// slice, entries with q != 0 are stepped over.  The array is never cleared, so every entry the walk visits must have been written
// by this batch:
//   - a reservation with base + n_i <= cap: every lane writes its request;
//   - a reservation that straddles the capacity (base < cap < base + n_i): the lanes with base + q < cap write a TOMBSTONE, an
//     entry whose number in the slice is not 0, which the walk steps over, and ALL n_i stretches of the slice go to k_gap_fix instead (a slice's
//     stretches go into one row: they stay together);
//   - a reservation at or behind the capacity, and the base of a batch without that kernel (SEL_REQ_NO_KERNEL): nothing is
//     written, the stretches go to k_gap_fix.
// A first entry at r therefore has r + n_i <= cap: the lanes q < n_i of the wave that takes it never read at or behind cap.
#pragma once
#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MXG_SEL_REQ_FN __host__ __device__ __forceinline__
#else
#define MXG_SEL_REQ_FN inline
#endif

namespace mxg {

constexpr uint32_t SEL_REQ = 8;               // stretches per slice that become requests (and: whose end lies behind the slice's strips)
constexpr uint32_t SEL_IREQ_SPARE = 8;        // entries behind the capacity: the walk reads SEL_REQ entries from any request on
constexpr uint32_t SEL_IREQ_CAP = 1u << 18;   // entries of the array (the upper part of the stretch array): capacity + spare
constexpr uint32_t SEL_IREQ_USABLE = SEL_IREQ_CAP - SEL_IREQ_SPARE;  // requests a batch's array takes (MXG_SEL_IREQ_CAP: fewer)
constexpr uint32_t SEL_REQ_NO_KERNEL = 0xFFFFFFFFu - SEL_REQ;        // "base" of a slice in a batch without k_sel_stretch
static_assert(SEL_REQ == SEL_IREQ_SPARE && SEL_REQ <= 8, "the number in the slice has three bits, the count four");

// fourth word of an entry: slice (24 bits) | number in the slice (3 bits) | stretches of the slice (5 bits)
MXG_SEL_REQ_FN uint32_t sel_req_word(uint32_t slice, uint32_t q, uint32_t n_i) { return slice | (q << 24) | (n_i << 27); }
// a tombstone: the lane's own entry with every bit of the number in the slice set -- never a first entry, whatever the lane (the
// slice kernel has the entry at hand: one select more on the path of a slice with stretches, no register more on any other)
constexpr uint32_t SEL_REQ_TOMBSTONE = 7u << 24;
MXG_SEL_REQ_FN uint32_t sel_req_tombstone(uint32_t word) { return word | SEL_REQ_TOMBSTONE; }
MXG_SEL_REQ_FN uint32_t sel_req_number(uint32_t word) { return (word >> 24) & 7u; }
MXG_SEL_REQ_FN uint32_t sel_req_count(uint32_t word) { return word >> 27 < SEL_REQ ? word >> 27 : SEL_REQ; }
MXG_SEL_REQ_FN uint32_t sel_req_slice(uint32_t word) { return word & 0xFFFFFFu; }
// does the walk take the slice of this entry?  (the bound on the slice costs nothing and keeps an entry that no rule above
// accounts for from indexing the slices' rows and counts)
MXG_SEL_REQ_FN bool sel_req_is_first(uint32_t word, uint32_t n_slices)
{
    return sel_req_number(word) == 0u && sel_req_count(word) != 0u && sel_req_slice(word) < n_slices;
}

enum SelReqSlot : uint32_t {
    SEL_SLOT_NONE = 0,       // the lane writes nothing (its stretch, if it has one, goes to k_gap_fix)
    SEL_SLOT_WRITE = 1,      // entry base + lane takes the lane's request
    SEL_SLOT_TOMBSTONE = 2,  // entry base + lane takes a tombstone, the lane's stretch goes to k_gap_fix
};
// what lane `lane` of a slice that reserved [base, base + n_i) does with entry base + lane of an array of `cap` usable entries
// (differences only: no sum that could wrap, whatever the base)
MXG_SEL_REQ_FN SelReqSlot sel_req_slot(uint32_t base, uint32_t n_i, uint32_t lane, uint32_t cap)
{
    if (lane >= n_i || base >= cap) return SEL_SLOT_NONE;
    const uint32_t room = cap - base;
    if (n_i <= room) return SEL_SLOT_WRITE;
    return lane < room ? SEL_SLOT_TOMBSTONE : SEL_SLOT_NONE;
}
// entries of the array the walk visits for a counter's end value
MXG_SEL_REQ_FN uint32_t sel_req_walk(uint32_t counter, uint32_t cap) { return counter < cap ? counter : cap; }

}  // namespace mxg
