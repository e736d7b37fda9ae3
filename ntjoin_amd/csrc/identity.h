// identity.h -- the edit distance of one segment: two stretches of bases whose ends the graph has pinned (mxg_identity_segments,
// DESIGN.md 4p).  identity.hip runs idy_align on the device, one lane per segment; tools/identity_check.cpp runs it on the host.
// Compiles for host and device.
//
// A segment has lq query bases Q[1 .. lq] and ls subject bases S[1 .. ls], d = ls - lq.  The DP runs over the diagonals
// lo = min(0, d) - E .. hi = max(0, d) + E (diagonal of cell (i, j): j - i), at most 64 of them; cells outside are +infinity.
// The band is one 64-bit word that moves down one row per column (Hyyro 2003): in column j bit b stands for row i = j - hi + b.
//   Pv / Mv   bit b: D[i][j] - D[i-1][j] is +1 / -1 (bit 0 looks out of the band and is never read)
//   Eq        bit b: Q[i] == S[j]; 0 for rows outside 1 .. lq
// Going from column j - 1 to column j, the cell at new bit b has its diagonal neighbour at old bit b, its left neighbour at old
// bit b + 1 and its upper neighbour at new bit b - 1:
//   PvS = Pv >> 1, MvS = (Mv >> 1) & band      the left neighbours' vertical deltas; the lowest diagonal's left neighbour lies
//                                              outside the band, so it may not pull the cell down
//   D0  = (((Eq & PvS) + PvS) ^ PvS) | Eq | MvS   the cell equals its diagonal neighbour
//   Ph  = MvS | ~(D0 | PvS), Mh = PvS & D0        horizontal deltas
//   Pv  = (Mh << 1) | ~(D0 | (Ph << 1)), Mv = D0 & (Ph << 1)
// Rows above the matrix (i <= 0 in the first hi columns) hold D[i][j] = j - i, which satisfies the recurrence with Eq = 0 and
// gives row 0 its values D[0][j] = j; rows below lq are never read by a row above them.  The score is carried along the diagonal
// of the last cell, bit hi - d: it starts as |d| in column 0 and grows by one in every column whose D0 bit there is clear.
// The query enters the Eq masks one base per column at bit 63, the masks shift down with the band.
#pragma once
#include <cstdint>

#include "ntjoin_mx.h"

#if defined(__HIPCC__)
#define IDY_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define IDY_HD inline
#endif

namespace mxg {

// byte class as text_index.h's byte_class: 0..3 = A C G T(U) in either case, 4 = any other base, 5 = a line break
IDY_HD uint32_t idy_byte_class(uint32_t b)
{
    if (b == '\n' || b == '\r') return 5u;
    const uint32_t u = b & 0xDFu;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : (u == 'T' || u == 'U') ? 3u : 4u;
}

// the first rule that keeps a segment from being aligned, or MXG_IDY_ALIGNED; needs no base
IDY_HD uint32_t idy_precheck(uint32_t lq, uint32_t ls, uint32_t max_seg)
{
    if (lq > max_seg || ls > max_seg) return MXG_IDY_SKIP_LEN;
    const int64_t d = (int64_t)ls - (int64_t)lq;
    if (d > (int64_t)MXG_IDY_MAX_SHIFT || d < -(int64_t)MXG_IDY_MAX_SHIFT) return MXG_IDY_SKIP_SHIFT;
    return MXG_IDY_ALIGNED;
}

// A segment that idy_precheck lets through.  q.next() / s.next() hand out the classes (0 .. 4) of Q[1], Q[2], ... and of S[1],
// S[2], ... (the subject's fetcher reverses and complements); each is called at most lq / ls times.  Returns MXG_IDY_SKIP_N at
// the first class 4 -- every base of either side is fetched before the last column ends -- else MXG_IDY_ALIGNED with *edits and
// *saturated (edits > |d| + 2 E: the value is the band's, an upper bound of the distance).
template <class FQ, class FS> IDY_HD uint32_t idy_align(FQ &q, FS &s, uint32_t lq, uint32_t ls, uint32_t *edits, uint32_t *saturated)
{
    const int32_t d = (int32_t)ls - (int32_t)lq;
    const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
    const uint32_t hi = (d > 0 ? (uint32_t)d : 0u) + MXG_IDY_E;  // <= 47
    const uint32_t width = ad + 2u * MXG_IDY_E + 1u;              // diagonals: 33 .. 64
    const uint64_t band = ~0ull >> (65u - width);                 // bits 0 .. width - 2
    const uint32_t tbit = hi - (uint32_t)d;                       // the last cell's diagonal: E or E + |d|
    uint64_t peq[4] = {0, 0, 0, 0};
    uint32_t fed = 0;  // query bases fetched
    // column 0: bit b is row b - hi; rows 1 .. 63 - hi enter the masks
    {
        const uint32_t pre = lq < 63u - hi ? lq : 63u - hi;
        for (; fed < pre; ++fed) {
            const uint32_t c = q.next();
            if (c > 3u) return MXG_IDY_SKIP_N;
            const uint64_t bit = 1ull << (hi + 1u + fed);  // (selects, not an index: the masks stay in registers)
            peq[0] |= c == 0u ? bit : 0ull;
            peq[1] |= c == 1u ? bit : 0ull;
            peq[2] |= c == 2u ? bit : 0ull;
            peq[3] |= c == 3u ? bit : 0ull;
        }
    }
    uint64_t Mv = ~0ull >> (63u - hi);  // rows <= 0: D falls towards row 0
    uint64_t Pv = ~Mv;                  // rows >= 1: D[i][0] = i
    uint32_t score = ad;
    for (uint32_t j = 1; j <= ls; ++j) {
        const uint32_t c = s.next();
        if (c > 3u) return MXG_IDY_SKIP_N;
        peq[0] >>= 1, peq[1] >>= 1, peq[2] >>= 1, peq[3] >>= 1;
        if (fed < lq) {  // row j - hi + 63
            const uint32_t cq = q.next();
            if (cq > 3u) return MXG_IDY_SKIP_N;
            ++fed;
            const uint64_t top = 1ull << 63;
            peq[0] |= cq == 0u ? top : 0ull;
            peq[1] |= cq == 1u ? top : 0ull;
            peq[2] |= cq == 2u ? top : 0ull;
            peq[3] |= cq == 3u ? top : 0ull;
        }
        const uint64_t Eq = c == 0u ? peq[0] : c == 1u ? peq[1] : c == 2u ? peq[2] : peq[3];
        const uint64_t PvS = Pv >> 1, MvS = (Mv >> 1) & band;
        const uint64_t D0 = (((Eq & PvS) + PvS) ^ PvS) | Eq | MvS;
        const uint64_t Ph = MvS | ~(D0 | PvS), Mh = PvS & D0;
        Pv = (Mh << 1) | ~(D0 | (Ph << 1));
        Mv = D0 & (Ph << 1);
        score += (uint32_t)(~D0 >> tbit) & 1u;
    }
    *edits = score;
    *saturated = score > ad + 2u * MXG_IDY_E ? 1u : 0u;
    return MXG_IDY_ALIGNED;
}

}  // namespace mxg
