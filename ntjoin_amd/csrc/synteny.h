// synteny.h -- synteny blocks between two assemblies of one graph (mxg_synteny_blocks): the rules of one anchor and
// of one pair of neighbouring anchors.  synteny.hip runs the functions below on the device, one thread per anchor or per piece;
// tools/synteny_check.cpp runs them serially on the host.  Compiles for host and device.
//
// An ANCHOR is a graph vertex seen from a query assembly q and a subject assembly s: where it lies in each.  The anchor list is in
// (query record, query position) order, or rebuilt through a piece table over the records of q (compose.h): piece by piece, a REV
// piece's anchors in falling order of their old position.  Neighbouring anchors i, i + 1 are LINKED with a direction when they
// share both records, their subject positions differ, and neither distance exceeds max_gap (0: no bound).  A BLOCK is a maximal run
// of links of one direction: link i is its HEAD when link i - 1 has another code, its TAIL when link i + 1 has.
#pragma once
#include <cstdint>

#include "bisect.h"
#include "ntjoin_mx.h"

#if defined(__HIPCC__)
#define SYN_HD __host__ __device__ inline
#else
#define SYN_HD inline
#endif

namespace mxg {

struct SynAnchor {  // 16 bytes: one aligned load
    uint32_t qrec, qpos, srec, spos;
};

enum : uint32_t { SYN_NONE = 0, SYN_FWD = 1, SYN_REV = 2 };  // the code of a link

// the link between an anchor and its successor in the list
SYN_HD uint32_t syn_link(const SynAnchor &a, const SynAnchor &b, uint32_t max_gap)
{
    if (a.qrec != b.qrec || a.srec != b.srec || a.spos == b.spos) return SYN_NONE;
    const int64_t dq = (int64_t)b.qpos - (int64_t)a.qpos, ds = (int64_t)b.spos - (int64_t)a.spos;
    if (max_gap && (dq > (int64_t)max_gap || (ds < 0 ? -ds : ds) > (int64_t)max_gap)) return SYN_NONE;
    return ds > 0 ? SYN_FWD : SYN_REV;
}

// link i with code c (not SYN_NONE) between links of codes prev and next (SYN_NONE where there is no such link)
SYN_HD bool syn_is_head(uint32_t prev, uint32_t c) { return c != SYN_NONE && prev != c; }
SYN_HD bool syn_is_tail(uint32_t c, uint32_t next) { return c != SYN_NONE && next != c; }

// the code of link i of a list of n anchors (links 0 .. n - 2); anything outside is SYN_NONE
SYN_HD uint32_t syn_link_at(const SynAnchor *a, uint64_t n, int64_t i, uint32_t max_gap)
{
    if (i < 0 || (uint64_t)i + 1 >= n) return SYN_NONE;
    return syn_link(a[i], a[i + 1], max_gap);
}

// the first anchor of a[0, n), sorted by (qrec, qpos), that is not below (rec, pos)
SYN_HD uint64_t syn_lower_bound(const SynAnchor *a, uint64_t n, uint32_t rec, uint32_t pos)
{
    const uint64_t key = (uint64_t)rec << 32 | pos;
    return first_where((uint64_t)0, n, [&](uint64_t i) { return ((uint64_t)a[i].qrec << 32 | a[i].qpos) >= key; });
}

// the anchors [lo, hi) a FWD / REV piece takes: those of its record with start <= qpos and qpos + k <= end
SYN_HD void syn_piece_range(const SynAnchor *a, uint64_t n, const mxg_seq_piece &p, uint32_t k, uint64_t &lo, uint64_t &hi)
{
    lo = hi = 0;
    if (p.kind == MXG_PIECE_GAP || p.end < k || p.end - k < p.start) return;
    lo = syn_lower_bound(a, n, p.record, p.start);
    hi = syn_lower_bound(a, n, p.record, p.end - k + 1u);  // (the first position that no longer fits; k >= 1: no wrap)
}

// the t-th anchor (in the new record's order) of a piece that takes a[lo, hi) and starts at base `off` of the new record `rec`
SYN_HD SynAnchor syn_piece_anchor(const SynAnchor *a, const mxg_seq_piece &p, uint32_t k, uint64_t lo, uint64_t hi, uint64_t t, uint32_t rec,
                                  uint32_t off)
{
    const bool rev = p.kind == MXG_PIECE_REV;
    const SynAnchor in = a[rev ? hi - 1 - t : lo + t];
    SynAnchor o;
    o.qrec = rec;
    o.qpos = rev ? off + (p.end - (in.qpos + k)) : off + (in.qpos - p.start);
    o.srec = in.srec;
    o.spos = in.spos;
    return o;
}

struct SynBlock {
    uint32_t n_anchors, q_record, q_start, q_end, s_record, s_start, s_end, reverse;
};

// the block of links j .. t (head j, tail t) over anchors j .. t + 1: its fields come from its first and last anchor alone, since
// it is monotone in both coordinates.  q_end and s_end as 64-bit sums: the caller checks them against the record lengths it has
SYN_HD SynBlock syn_block(const SynAnchor &first, const SynAnchor &last, uint64_t j, uint64_t t, uint32_t k)
{
    SynBlock b;
    b.n_anchors = (uint32_t)(t - j + 2);
    b.q_record = first.qrec;
    b.q_start = first.qpos;
    b.q_end = last.qpos + k;
    b.s_record = first.srec;
    b.s_start = first.spos < last.spos ? first.spos : last.spos;
    b.s_end = (first.spos < last.spos ? last.spos : first.spos) + k;
    b.reverse = last.spos < first.spos ? 1u : 0u;
    return b;
}

SYN_HD bool syn_keep(const SynBlock &b, uint32_t min_anchors, uint32_t min_span)
{
    return b.n_anchors >= min_anchors && b.q_end - b.q_start >= min_span;
}

// PAF columns 10 and 11 of a block
SYN_HD uint64_t syn_matches(const SynBlock &b, uint32_t k)
{
    const uint64_t q = b.q_end - b.q_start, s = b.s_end - b.s_start, m = (uint64_t)b.n_anchors * k;
    return m < q ? (m < s ? m : s) : (q < s ? q : s);
}
SYN_HD uint64_t syn_blocklen(const SynBlock &b)
{
    const uint64_t q = b.q_end - b.q_start, s = b.s_end - b.s_start;
    return q > s ? q : s;
}

}  // namespace mxg
