// assess.h -- reference-based assessment of the kept synteny blocks (mxg_synteny_assess): the rules of one pair of
// neighbouring blocks, of one chain, of one pair of neighbouring chains, of the Nx figures and of the union of subject intervals.
// assess.hip runs the functions below on the device, one thread per block, chain or chain boundary; tools/assess_check.cpp runs
// them serially on the host.  Compiles for host and device.
//
// Blocks i and i + 1 are JOINED when they agree in both records and in direction, the second starts beyond the first one's last
// anchor on both assemblies, neither gap exceeds merge_gap and the two gaps differ by no more than max_indel -- join_indel where
// the two blocks lie in different pieces of the query record (a join the scaffolder made).  A CHAIN is a maximal run of joined
// blocks; a BREAKPOINT is a pair of neighbouring chains of one query record.
#pragma once
#include <cstdint>

#include "compose.h"
#include "ntjoin_mx.h"
#include "synteny.h"

namespace mxg {

// block i of the eight arrays of n words k_syn_compact writes (the order of SynBlock's fields)
SYN_HD SynBlock as_block(const uint32_t *blk, uint64_t n, uint64_t i)
{
    SynBlock b;
    b.n_anchors = blk[i], b.q_record = blk[n + i], b.q_start = blk[2 * n + i], b.q_end = blk[3 * n + i];
    b.s_record = blk[4 * n + i], b.s_start = blk[5 * n + i], b.s_end = blk[6 * n + i], b.reverse = blk[7 * n + i];
    return b;
}

// the piece of query record r that holds base x (pre: every piece's offset in its record, first: n_records + 1 offsets into pre);
// without a table (pre == nullptr) every record is one piece
SYN_HD uint32_t as_piece_of(const uint32_t *pre, const uint32_t *first, uint32_t r, uint32_t x)
{
    if (!pre) return 0u;
    return last_le(pre + first[r], 0u, first[r + 1] - first[r], x);  // (its prefix starts at 0 and rises, at least one piece)
}

// does the border between block a and its successor b (same query record) fall on a change of piece
SYN_HD bool as_at_join(const SynBlock &a, const SynBlock &b, const uint32_t *pre, const uint32_t *first)
{
    return as_piece_of(pre, first, a.q_record, a.q_end - 1u) != as_piece_of(pre, first, a.q_record, b.q_start);
}

SYN_HD bool as_joined(const SynBlock &a, const SynBlock &b, uint32_t k, const mxg_assess_params &p, const uint32_t *pre, const uint32_t *first)
{
    if (a.q_record != b.q_record || a.s_record != b.s_record || (a.reverse != 0) != (b.reverse != 0)) return false;
    const int64_t gq = (int64_t)b.q_start - (int64_t)a.q_end;
    const int64_t gs = a.reverse ? (int64_t)a.s_start - (int64_t)b.s_end : (int64_t)b.s_start - (int64_t)a.s_end;
    const int64_t least = 1 - (int64_t)k;
    if (gq < least || gs < least) return false;
    if (p.merge_gap && (gq > gs ? gq : gs) > (int64_t)p.merge_gap) return false;
    const uint32_t bound = as_at_join(a, b, pre, first) ? p.join_indel : p.max_indel;
    const int64_t d = gq > gs ? gq - gs : gs - gq;
    return !bound || d <= (int64_t)bound;
}

struct AsChain {
    uint32_t n_blocks, first_block, n_anchors, q_record, q_start, q_end, s_record, s_start, s_end, reverse;
};
constexpr uint32_t AS_CHAIN_FIELDS = 10;

// the chain of blocks f .. l (a its first, b its last block), n_anchors = the sum of their counts
SYN_HD AsChain as_chain(const SynBlock &a, const SynBlock &b, uint32_t f, uint32_t l, uint32_t n_anchors)
{
    AsChain c;
    c.n_blocks = l - f + 1u;
    c.first_block = f;
    c.n_anchors = n_anchors;
    c.q_record = a.q_record;
    c.q_start = a.q_start;
    c.q_end = b.q_end;
    c.s_record = a.s_record;
    c.s_start = a.s_start < b.s_start ? a.s_start : b.s_start;
    c.s_end = a.s_end > b.s_end ? a.s_end : b.s_end;
    c.reverse = a.reverse ? 1u : 0u;
    return c;
}

// the kind of the breakpoint between two neighbouring chains of one query record
SYN_HD uint32_t as_kind(uint32_t s_rec_a, uint32_t rev_a, uint32_t s_rec_b, uint32_t rev_b)
{
    if (s_rec_a != s_rec_b) return MXG_BP_TRANSLOCATION;
    if ((rev_a != 0) != (rev_b != 0)) return MXG_BP_INVERSION;
    return MXG_BP_RELOCATION;
}

// ---- Nx: lengths sorted descending, ex[j] = the sum of the first j (ex: n + 1 entries).  Lx = the smallest j >= 1 with
// 100 ex[j] >= x D, or 0 when none reaches it or D == 0
SYN_HD bool as_nx_reached(uint64_t s, uint32_t x, uint64_t d)
{
    return (unsigned __int128)s * 100u >= (unsigned __int128)d * x;
}
SYN_HD uint64_t as_lx(const uint64_t *ex, uint64_t n, uint32_t x, uint64_t d)
{
    if (!d || !n || !as_nx_reached(ex[n], x, d)) return 0;
    // ex[0] does not reach it (x D > 0), ex[n] does
    return first_where((uint64_t)1, n, [&](uint64_t j) { return as_nx_reached(ex[j], x, d); });
}

// ---- the union of subject intervals, chains in (s_record, s_start) order.  The running maximum of (s_record << 32 | s_end) over
// the chains in front of one IS the largest s_end of its own record so far whenever its upper half names that record: records only
// rise along the order, so the maximum "resets" at a record border by itself (0: nothing in front)
SYN_HD uint64_t as_cover_word(uint32_t s_record, uint32_t s_end) { return (uint64_t)s_record << 32 | s_end; }
SYN_HD uint64_t as_uncovered(uint64_t before, uint32_t s_record, uint32_t s_start, uint32_t s_end)
{
    uint32_t from = s_start;
    if (before && (uint32_t)(before >> 32) == s_record && (uint32_t)before > from) from = (uint32_t)before;
    return s_end > from ? (uint64_t)(s_end - from) : 0u;
}

// the sort keys: chains by subject place, lengths descending
SYN_HD uint64_t as_place_key(uint32_t s_record, uint32_t s_start) { return (uint64_t)s_record << 32 | s_start; }
SYN_HD uint64_t as_len_key(uint32_t len) { return (uint64_t)(0xFFFFFFFFu - len); }
SYN_HD uint32_t as_key_len(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

}  // namespace mxg
