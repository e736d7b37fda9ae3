// compose.h -- piece tables and their composition (mxg_compose_pieces): what one record of a scaffold file is made
// of, in terms of the records of the file it was cut from, and the same after two rounds of scaffolding in terms of the first
// round's input.  compose.hip runs the functions below on the device, one thread per piece; tools/compose_check.cpp runs them
// serially on the host.  Compiles for host and device.
//
// A piece table spells n records: record r is the concatenation of pieces[first[r] .. first[r + 1]).  A piece is
//     FWD  bases [start, end) of `record`                        REV  the same, reverse-complemented
//     GAP  end - start Ns (record = start = 0)
// A VALID table has at least one piece per record, start < end in every piece, and no record longer than 2^32 - 1 bases; its
// PREFIX pre[j] is the number of bases of its record in front of piece j (0 at the record's first piece).
// Composition: `outer` names records of `inner`.  An outer FWD / REV piece over [a, b) of inner record r becomes the inner pieces of
// r that meet [a, b) -- pieces j_lo .. j_hi, found by bisection over r's prefix -- each clipped to [a, b); under REV in reverse
// order with FWD and REV swapped.  An outer GAP stays.  Neighbouring GAPs of one record are then joined (compose.hip's second half).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "bisect.h"
#include "ntjoin_mx.h"

#if defined(__HIPCC__)
#define CMP_HD __host__ __device__ inline
#else
#define CMP_HD inline
#endif

namespace mxg {

constexpr uint64_t CMP_MAX_PIECES = 0x7FFFFFFFull;  // a table of 2^31 pieces or more is MXG_ELIMIT

CMP_HD uint32_t cmp_len(const mxg_seq_piece &p) { return p.end - p.start; }

// the inner pieces [j_lo, j_hi] of a record that meet [a, b), a < b <= the record's length.  The piece of a record that holds
// base a: the largest j < m with pre[j] <= a   (pre[0] = 0, pre increasing, m >= 1)
CMP_HD void cmp_range(const uint32_t *pre, uint32_t m, uint32_t a, uint32_t b, uint32_t &j_lo, uint32_t &j_hi)
{
    j_lo = last_le(pre, 0u, m, a);
    j_hi = last_le(pre, 0u, m, b - 1u);
}

// inner piece q, which starts at base `at` of its record, clipped to [a, b) of that record (they meet), as a piece of the outer
// record; rev: the outer piece is REV.  With [lo, hi) = the part of q's own spelling that is kept:
//   q GAP: hi - lo Ns.   q FWD: [start + lo, start + hi).   q REV: its spelling runs from `end` down: [end - hi, end - lo).
CMP_HD mxg_seq_piece cmp_clip(const mxg_seq_piece &q, uint32_t at, uint32_t a, uint32_t b, bool rev)
{
    const uint32_t n = cmp_len(q);
    const uint32_t lo = a > at ? a - at : 0u;
    const uint32_t hi = b - at < n ? b - at : n;
    mxg_seq_piece o;
    if (q.kind == MXG_PIECE_GAP) {
        o.record = 0;
        o.start = 0;
        o.end = hi - lo;
        o.kind = MXG_PIECE_GAP;
        return o;
    }
    o.record = q.record;
    if (q.kind == MXG_PIECE_FWD) {
        o.start = q.start + lo;
        o.end = q.start + hi;
    } else {
        o.start = q.end - hi;
        o.end = q.end - lo;
    }
    o.kind = (q.kind == MXG_PIECE_REV) != rev ? MXG_PIECE_REV : MXG_PIECE_FWD;
    return o;
}

// the t-th piece (in the outer record's order) of what outer piece p becomes; [j_lo, j_hi] from cmp_range
CMP_HD mxg_seq_piece cmp_expand(const mxg_seq_piece &p, const mxg_seq_piece *ip, const uint32_t *pre, uint32_t j_lo, uint32_t j_hi, uint32_t t)
{
    const bool rev = p.kind == MXG_PIECE_REV;
    const uint32_t j = rev ? j_hi - t : j_lo + t;
    return cmp_clip(ip[j], pre[j], p.start, p.end, rev);
}

// a piece table as the device code takes it: checked, with 32-bit offsets, the prefix, every record's length and every piece's record
struct CmpTable {
    std::vector<uint32_t> first, pre, len, rec;
};

// Checks pieces[0, first[n_records]) as a valid table and fills t.  n_ref: the number of records its FWD / REV pieces may name
// (~0: not known); ref_len: their lengths, or null.  Returns MXG_OK, or MXG_EINVAL / MXG_ELIMIT with the reason in msg.
inline int cmp_table(const char *what, const mxg_seq_piece *pieces, const uint64_t *first, uint64_t n_records, uint64_t n_ref, const uint32_t *ref_len,
                     CmpTable &t, std::string &msg)
{
    char buf[256];
    if (first[0] != 0) {
        msg = std::string(what) + "_first does not start at 0";
        return MXG_EINVAL;
    }
    for (uint64_t r = 0; r < n_records; ++r)
        if (first[r + 1] <= first[r]) {
            snprintf(buf, sizeof buf, "%s record %llu has no pieces", what, (unsigned long long)r);
            msg = buf;
            return MXG_EINVAL;
        }
    const uint64_t n = first[n_records];
    if (n >= CMP_MAX_PIECES || n_records >= CMP_MAX_PIECES) {
        snprintf(buf, sizeof buf, "%s: %llu pieces in %llu records (at most 2^31 - 2)", what, (unsigned long long)n, (unsigned long long)n_records);
        msg = buf;
        return MXG_ELIMIT;
    }
    t.first.resize(n_records + 1);
    t.len.resize(n_records);
    t.pre.resize(n);
    t.rec.resize(n);
    for (uint64_t r = 0; r < n_records; ++r) {
        t.first[r] = (uint32_t)first[r];
        uint64_t at = 0;
        for (uint64_t j = first[r]; j < first[r + 1]; ++j) {
            const mxg_seq_piece &p = pieces[j];
            const char *bad = nullptr;
            if (p.kind > MXG_PIECE_GAP) bad = "has an unknown kind";
            else if (p.start >= p.end) bad = "is empty or inverted";
            else if (p.kind != MXG_PIECE_GAP && p.record >= n_ref) bad = "names a record that does not exist";
            else if (p.kind != MXG_PIECE_GAP && ref_len && p.end > ref_len[p.record]) bad = "is not inside its inner record";
            if (bad) {
                snprintf(buf, sizeof buf, "%s record %llu piece %llu {%u, %u, %u, %u} %s", what, (unsigned long long)r,
                         (unsigned long long)(j - first[r]), p.record, p.start, p.end, p.kind, bad);
                msg = buf;
                return MXG_EINVAL;
            }
            t.pre[j] = (uint32_t)at;
            t.rec[j] = (uint32_t)r;
            at += cmp_len(p);
            if (at > 0xFFFFFFFFull) {
                snprintf(buf, sizeof buf, "%s record %llu is longer than 2^32 - 1 bases", what, (unsigned long long)r);
                msg = buf;
                return MXG_ELIMIT;
            }
        }
        t.len[r] = (uint32_t)at;
    }
    t.first[n_records] = (uint32_t)n;
    return MXG_OK;
}

}  // namespace mxg
