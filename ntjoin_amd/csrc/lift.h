// lift.h -- features of the source records carried through a piece table onto the records it spells (mxg_lift_prepare,
// mxg_lift_intervals, mxg_lift_bed; include/ntjoin_mx.h row f15): the part of a feature in a piece, the status rule,
// the two bisections over the sorted index, the BED line rules and the strand flip.  lift.hip runs the functions below on the
// device, one thread per feature; host_io.cpp parses BED lines with them; tools/lift_check.cpp runs all of them serially on the
// host.  Compiles for host and device.
//
// The INDEX of a table is its sequence pieces sorted, stably, by (record << 32) | start -- equal keys keep the table's order -- as
//     key[i]   (record << 32) | start
//     ent[i]   start, end, the table record R of the piece (bit 31: the piece is REV), the bases of R in front of it
//     rmax[i]  the maximum of (record << 32) | end over [0, i]: records rise, so within a record the running maximum of `end`
// The pieces that meet [a, b) of record r lie in [lo, hi): hi = the first i with key[i] >= (r << 32) | b (every piece of r that
// starts below b), lo = the first i with rmax[i] > (r << 32) | a (no piece in front of it ends behind a); of those, the ones with
// end > a are the parts.  A bisection over the ends themselves would not do: a short piece behind a long one ends before it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "bisect.h"
#include "ntjoin_mx.h"

#if defined(__HIPCC__)
#define LFT_HD __host__ __device__ inline
#else
#define LFT_HD inline
#endif

namespace mxg {

constexpr uint64_t LFT_MAX = 0x7FFFFFFFull;  // 2^31 features, parts or source records or more: MXG_ELIMIT
constexpr uint32_t LFT_REV = 0x80000000u;
constexpr uint32_t LFT_NONE = 0xFFFFFFFFu;

struct LiftEntry {
    uint32_t start, end, trec, off;  // trec: the table record, | LFT_REV
};

struct LiftPart {
    uint32_t s_record, s_start, s_end, src_start, reverse;
};

LFT_HD uint64_t lift_key(uint32_t record, uint32_t pos) { return (uint64_t)record << 32 | pos; }

// is (r, a, b) a feature of the source records at all
LFT_HD bool lift_valid(uint32_t r, uint32_t a, uint32_t b, uint64_t n_source, const uint32_t *source_length)
{
    return r < n_source && a < b && b <= source_length[r];
}

// the first i in [0, m] with arr[i] >= k (strict = false) or arr[i] > k (strict = true); arr rises
LFT_HD uint32_t lift_bound(const uint64_t *arr, uint32_t m, uint64_t k, bool strict)
{
    return first_where(0u, m, [&](uint32_t i) { return strict ? arr[i] > k : arr[i] >= k; });
}

// the candidates [lo, hi) of feature (r, a, b); lo >= hi: none
LFT_HD void lift_range(const uint64_t *key, const uint64_t *rmax, uint32_t m, uint32_t r, uint32_t a, uint32_t b, uint32_t &lo, uint32_t &hi)
{
    hi = lift_bound(key, m, lift_key(r, b), false);
    lo = lift_bound(rmax, hi, lift_key(r, a), true);
}

// the part of [a, b) in piece e (they meet: e.start < b and e.end > a)
LFT_HD LiftPart lift_part(const LiftEntry &e, uint32_t a, uint32_t b)
{
    const uint32_t lo = a > e.start ? a : e.start, hi = b < e.end ? b : e.end;
    LiftPart p;
    p.s_record = e.trec & ~LFT_REV;
    p.src_start = lo;
    p.reverse = e.trec >> 31;
    if (p.reverse) {
        p.s_start = e.off + (e.end - hi);
        p.s_end = e.off + (e.end - lo);
    } else {
        p.s_start = e.off + (lo - e.start);
        p.s_end = e.off + (hi - e.start);
    }
    return p;
}

// n_parts parts that hold `lifted` of the b - a bases
LFT_HD uint32_t lift_status(uint64_t n_parts, uint64_t lifted, uint32_t a, uint32_t b)
{
    if (n_parts == 0) return MXG_LIFT_LOST;
    if (n_parts == 1 && lifted == (uint64_t)(b - a)) return MXG_LIFT_WHOLE;
    if (lifted < (uint64_t)(b - a)) return MXG_LIFT_PARTIAL;
    return MXG_LIFT_SPLIT;
}

// a feature's parts counted, and its status (a valid feature)
LFT_HD uint32_t lift_count(const LiftEntry *ent, uint32_t lo, uint32_t hi, uint32_t a, uint32_t b, uint64_t &n_parts)
{
    uint64_t c = 0, lifted = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        const LiftEntry e = ent[i];
        if (e.end <= a) continue;
        ++c;
        lifted += (uint64_t)((b < e.end ? b : e.end) - (a > e.start ? a : e.start));
    }
    n_parts = c;
    return lift_status(c, lifted, a, b);
}

LFT_HD const char *lift_reason(uint32_t status)
{
    switch (status) {
    case MXG_LIFT_SPLIT: return "Split in new";
    case MXG_LIFT_PARTIAL: return "Partially deleted in new";
    case MXG_LIFT_LOST: return "Deleted in new";
    case MXG_LIFT_INVALID: return "Invalid";
    case MXG_LIFT_UNKNOWN: return "Unknown record";
    default: return "";
    }
}

LFT_HD char lift_flip(char strand) { return strand == '+' ? '-' : strand == '-' ? '+' : strand; }

// ---- BED lines ---------------------------------------------------------------------------------------------------------------------
// A line is the bytes between two '\n' (the last one may lack its '\n'), less one '\r' at its end.
struct BedLine {
    bool ok;                        // columns 1 to 3 are there and columns 2 and 3 are numbers
    uint32_t name_len;              // column 1 is line[0, name_len)
    uint32_t a, b;                  // columns 2 and 3
    uint64_t rest_off, rest_len;    // column 4 to the line's end, from line[rest_off] on; rest_off = 0: fewer than four columns
    uint64_t strand_off;            // where column 6 lies when it is exactly "+" or "-"; 0: it is not
};

inline uint64_t bed_line_end(const char *line, uint64_t len) { return len && line[len - 1] == '\r' ? len - 1 : len; }

// empty lines and lines that begin with '#', "track" or "browser" hold no feature
inline bool bed_skipped(const char *line, uint64_t len)
{
    len = bed_line_end(line, len);
    if (len == 0 || line[0] == '#') return true;
    auto begins = [&](const char *w, uint64_t n) {
        for (uint64_t i = 0; i < n; ++i)
            if (i >= len || line[i] != w[i]) return false;
        return true;
    };
    return begins("track", 5) || begins("browser", 7);
}

// 1 to 10 decimal digits and nothing else, at most 2^32 - 1
inline bool bed_number(const char *s, uint64_t n, uint32_t &v)
{
    if (n < 1 || n > 10) return false;
    uint64_t x = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        x = x * 10u + (uint64_t)(s[i] - '0');
    }
    if (x > 0xFFFFFFFFull) return false;
    v = (uint32_t)x;
    return true;
}

inline BedLine bed_parse(const char *line, uint64_t len)
{
    len = bed_line_end(line, len);
    BedLine o{};
    uint64_t tab[6], n_tab = 0;  // the first five tabs, then the end of column 6
    for (uint64_t i = 0; i < len && n_tab < 6; ++i)
        if (line[i] == '\t') tab[n_tab++] = i;
    const uint64_t n_col = n_tab + 1;
    o.name_len = (uint32_t)(n_tab ? (tab[0] < 0xFFFFFFFFull ? tab[0] : 0xFFFFFFFFull) : 0);
    if (n_col >= 4) o.rest_off = tab[2] + 1, o.rest_len = len - o.rest_off;
    if (n_col >= 6) {
        const uint64_t c6 = tab[4] + 1, c6_end = n_tab >= 6 ? tab[5] : len;
        if (c6_end - c6 == 1 && (line[c6] == '+' || line[c6] == '-')) o.strand_off = c6;
    }
    if (n_col < 3) return o;
    const uint64_t c3_end = n_tab >= 3 ? tab[2] : len;
    o.ok = bed_number(line + tab[0] + 1, tab[1] - tab[0] - 1, o.a) && bed_number(line + tab[1] + 1, c3_end - tab[1] - 1, o.b);
    return o;
}

}  // namespace mxg
