// seqstat.h -- the assembly report (row f10; contract in include/ntjoin_mx.h; executable in
// tests/_seqreport_restatement.py): base classes, N runs, gaps and contigs of a stretch of FASTA text as a summary that combines
// associatively, and the contiguity block (N50 ...) of a list of lengths.  report.hip makes one summary per 16 bytes of a lane,
// folds a work item's 256 of them and scans the items; tools/seqstat_check.cpp runs the same code on the host.
//
// A byte of text is a base (one of six classes) or a byte that is passed over (a line end, a byte of a header); in front of some
// bytes a record begins (a border).  The STATE between two stretches of one record is {ctg, nrun}: the bases of the contig
// that is open, without the N run that is open at the end, and that run's length.  Whether a run is a gap is decided where the
// run ENDS (a base that is no N, or a border), from all of its length: two runs of min_gap / 2 on either side of a cut are one gap.
// That is why a stretch's summary (SeqPart) keeps its first and its last N run apart from what lies between: only runs with both
// ends inside are decided inside.  A border closes the run and the contig and forgets the state.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SQ_HD __host__ __device__ inline
#else
#define SQ_HD inline
#endif

namespace mxg {

enum : uint32_t { SQ_A = 0, SQ_C = 1, SQ_G = 2, SQ_T = 3, SQ_N = 4, SQ_OTHER = 5, SQ_LOWER = 6, SQ_COUNTS = 7, SQ_SKIP = 7 };

// the class of a byte of sequence text: byte_class (text_index.h) with N apart from the other invalid bases; U counts as T there too
SQ_HD uint32_t seq_class(uint32_t b)
{
    if (b == (uint32_t)'\n' || b == (uint32_t)'\r') return SQ_SKIP;
    const uint32_t u = b & 0xDFu;
    return u == 'A' ? SQ_A : u == 'C' ? SQ_C : u == 'G' ? SQ_G : (u == 'T' || u == 'U') ? SQ_T : u == 'N' ? SQ_N : SQ_OTHER;
}

struct SeqState {
    uint64_t ctg = 0;   // bases of the open contig in front of the open N run
    uint64_t nrun = 0;  // the N run that is open at the end
    uint32_t open = 0;  // a record is open
};

// bases of one record: [head_n N] mid_first [gap ... gap mid_last] [tail_n N]; all_n: nothing but the head_n N (or nothing at all)
struct SeqPart {
    uint64_t head_n = 0, tail_n = 0;
    uint64_t mid_first = 0;  // bases from behind the first run to the first gap inside (to the last run, without one)
    uint64_t mid_last = 0;   // has_gap: bases from behind the last gap inside to the last run
    uint32_t all_n = 1, has_gap = 0;
};

// the summary of a stretch: what lies behind its last border, and whether it has one
struct SeqSum {
    SeqPart p;
    uint32_t reset = 0;
};

SQ_HD SeqPart seq_part_n(uint64_t c)
{
    SeqPart p;
    p.head_n = c;
    return p;
}
SQ_HD SeqPart seq_part_b(uint64_t c)
{
    SeqPart p;
    if (c) p.all_n = 0, p.mid_first = c;
    return p;
}

// A followed directly by B inside one record
SQ_HD SeqPart seq_cat(const SeqPart &A, const SeqPart &B, uint64_t min_gap)
{
    if (B.all_n) {
        SeqPart r = A;
        if (A.all_n) r.head_n += B.head_n; else r.tail_n += B.head_n;
        return r;
    }
    if (A.all_n) {
        SeqPart r = B;
        r.head_n += A.head_n;
        return r;
    }
    SeqPart r;
    r.all_n = 0, r.head_n = A.head_n, r.tail_n = B.tail_n;
    const uint64_t J = A.tail_n + B.head_n;  // the run between them: both of its ends are known now
    if (J >= min_gap) {
        r.has_gap = 1, r.mid_first = A.mid_first, r.mid_last = B.has_gap ? B.mid_last : B.mid_first;
        return r;
    }
    r.has_gap = A.has_gap | B.has_gap;
    if (!A.has_gap) r.mid_first = A.mid_first + J + B.mid_first;
    else r.mid_first = A.mid_first;
    if (B.has_gap) r.mid_last = B.mid_last;
    else if (A.has_gap) r.mid_last = A.mid_last + J + B.mid_first;
    return r;
}

// the operator of the scan: a stretch with a border forgets what is in front of it
SQ_HD SeqSum seq_combine(const SeqSum &A, const SeqSum &B, uint64_t min_gap)
{
    if (B.reset) return B;
    SeqSum r;
    r.reset = A.reset;
    r.p = seq_cat(A.p, B.p, min_gap);
    return r;
}

// a state as the part that leaves it, and the state a part leaves behind a border
SQ_HD SeqPart seq_part_of(const SeqState &s)
{
    return seq_cat(seq_part_b(s.ctg), seq_part_n(s.nrun), 1);
}
SQ_HD SeqState seq_state_of(const SeqPart &p, uint64_t min_gap, uint32_t open)
{
    SeqState s;
    s.open = open;
    if (p.all_n) s.nrun = p.head_n;
    else s.nrun = p.tail_n, s.ctg = p.has_gap ? p.mid_last : p.head_n >= min_gap ? p.mid_first : p.head_n + p.mid_first;
    return s;
}
// the state behind a stretch with the summary B that is entered with the state s
SQ_HD SeqState seq_apply(const SeqState &s, const SeqSum &B, uint64_t min_gap)
{
    if (B.reset) return seq_state_of(B.p, min_gap, 1);
    return seq_state_of(seq_cat(seq_part_of(s), B.p, min_gap), min_gap, s.open);
}

// ---- the walk: Sink has gap(uint64_t) and contig(uint64_t) ----
// c bases that are N / that are not
SQ_HD void seq_step_n(SeqState &s, uint64_t c)
{
    s.nrun += c;
}
template <class Sink> SQ_HD void seq_end_run(SeqState &s, uint64_t min_gap, Sink &o)
{
    if (s.nrun >= min_gap) {
        o.gap(s.nrun);
        if (s.ctg) o.contig(s.ctg);
        s.ctg = 0;
    } else {
        s.ctg += s.nrun;
    }
    s.nrun = 0;
}
template <class Sink> SQ_HD void seq_step_b(SeqState &s, uint64_t c, uint64_t min_gap, Sink &o)
{
    if (!c) return;
    if (s.nrun) seq_end_run(s, min_gap, o);
    s.ctg += c;
}
// a border: the record that is open ends
template <class Sink> SQ_HD void seq_close(SeqState &s, uint64_t min_gap, Sink &o)
{
    if (s.nrun) seq_end_run(s, min_gap, o);
    if (s.ctg) o.contig(s.ctg);
    s.ctg = 0;
}

// 16 bytes of text as three masks: bit j of n / b = byte j is an N / another base, bit j of r = a record begins in front of byte j.
// Walks the runs of one class, not the bytes: bytes that are passed over (in neither n nor b) interrupt nothing.
template <class Sink> SQ_HD void seq_walk_masks(SeqState &s, uint32_t n, uint32_t b, uint32_t r, uint64_t min_gap, Sink &o)
{
    uint32_t at = 0;  // bits below are done
    for (;;) {
        const uint32_t rest = ~((1u << at) - 1u);
        const uint32_t rr = r & rest;
        const uint32_t stop = rr ? (uint32_t)__builtin_ctz(rr) : 16u;  // the next border
        const uint32_t seg = ((1u << stop) - 1u) & rest;
        uint32_t x = (n | b) & seg;
        while (x) {
            const uint32_t i = (uint32_t)__builtin_ctz(x);
            const bool is_n = (n >> i) & 1u;
            const uint32_t other = (is_n ? b : n) & x;
            const uint32_t j = other ? (uint32_t)__builtin_ctz(other) : 16u;
            const uint32_t run = x & ((1u << j) - 1u);
            const uint32_t c = (uint32_t)__builtin_popcount(run);
            if (is_n) seq_step_n(s, c); else seq_step_b(s, c, min_gap, o);
            x &= ~run;
        }
        if (stop >= 16u) return;
        seq_close(s, min_gap, o);
        s.open = 1;
        r &= ~(1u << stop);
        at = stop;
    }
}

struct SeqNoSink {
    SQ_HD void gap(uint64_t) {}
    SQ_HD void contig(uint64_t) {}
};

// the summary of the same 16 bytes
SQ_HD SeqSum seq_sum_masks(uint32_t n, uint32_t b, uint32_t r, uint64_t min_gap)
{
    SeqSum s;
    if (r) {
        const uint32_t last = 31u - (uint32_t)__builtin_clz(r);
        const uint32_t keep = ~((1u << last) - 1u);
        n &= keep, b &= keep;
        s.reset = 1;
    }
    uint32_t x = n | b;
    if (x && !n) {  // (the common case)
        s.p = seq_part_b((uint32_t)__builtin_popcount(x));
        return s;
    }
    while (x) {
        const uint32_t i = (uint32_t)__builtin_ctz(x);
        const bool is_n = (n >> i) & 1u;
        const uint32_t other = (is_n ? b : n) & x;
        const uint32_t j = other ? (uint32_t)__builtin_ctz(other) : 16u;
        const uint32_t run = x & ((1u << j) - 1u);
        const uint32_t c = (uint32_t)__builtin_popcount(run);
        s.p = seq_cat(s.p, is_n ? seq_part_n(c) : seq_part_b(c), min_gap);
        x &= ~run;
    }
    return s;
}

// ---- 16 bytes as four words: the classes by bit operations on whole words ----
// 0x80 in every byte of w that equals c
SQ_HD uint32_t sq_eq(uint32_t w, uint32_t c)
{
    const uint32_t x = w ^ (c * 0x01010101u);
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
// the four 0x80 bits of m as bits 0 .. 3
SQ_HD uint32_t sq_nib(uint32_t m)
{
    return (((m >> 7) * 0x01020408u) >> 24) & 15u;
}

struct SeqLane {
    uint32_t n = 0, b = 0;     // masks over the 16 bytes (valid ones only)
    uint32_t cnt[SQ_COUNTS] = {0, 0, 0, 0, 0, 0, 0};
};

// w: the 16 bytes; valid: bit j = byte j is sequence text of the stretch (line ends among them are told here)
SQ_HD SeqLane seq_lane(const uint32_t w[4], uint32_t valid)
{
    SeqLane L;
    uint32_t m[SQ_COUNTS] = {0, 0, 0, 0, 0, 0, 0}, base = 0;
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t v = w[q], f = v | 0x20202020u;
        const uint32_t skip = sq_eq(v, '\n') | sq_eq(v, '\r');
        const uint32_t a = sq_eq(f, 'a'), c = sq_eq(f, 'c'), g = sq_eq(f, 'g'), t = sq_eq(f, 't') | sq_eq(f, 'u'), n = sq_eq(f, 'n');
        const uint32_t l7 = v & 0x7F7F7F7Fu;  // 'a' .. 'z': at least 0x61, below 0x7B, bit 7 clear
        const uint32_t low = (l7 + 0x1F1F1F1Fu) & ~(l7 + 0x05050505u) & ~v & 0x80808080u;
        m[SQ_A] |= sq_nib(a) << (4u * q), m[SQ_C] |= sq_nib(c) << (4u * q), m[SQ_G] |= sq_nib(g) << (4u * q);
        m[SQ_T] |= sq_nib(t) << (4u * q), m[SQ_N] |= sq_nib(n) << (4u * q), m[SQ_LOWER] |= sq_nib(low) << (4u * q);
        base |= sq_nib(~skip & 0x80808080u) << (4u * q);
    }
    base &= valid;
    uint32_t known = 0;
    for (uint32_t c = SQ_A; c <= SQ_N; ++c) {
        L.cnt[c] = (uint32_t)__builtin_popcount(m[c] & base);
        known |= m[c];
    }
    L.cnt[SQ_OTHER] = (uint32_t)__builtin_popcount(base & ~known);
    L.cnt[SQ_LOWER] = (uint32_t)__builtin_popcount(m[SQ_LOWER] & base);
    L.n = m[SQ_N] & base;
    L.b = base & ~m[SQ_N];
    return L;
}

// ---- the serial walk: what the kernels must agree with ----
struct SeqCounts {
    uint64_t cnt[SQ_COUNTS] = {0, 0, 0, 0, 0, 0, 0};
    uint64_t bases = 0, records = 0;
};

// text[lo, hi) entered with the state s.  kind (may be null: all text): per byte 0 = sequence text, 1 = passed over (a header's byte),
// 2 = passed over and a record begins here (a header's '>').
template <class Sink>
SQ_HD void seq_walk(const unsigned char *text, const unsigned char *kind, uint64_t lo, uint64_t hi, SeqState &s, uint64_t min_gap, SeqCounts &k,
                    Sink &o)
{
    for (uint64_t a = lo; a < hi; ++a) {
        const uint32_t kd = kind ? kind[a] : 0u;
        if (kd == 2u) {
            seq_close(s, min_gap, o);
            s.open = 1;
            ++k.records;
        }
        if (kd) continue;
        const uint32_t b = text[a], c = seq_class(b);
        if (c == SQ_SKIP) continue;
        ++k.cnt[c], ++k.bases;
        if (b >= 'a' && b <= 'z') ++k.cnt[SQ_LOWER];
        if (c == SQ_N) seq_step_n(s, 1); else seq_step_b(s, 1, min_gap, o);
    }
}

// ---- the contiguity block ----
struct SeqContig {
    uint64_t n = 0, n_min = 0, sum = 0, min = 0, max = 0;
    uint64_t nx[3] = {0, 0, 0}, lx[3] = {0, 0, 0};  // x = 50, 75, 90
};

// len[0, n) is sorted in place, descending
inline SeqContig seq_contiguity(uint64_t *len, uint64_t n, uint64_t min_len)
{
    SeqContig c;
    c.n = n;
    // (insertion is not for lists of this size: a plain heap sort, no library needed on either side)
    auto sift = [&](uint64_t root, uint64_t end) {
        for (;;) {
            uint64_t ch = 2 * root + 1;
            if (ch >= end) return;
            if (ch + 1 < end && len[ch + 1] < len[ch]) ++ch;
            if (len[root] <= len[ch]) return;
            const uint64_t t = len[root];
            len[root] = len[ch], len[ch] = t, root = ch;
        }
    };
    for (uint64_t i = n / 2; i-- > 0;) sift(i, n);
    for (uint64_t e = n; e > 1; --e) {
        const uint64_t t = len[0];
        len[0] = len[e - 1], len[e - 1] = t;
        sift(0, e - 1);
    }
    uint64_t m = 0;
    while (m < n && len[m] >= min_len) ++m;
    c.n_min = m;
    if (!m) return c;
    for (uint64_t j = 0; j < m; ++j) c.sum += len[j];
    c.max = len[0], c.min = len[m - 1];
    const uint32_t xs[3] = {50, 75, 90};
    for (uint32_t u = 0; u < 3; ++u) {
        // 100 S_j >= x sum without leaving 64 bits: S_j >= ceil(x sum / 100), the product split at sum / 100
        const uint64_t q = c.sum / 100, r = c.sum % 100;
        const uint64_t need = xs[u] * q + (xs[u] * r + 99) / 100;
        uint64_t S = 0;
        for (uint64_t j = 0; j < m; ++j) {
            S += len[j];
            if (S >= need) {
                c.lx[u] = j + 1, c.nx[u] = len[j];
                break;
            }
        }
    }
    return c;
}

}  // namespace mxg
