// fai_scan.h -- the line structure of a FASTA record as `samtools faidx` wants it (reference ntJoin:152-153, 207-208), as a summary
// of a byte range that combines associatively: fai.hip makes one summary per 16 bytes of a lane, folds a work item's 256 of them, and
// scans the items of all records; tools/fai_check.cpp runs the same code over a file on the host.  Compiles for host and device.
//
// A record's sequence text T is split at '\n' into lines.  A line is bases (0x21 .. 0x7E), an optional '\r', and its '\n' (the last
// line of the file may lack it); its SHAPE is bases << 2 | kind, kind 0 = no line end, 1 = "\n", 2 = "\r\n".  An accepted record is
//     X ... X [Y] [empty ...]        X = the first line's shape; Y: fewer bases (at least one), the same kind -- or no line end at
// the end of the text, then as many bases as X at the most; empty lines behind the last record of the file only.  The complete lines
// of a range that does not start a record have the same form with any part missing, which is what FaiForm holds; the bytes in front of
// a range's first '\n' and behind its last belong to lines that neighbours complete.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FAI_HD __host__ __device__ inline
#else
#define FAI_HD inline
#endif

namespace mxg {

constexpr uint64_t FAI_NONE = ~0ull;
constexpr uint64_t FAI_INTERNAL = ~0ull - 1;  // FaiRow::err_at: the bases counted here are not the record's length
enum : uint32_t { FAI_BASE = 0, FAI_CR = 1, FAI_NL = 2, FAI_NL_CR = 3, FAI_BAD = 4 };

// the byte b between prev and next (next = 0 behind the text's last byte): a '\r' is legal directly in front of a '\n' only
FAI_HD uint32_t fai_byte_class(uint32_t prev, uint32_t b, uint32_t next)
{
    if (b >= 0x21u && b <= 0x7Eu) return FAI_BASE;
    if (b == (uint32_t)'\n') return prev == (uint32_t)'\r' ? FAI_NL_CR : FAI_NL;
    if (b == (uint32_t)'\r' && next == (uint32_t)'\n') return FAI_CR;
    return FAI_BAD;
}

struct FaiForm {  // complete lines in file order: k of shape x, then one of shape y (FAI_NONE: none), then e empty ones
    uint64_t x = 0, k = 0, x_at = 0;  // (*_at: where the first such line starts in the text)
    uint64_t y = FAI_NONE, y_at = 0;
    uint64_t e = 0, e_at = 0;
};

struct FaiSum {
    uint64_t len = 0, bases = 0, nl = 0;     // bytes, bases, '\n' of the range
    uint64_t head = 0;                       // nl > 0: bases in front of the first '\n' << 2 | that line end's kind
    uint64_t tail_b = 0;                     // bases behind the last '\n' (all of them for nl = 0)
    uint64_t first_nl = 0, last_nl = 0;      // nl > 0: text offsets
    FaiForm in;                              // the lines behind the first '\n' that end inside the range
    uint64_t err_at = FAI_NONE;              // where the first offending line starts ...
    uint32_t err_pending = 0;                // ... or: it starts in front of the range
    uint32_t seg = 0;                        // the scan over work items: the range begins a record
};

FAI_HD void fai_note(uint64_t &err, uint64_t at)
{
    if (at < err) err = at;
}

FAI_HD FaiForm fai_form_line(uint64_t shape, uint64_t at)
{
    FaiForm f;
    if (shape >> 2) f.x = shape, f.k = 1, f.x_at = at;
    else f.e = 1, f.e_at = at;
    return f;
}

// may a line of shape `last` be the last non-empty one of a record whose first line has shape `first`?
FAI_HD bool fai_may_end(uint64_t first, uint64_t last)
{
    const uint64_t bf = first >> 2, bl = last >> 2, kf = first & 3u, kl = last & 3u;
    return bl >= 1 && ((kl == kf && bl < bf) || (kl == 0 && bl <= bf));
}

// F followed by G; what cannot be part of an accepted record is noted in err
FAI_HD void fai_form_cat(FaiForm &F, const FaiForm &G, uint64_t &err)
{
    if (!G.k && !G.e) return;
    if (!F.k && !F.e) {
        F = G;
        return;
    }
    if (!G.k) {  // empty lines only
        if (!F.e) F.e_at = G.e_at;
        F.e += G.e;
        return;
    }
    if (F.e) fai_note(err, F.e_at);                    // an empty line in front of a line with bases
    else if (F.y != FAI_NONE) fai_note(err, F.y_at);   // a line unlike the first that is not the last one
    if (!F.k) {
        F = G;
        return;
    }
    if (G.x == F.x) {
        F.k += G.k;
        F.y = G.y, F.y_at = G.y_at;
    } else if (G.k == 1 && G.y == FAI_NONE && fai_may_end(F.x, G.x)) {
        F.y = G.x, F.y_at = G.x_at;
    } else {
        fai_note(err, G.x_at);
    }
    F.e = G.e, F.e_at = G.e_at;
}

// the summary of one byte at text offset `at`
FAI_HD FaiSum fai_byte(uint32_t cls, uint64_t at)
{
    FaiSum s;
    s.len = 1;
    if (cls == FAI_BASE) s.bases = s.tail_b = 1;
    else if (cls == FAI_BAD) s.err_pending = 1;
    else if (cls != FAI_CR) s.nl = 1, s.head = cls == FAI_NL_CR ? 2u : 1u, s.first_nl = s.last_nl = at;
    return s;
}

// n bases and nothing else
FAI_HD FaiSum fai_bases(uint64_t n)
{
    FaiSum s;
    s.len = s.bases = s.tail_b = n;
    return s;
}

// A followed directly by B, both inside one record
FAI_HD FaiSum fai_combine(const FaiSum &A, const FaiSum &B)
{
    if (!B.len) return A;
    if (!A.len) {
        FaiSum r = B;
        r.seg |= A.seg;
        return r;
    }
    FaiSum r;
    r.len = A.len + B.len, r.bases = A.bases + B.bases, r.nl = A.nl + B.nl;
    r.seg = A.seg | B.seg;
    uint64_t err = FAI_NONE;
    bool pending = false;
    if (!B.nl) {
        r.head = A.head, r.first_nl = A.first_nl, r.last_nl = A.last_nl, r.in = A.in;
        r.tail_b = A.tail_b + B.tail_b;
        if (B.err_pending) {
            if (A.nl) fai_note(err, A.last_nl + 1);
            else pending = true;
        }
    } else {
        const uint64_t joined = (A.tail_b + (B.head >> 2)) << 2 | (B.head & 3u);  // the line A's last bytes begin and B's first '\n' ends
        if (!A.nl) {
            r.head = joined, r.first_nl = B.first_nl, r.in = B.in;
            pending = B.err_pending != 0;
        } else {
            r.head = A.head, r.first_nl = A.first_nl, r.in = A.in;
            fai_form_cat(r.in, fai_form_line(joined, A.last_nl + 1), err);
            fai_form_cat(r.in, B.in, err);
            if (B.err_pending) fai_note(err, A.last_nl + 1);
        }
        r.last_nl = B.last_nl, r.tail_b = B.tail_b;
    }
    fai_note(err, B.err_at);
    if (A.err_pending || A.err_at != FAI_NONE) r.err_pending = A.err_pending, r.err_at = A.err_at;  // (the first offence stays)
    else r.err_pending = pending ? 1u : 0u, r.err_at = pending ? FAI_NONE : err;
    return r;
}

// the operator of the scan over the work items of all records: a range that begins a record forgets what is in front of it
FAI_HD FaiSum fai_seg_combine(const FaiSum &A, const FaiSum &B)
{
    if (B.seg) return B;
    return fai_combine(A, B);
}

struct FaiRow {  // one line of the .fai
    uint64_t length = 0, offset = 0, linebases = 0, linewidth = 0;
    uint64_t err_at = FAI_NONE;  // refused: where the first offending line starts (FAI_INTERNAL: see above)
};

// the row of a record whose text [t_lo, t_lo + s.len) has the summary s
FAI_HD FaiRow fai_finish(const FaiSum &s, uint64_t t_lo, bool last_record)
{
    FaiRow row;
    row.offset = t_lo;
    row.length = s.bases;
    if (!s.len) return row;
    uint64_t err = s.err_pending ? t_lo : s.err_at;
    if (!s.nl) {
        row.linebases = s.bases, row.linewidth = s.len;
    } else {
        row.linebases = s.head >> 2, row.linewidth = (s.head >> 2) + (s.head & 3u);
        FaiForm f = fai_form_line(s.head, t_lo);
        fai_form_cat(f, s.in, err);
        if (t_lo + s.len > s.last_nl + 1 && s.tail_b) fai_form_cat(f, fai_form_line(s.tail_b << 2, s.last_nl + 1), err);
        if (f.e && !last_record) fai_note(err, f.e_at);
    }
    row.err_at = err;
    return row;
}

// the summary of text[lo, lo + len) read byte by byte; text_bytes: where the text ends
FAI_HD FaiSum fai_scan_bytes(const unsigned char *text, uint64_t lo, uint64_t len, uint64_t text_bytes)
{
    FaiSum s;
    for (uint64_t a = lo; a < lo + len; ++a) {
        const uint32_t prev = a ? text[a - 1] : (uint32_t)'\n', next = a + 1 < text_bytes ? text[a + 1] : 0u;
        s = fai_combine(s, fai_byte(fai_byte_class(prev, text[a], next), a));
    }
    return s;
}

}  // namespace mxg
