// fai_check.cpp -- the .fai of a FASTA file by the code of the device route run on the host (ntjoin_amd/csrc/fai_scan.h): the file cut
// into work items of one 4096-byte tile at the most at record borders as load_fasta_device cuts it, every item's summary folded in
// order from its lanes' 16 bytes, the items of all records scanned in tiles of 256 with the segmented operator; the tiles' totals
// turned into what precedes every tile as k_fai_tile_scan does it: rounds of 256 tiles, the steps of fai_block_inclusive over a round,
// `excl` written from `carry` and the value of the thread in front, then `carry` folded with the round's total.
//   fai_check FASTA          the index on stdout; or, refused: exit status 3 and "refused RECORD ID OFFSET" on stdout
//   fai_check FASTA FAULT    the same with ONE fault switched on in the scan of the items (what a test input has to be able to show):
//       nocarry        the round carry ignored when excl is written        nocarry_t0 / nocarry_rest   by thread 0 / by the others only
//       early          the carry folded before excl is written: a round sees its own total
//       plain          carry and round combined with the plain operator instead of the segmented one
//       restart        the carry restarted from the round's total instead of folded onto the one before
//       inclusive      excl written from the thread's own value instead of the one in front of it
//       rounds         whole rounds only: a last round of fewer than 256 tiles is not run
//       rows_plain     a tile's rows take what precedes the tile with the plain operator: a record that begins a tile does not forget
// A stand-alone host program (c++ -std=c++17 -I ntjoin_amd/csrc tools/fai_check.cpp); tests/test_fai_cpu.py builds it plainly and
// with AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "fai_scan.h"

using namespace mxg;

namespace {
constexpr uint64_t TILE = 4096;
enum { F_NONE, F_NOCARRY, F_NOCARRY_T0, F_NOCARRY_REST, F_EARLY, F_PLAIN, F_RESTART, F_INCLUSIVE, F_ROUNDS, F_ROWS_PLAIN, F_COUNT };
const char *const FAULTS[F_COUNT] = {"", "nocarry", "nocarry_t0", "nocarry_rest", "early", "plain", "restart", "inclusive", "rounds", "rows_plain"};
struct Item {
    uint64_t lo;
    uint32_t len, rec;
};
struct Rec {
    std::string id;
    uint64_t text_off;
};

// as the 256 lanes of k_fai_items: 16 aligned bytes each, then the fold in thread order
FaiSum item_summary(const std::vector<unsigned char> &text, const Item &it)
{
    const uint64_t tile = it.lo & ~(TILE - 1);
    FaiSum lanes[256];
    bool plain = true;
    for (uint32_t t = 0; t < 256; ++t) {
        const uint64_t a0 = tile + 16u * t, lo = a0 > it.lo ? a0 : it.lo, hi = a0 + 16 < it.lo + it.len ? a0 + 16 : it.lo + it.len;
        if (lo >= hi) continue;
        uint64_t n_base = 0;
        for (uint64_t a = lo; a < hi; ++a) n_base += text[a] >= 0x21u && text[a] <= 0x7Eu;
        if (n_base == hi - lo) {  // (nothing but bases: no combine, as in the kernel)
            lanes[t] = fai_bases(n_base);
            continue;
        }
        lanes[t] = fai_scan_bytes(text.data(), lo, hi - lo, text.size());
        plain = false;
    }
    if (plain) return fai_bases(it.len);
    for (uint32_t o = 1; o < 256; o <<= 1)  // (the steps of fai_block_inclusive, from the top down so that one array serves)
        for (uint32_t t = 255; t >= o; --t) lanes[t] = fai_seg_combine(lanes[t - o], lanes[t]);
    return lanes[255];
}
}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2 && argc != 3) return 2;
    int fault = F_NONE;
    if (argc == 3) {
        for (int f = 1; f < F_COUNT; ++f)
            if (!strcmp(argv[2], FAULTS[f])) fault = f;
        if (fault == F_NONE) return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> text;
    unsigned char buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.insert(text.end(), buf, buf + n);
    fclose(f);
    const uint64_t tsz = text.size();
    // ---- header lines: '>' at the start of a line; the items of every record's text
    std::vector<Rec> recs;
    std::vector<Item> items;
    std::vector<uint64_t> item0;
    std::vector<uint64_t> hdr_at, hdr_end;
    for (uint64_t p = 0; p < tsz;) {
        if (text[p] == '>' && (p == 0 || text[p - 1] == '\n')) {
            const void *nl = memchr(text.data() + p, '\n', tsz - p);
            const uint64_t end = nl ? (uint64_t)(static_cast<const unsigned char *>(nl) - text.data()) : tsz;
            hdr_at.push_back(p), hdr_end.push_back(end);
            p = end + 1;
        } else {
            ++p;
        }
    }
    for (size_t r = 0; r < hdr_at.size(); ++r) {
        const uint64_t sb0 = hdr_end[r] + 1 < tsz ? hdr_end[r] + 1 : tsz, se = r + 1 < hdr_at.size() ? hdr_at[r + 1] : tsz;
        uint64_t e = hdr_at[r] + 1;
        while (e < hdr_end[r] && text[e] != ' ' && text[e] != '\t' && text[e] != '\r' && text[e] != '\n') ++e;
        recs.push_back(Rec{std::string(text.begin() + hdr_at[r] + 1, text.begin() + e), sb0});
        item0.push_back(items.size());
        for (uint64_t p = sb0; p < se;) {
            const uint64_t tile_end = (p / TILE + 1) * TILE, e2 = se < tile_end ? se : tile_end;
            items.push_back(Item{p, (uint32_t)(e2 - p), (uint32_t)r});
            p = e2;
        }
    }
    item0.push_back(items.size());
    // ---- the items' summaries; tiles of 256 items; what precedes every tile; the rows
    const size_t n_items = items.size(), n_tiles = (n_items + 255) / 256;
    std::vector<FaiSum> sums(n_items), agg(n_tiles), excl(n_tiles);
    for (size_t i = 0; i < n_items; ++i) {
        sums[i] = item_summary(text, items[i]);
        sums[i].seg = i == item0[items[i].rec] ? 1u : 0u;
    }
    for (size_t t = 0; t < n_tiles; ++t)
        for (size_t i = t * 256; i < n_items && i < (t + 1) * 256; ++i) agg[t] = fai_seg_combine(agg[t], sums[i]);
    // as k_fai_tile_scan: thread t of round `base` holds tile base + t
    const auto op = fault == F_PLAIN ? fai_combine : fai_seg_combine;
    FaiSum carry;
    for (size_t base = 0; fault == F_ROUNDS ? base + 256 <= n_tiles : base < n_tiles; base += 256) {
        FaiSum sh[256];
        for (uint32_t t = 0; t < 256; ++t)
            if (base + t < n_tiles) sh[t] = agg[base + t];
        for (uint32_t o = 1; o < 256; o <<= 1)
            for (uint32_t t = 255; t >= o; --t) sh[t] = fai_seg_combine(sh[t - o], sh[t]);
        if (fault == F_EARLY) carry = op(carry, sh[255]);
        for (uint32_t t = 0; t < 256 && base + t < n_tiles; ++t) {
            const bool drop = fault == F_NOCARRY || (fault == F_NOCARRY_T0 && !t) || (fault == F_NOCARRY_REST && t);
            const FaiSum c = drop ? FaiSum() : carry;
            if (fault == F_INCLUSIVE) excl[base + t] = op(c, sh[t]);
            else excl[base + t] = t ? op(c, sh[t - 1]) : c;
        }
        if (fault == F_RESTART) carry = sh[255];
        else if (fault != F_EARLY) carry = op(carry, sh[255]);
    }
    std::vector<FaiRow> rows(recs.size());
    for (size_t r = 0; r < recs.size(); ++r) rows[r].offset = recs[r].text_off;
    for (size_t t = 0; t < n_tiles; ++t) {
        FaiSum run;
        for (size_t i = t * 256; i < n_items && i < (t + 1) * 256; ++i) {
            run = fai_seg_combine(run, sums[i]);
            const uint32_t r = items[i].rec;
            if (i + 1 < n_items && items[i + 1].rec == r) continue;
            const FaiSum whole = fault == F_ROWS_PLAIN ? fai_combine(excl[t], run) : fai_seg_combine(excl[t], run);
            rows[r] = fai_finish(whole, recs[r].text_off, (size_t)r + 1 == recs.size());
        }
    }
    for (size_t r = 0; r < recs.size(); ++r)
        if (rows[r].err_at != FAI_NONE) {
            printf("refused %zu %s %llu\n", r, recs[r].id.c_str(), (unsigned long long)rows[r].err_at);
            return 3;
        }
    std::unordered_set<std::string> seen;
    for (size_t r = 0; r < recs.size(); ++r) {
        if (!seen.insert(recs[r].id).second) {
            fprintf(stderr, "ignoring duplicate sequence \"%s\"\n", recs[r].id.c_str());
            continue;
        }
        printf("%s\t%llu\t%llu\t%llu\t%llu\n", recs[r].id.c_str(), (unsigned long long)rows[r].length, (unsigned long long)rows[r].offset,
               (unsigned long long)rows[r].linebases, (unsigned long long)rows[r].linewidth);
    }
    return 0;
}
