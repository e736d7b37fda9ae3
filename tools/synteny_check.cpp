// synteny_check.cpp -- the synteny blocks of an anchor list (mxg_synteny_blocks) by the code of the device route run serially on the
// host (ntjoin_amd/csrc/synteny.h, compose.h's table check): per piece the two lower bounds and every anchor it takes, per link its
// code, head and tail flags, the heads counted, every block from its first and last anchor, the filter.
//   synteny_check FILE      FILE holds numbers separated by white space:
//                           k max_gap min_anchors min_span
//                           the number of query records, then their lengths
//                           the number of anchors, then four numbers {qrec qpos srec spos} per anchor, in any order (sorted here by
//                           (qrec, qpos), as the query's sketch is)
//                           0, or 1 and a piece table: n_records, then per record its number of pieces and four numbers
//                           {record start end kind} per piece
//   stdout: "n_anchors_total n_links", then one line per kept block:
//           n_anchors q_record q_start q_end s_record s_start s_end reverse matches blocklen    (the last two: PAF columns 10, 11)
//   exit status 0; 2: usage / unreadable file; 3: refused as MXG_EINVAL, 4: as MXG_ELIMIT (the reason on stderr)
// A stand-alone host program (c++ -std=c++17 -I include -I ntjoin_amd/csrc tools/synteny_check.cpp); tests/test_synteny_cpu.py builds
// it with AddressSanitizer + UndefinedBehaviorSanitizer.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "compose.h"
#include "synteny.h"

using namespace mxg;

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *fh = fopen(argv[1], "r");
    if (!fh) return 2;
    struct Closer {
        FILE *f;
        ~Closer() { fclose(f); }
    } closer{fh};
    uint32_t k = 0, max_gap = 0, min_anchors = 0, min_span = 0;
    unsigned long long n_qrec = 0, n = 0, has_table = 0;
    if (fscanf(fh, "%u %u %u %u %llu", &k, &max_gap, &min_anchors, &min_span, &n_qrec) != 5) return 2;
    std::vector<uint32_t> qlen(n_qrec);
    for (uint32_t &v : qlen)
        if (fscanf(fh, "%u", &v) != 1) return 2;
    if (fscanf(fh, "%llu", &n) != 1) return 2;
    std::vector<SynAnchor> a(n);
    for (SynAnchor &x : a)
        if (fscanf(fh, "%u %u %u %u", &x.qrec, &x.qpos, &x.srec, &x.spos) != 4) return 2;
    if (fscanf(fh, "%llu", &has_table) != 1) return 2;
    std::vector<mxg_seq_piece> pieces;
    std::vector<uint64_t> first{0};
    if (has_table) {
        unsigned long long n_rec = 0, m = 0;
        if (fscanf(fh, "%llu", &n_rec) != 1) return 2;
        for (unsigned long long r = 0; r < n_rec; ++r) {
            if (fscanf(fh, "%llu", &m) != 1) return 2;
            for (unsigned long long j = 0; j < m; ++j) {
                mxg_seq_piece p;
                if (fscanf(fh, "%u %u %u %u", &p.record, &p.start, &p.end, &p.kind) != 4) return 2;
                pieces.push_back(p);
            }
            first.push_back(pieces.size());
        }
    }
    if (min_anchors < 2) {
        fprintf(stderr, "min_anchors is %u; a block has at least two anchors\n", min_anchors);
        return 3;
    }
    std::sort(a.begin(), a.end(), [](const SynAnchor &x, const SynAnchor &y) { return x.qrec != y.qrec ? x.qrec < y.qrec : x.qpos < y.qpos; });
    // ---- through the piece table: count, offsets, emit
    if (has_table) {
        CmpTable t;
        std::string msg;
        const int rc = cmp_table("query", pieces.data(), first.data(), first.size() - 1, n_qrec, qlen.data(), t, msg);
        if (rc != MXG_OK) {
            fprintf(stderr, "%s\n", msg.c_str());
            return rc == MXG_ELIMIT ? 4 : 3;
        }
        std::vector<uint64_t> lo(pieces.size()), hi(pieces.size()), at(pieces.size() + 1, 0);
        for (size_t i = 0; i < pieces.size(); ++i) {
            syn_piece_range(a.data(), a.size(), pieces[i], k, lo[i], hi[i]);
            at[i + 1] = at[i] + (hi[i] - lo[i]);
        }
        std::vector<SynAnchor> out(at.back());
        for (size_t i = 0; i < pieces.size(); ++i)
            for (uint64_t u = 0; u < hi[i] - lo[i]; ++u) out[at[i] + u] = syn_piece_anchor(a.data(), pieces[i], k, lo[i], hi[i], u, t.rec[i], t.pre[i]);
        a.swap(out);
    }
    // ---- links, heads, the blocks' ends, the blocks
    const uint64_t m = a.size();
    std::vector<uint32_t> head(m, 0), hscan(m, 0);
    uint64_t n_links = 0, n_blk = 0;
    for (uint64_t i = 0; i < m; ++i) {
        const uint32_t c = syn_link_at(a.data(), m, (int64_t)i, max_gap);
        n_links += c != SYN_NONE;
        head[i] = syn_is_head(syn_link_at(a.data(), m, (int64_t)i - 1, max_gap), c) ? 1u : 0u;
        hscan[i] = (uint32_t)n_blk;
        n_blk += head[i];
    }
    std::vector<uint64_t> bfirst(n_blk, ~0ull), blast(n_blk, ~0ull);
    for (uint64_t i = 0; i < m; ++i) {
        const uint32_t c = syn_link_at(a.data(), m, (int64_t)i, max_gap);
        if (c == SYN_NONE) continue;
        if (head[i]) bfirst.at(hscan[i]) = i;
        if (syn_is_tail(c, syn_link_at(a.data(), m, (int64_t)i + 1, max_gap))) blast.at(hscan[i] + head[i] - 1u) = i + 1;
    }
    printf("%llu %llu\n", (unsigned long long)m, (unsigned long long)n_links);
    for (uint64_t b = 0; b < n_blk; ++b) {
        if (bfirst[b] >= blast[b] || blast[b] >= m) {
            fprintf(stderr, "block %llu has no head or no tail\n", (unsigned long long)b);
            return 5;
        }
        const SynBlock o = syn_block(a[bfirst[b]], a[blast[b]], bfirst[b], blast[b] - 1, k);
        if (!syn_keep(o, min_anchors, min_span)) continue;
        printf("%u %u %u %u %u %u %u %u %llu %llu\n", o.n_anchors, o.q_record, o.q_start, o.q_end, o.s_record, o.s_start, o.s_end, o.reverse,
               (unsigned long long)syn_matches(o, k), (unsigned long long)syn_blocklen(o));
    }
    return 0;
}
