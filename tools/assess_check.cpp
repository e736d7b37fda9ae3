// assess_check.cpp -- chains, breakpoints and the summary of a list of kept synteny blocks (mxg_synteny_assess) by the code of the
// device route run serially on the host (ntjoin_amd/csrc/assess.h): per block its head flag, the heads and the anchors counted, per
// chain its first and last block, per chain boundary its kind and whether it falls on a join, the chains sorted by their key in
// subject order and the running maximum of the cover words, the lengths sorted by their key, their running sums and the lower
// bounds.  Only the sort itself is the host's (std::stable_sort over the same keys).
//   assess_check FILE       FILE holds numbers separated by white space:
//                           k merge_gap max_indel join_indel
//                           the number of query records, then their lengths; the number of subject records, then their lengths
//                           the number of blocks, then eight numbers per block, in order:
//                               n_anchors q_record q_start q_end s_record s_start s_end reverse
//                           0, or 1 and the query's piece table: n_records, then per record its number of pieces and their lengths
//   stdout: n_blocks n_chains n_breakpoints, the six counters (kind-major, at_join 0 then 1), query_bases subject_bases
//           aligned_query chained_subject covered_subject;
//           a line "X" + 18 numbers: na, nga, ng as n50 l50 n75 l75 n90 l90;
//           one line "C" + ten fields per chain, one line "B" + five fields per breakpoint (the orders of the view)
//   exit status 0; 2: usage / unreadable file; 5: internal inconsistency
// A stand-alone host program (c++ -std=c++17 -I include -I ntjoin_amd/csrc tools/assess_check.cpp); tests/test_assess_cpu.py builds
// it plainly and with AddressSanitizer + UndefinedBehaviorSanitizer.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "assess.h"

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
    uint32_t k = 0;
    mxg_assess_params p{};
    p.struct_size = sizeof p;
    unsigned long long n_q = 0, n_s = 0, n = 0, has_table = 0;
    if (fscanf(fh, "%u %u %u %u %llu", &k, &p.merge_gap, &p.max_indel, &p.join_indel, &n_q) != 5) return 2;
    std::vector<uint32_t> qlen(n_q);
    for (uint32_t &v : qlen)
        if (fscanf(fh, "%u", &v) != 1) return 2;
    if (fscanf(fh, "%llu", &n_s) != 1) return 2;
    std::vector<uint32_t> slen(n_s);
    for (uint32_t &v : slen)
        if (fscanf(fh, "%u", &v) != 1) return 2;
    if (fscanf(fh, "%llu", &n) != 1) return 2;
    std::vector<uint32_t> blk(n * 8);  // eight arrays of n words, as the view's host copy holds them
    for (unsigned long long i = 0; i < n; ++i)
        for (unsigned long long u = 0; u < 8; ++u)
            if (fscanf(fh, "%u", &blk[u * n + i]) != 1) return 2;
    if (fscanf(fh, "%llu", &has_table) != 1) return 2;
    std::vector<uint32_t> pre, first{0};
    if (has_table) {
        unsigned long long n_rec = 0, m = 0;
        if (fscanf(fh, "%llu", &n_rec) != 1) return 2;
        for (unsigned long long r = 0; r < n_rec; ++r) {
            if (fscanf(fh, "%llu", &m) != 1) return 2;
            uint32_t at = 0, len = 0;
            for (unsigned long long j = 0; j < m; ++j) {
                if (fscanf(fh, "%u", &len) != 1) return 2;
                pre.push_back(at);
                at += len;
            }
            first.push_back((uint32_t)pre.size());
        }
    }
    const uint32_t *d_pre = has_table ? pre.data() : nullptr, *d_first = has_table ? first.data() : nullptr;
    // ---- heads, scanned; the anchors, scanned; the chains' ends
    std::vector<uint32_t> head(n, 0), hscan(n, 0), ascan(n + 1, 0);
    uint32_t n_ch = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const SynBlock b = as_block(blk.data(), n, i);
        head[i] = (i == 0 || !as_joined(as_block(blk.data(), n, i - 1), b, k, p, d_pre, d_first)) ? 1u : 0u;
        hscan[i] = n_ch;
        n_ch += head[i];
        ascan[i + 1] = ascan[i] + b.n_anchors;
    }
    std::vector<uint32_t> cfirst(n_ch, ~0u), clast(n_ch, ~0u);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t c = hscan[i] + head[i] - 1u;
        if (head[i]) cfirst.at(c) = (uint32_t)i;
        if (i + 1 == n || head[i + 1]) clast.at(c) = (uint32_t)i;
    }
    std::vector<AsChain> chain(n_ch);
    uint64_t aligned = 0, chained = 0;
    for (uint32_t c = 0; c < n_ch; ++c) {
        const uint32_t f = cfirst[c], l = clast[c];
        if (f > l || l >= n) {
            fprintf(stderr, "chain %u has no first or no last block\n", c);
            return 5;
        }
        chain[c] = as_chain(as_block(blk.data(), n, f), as_block(blk.data(), n, l), f, l, ascan[l + 1] - ascan[f]);
        aligned += chain[c].q_end - chain[c].q_start;
        chained += chain[c].s_end - chain[c].s_start;
    }
    // ---- breakpoints
    struct Bp {
        uint32_t chain, kind, at_join, q_lo, q_hi;
    };
    std::vector<Bp> bps;
    uint64_t counter[6] = {};
    for (uint32_t c = 0; c + 1 < n_ch; ++c) {
        const AsChain &x = chain[c], &y = chain[c + 1];
        if (x.q_record != y.q_record) continue;
        const uint32_t kind = as_kind(x.s_record, x.reverse, y.s_record, y.reverse);
        const uint32_t j = as_at_join(as_block(blk.data(), n, x.first_block + x.n_blocks - 1u), as_block(blk.data(), n, y.first_block), d_pre, d_first) ? 1u : 0u;
        bps.push_back({c, kind, j, x.q_end, y.q_start});
        ++counter[kind * 2 + j];
    }
    // ---- the union of the subject intervals
    std::vector<std::pair<uint64_t, uint32_t>> order(n_ch);
    for (uint32_t c = 0; c < n_ch; ++c) order[c] = {as_place_key(chain[c].s_record, chain[c].s_start), c};
    std::stable_sort(order.begin(), order.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    uint64_t run = 0, covered = 0;
    for (const auto &o : order) {
        const uint64_t w = as_cover_word((uint32_t)(o.first >> 32), chain[o.second].s_end);
        covered += as_uncovered(run, (uint32_t)(o.first >> 32), (uint32_t)o.first, (uint32_t)w);
        if (w > run) run = w;
    }
    // ---- Nx
    uint64_t query_bases = 0, subject_bases = 0;
    for (uint32_t v : qlen) query_bases += v;
    for (uint32_t v : slen) subject_bases += v;
    auto nx = [](std::vector<uint64_t> keys, std::initializer_list<uint64_t> ds) {
        std::stable_sort(keys.begin(), keys.end());
        std::vector<uint64_t> ex(keys.size() + 1, 0);
        for (size_t j = 0; j < keys.size(); ++j) ex[j + 1] = ex[j] + as_key_len(keys[j]);
        for (uint64_t d : ds)
            for (uint32_t x : {50u, 75u, 90u}) {
                const uint64_t l = as_lx(ex.data(), keys.size(), x, d);
                printf(" %u %llu", l ? as_key_len(keys[l - 1]) : 0u, (unsigned long long)l);
            }
    };
    printf("%llu %u %zu", n, n_ch, bps.size());
    for (uint64_t v : counter) printf(" %llu", (unsigned long long)v);
    printf(" %llu %llu %llu %llu %llu\n", (unsigned long long)query_bases, (unsigned long long)subject_bases, (unsigned long long)aligned,
           (unsigned long long)chained, (unsigned long long)covered);
    std::vector<uint64_t> spans(n_ch), qkeys(qlen.size());
    for (uint32_t c = 0; c < n_ch; ++c) spans[c] = as_len_key(chain[c].q_end - chain[c].q_start);
    for (size_t r = 0; r < qlen.size(); ++r) qkeys[r] = as_len_key(qlen[r]);
    printf("X");
    nx(spans, {query_bases, subject_bases});
    nx(qkeys, {subject_bases});
    printf("\n");
    for (const AsChain &c : chain)
        printf("C %u %u %u %u %u %u %u %u %u %u\n", c.n_blocks, c.first_block, c.n_anchors, c.q_record, c.q_start, c.q_end, c.s_record, c.s_start, c.s_end,
               c.reverse);
    for (const Bp &b : bps) printf("B %u %u %u %u %u\n", b.chain, b.kind, b.at_join, b.q_lo, b.q_hi);
    return 0;
}
