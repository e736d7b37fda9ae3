// compose_check.cpp -- the composition of two piece tables (mxg_compose_pieces) by the code of the device route run serially on the
// host (ntjoin_amd/csrc/compose.h): the tables' check and prefix, per outer piece the bisection and the clip of every inner piece it
// meets, then neighbouring gaps of one record joined.
//   compose_check FILE      FILE holds numbers separated by white space: the inner table, then the outer table, each as
//                           n_records, then per record its number of pieces and four numbers {record start end kind} per piece
//   stdout: one line per outer record: its number of pieces, then four numbers per piece
//   exit status 0; 2: usage / unreadable file; 3: the tables are refused as MXG_EINVAL, 4: as MXG_ELIMIT (the reason on stderr)
// A stand-alone host program (c++ -std=c++17 -I include -I ntjoin_amd/csrc tools/compose_check.cpp); tests/test_compose_cpu.py builds
// it plainly and with AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "compose.h"

using namespace mxg;

namespace {

struct Table {
    std::vector<mxg_seq_piece> pieces;
    std::vector<uint64_t> first{0};
};

bool read_table(FILE *fh, Table &t)
{
    unsigned long long n = 0, m = 0;
    if (fscanf(fh, "%llu", &n) != 1) return false;
    for (unsigned long long r = 0; r < n; ++r) {
        if (fscanf(fh, "%llu", &m) != 1) return false;
        for (unsigned long long j = 0; j < m; ++j) {
            mxg_seq_piece p;
            if (fscanf(fh, "%u %u %u %u", &p.record, &p.start, &p.end, &p.kind) != 4) return false;
            t.pieces.push_back(p);
        }
        t.first.push_back(t.pieces.size());
    }
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *fh = fopen(argv[1], "r");
    if (!fh) return 2;
    Table in, out;
    const bool ok = read_table(fh, in) && read_table(fh, out);
    fclose(fh);
    if (!ok) return 2;
    const uint64_t n_inner = in.first.size() - 1, n_outer = out.first.size() - 1;
    CmpTable ti, to;
    std::string msg;
    int rc = cmp_table("inner", in.pieces.data(), in.first.data(), n_inner, ~0ull, nullptr, ti, msg);
    if (rc == MXG_OK) rc = cmp_table("outer", out.pieces.data(), out.first.data(), n_outer, n_inner, ti.len.data(), to, msg);
    if (rc != MXG_OK) {
        fprintf(stderr, "%s\n", msg.c_str());
        return rc == MXG_ELIMIT ? 4 : 3;
    }
    for (uint64_t r = 0; r < n_outer; ++r) {
        std::vector<mxg_seq_piece> res;
        for (uint32_t i = to.first[r]; i < to.first[r + 1]; ++i) {
            const mxg_seq_piece &p = out.pieces[i];
            uint32_t n = 1, f = 0, j_lo = 0, j_hi = 0;
            if (p.kind != MXG_PIECE_GAP) {
                f = ti.first[p.record];
                cmp_range(ti.pre.data() + f, ti.first[p.record + 1] - f, p.start, p.end, j_lo, j_hi);
                n = j_hi - j_lo + 1;
            }
            for (uint32_t t = 0; t < n; ++t) {
                mxg_seq_piece o = {0, 0, cmp_len(p), MXG_PIECE_GAP};
                if (p.kind != MXG_PIECE_GAP) o = cmp_expand(p, in.pieces.data() + f, ti.pre.data() + f, j_lo, j_hi, t);
                if (o.kind == MXG_PIECE_GAP && !res.empty() && res.back().kind == MXG_PIECE_GAP) res.back().end += cmp_len(o);
                else res.push_back(o);
            }
        }
        printf("%zu", res.size());
        for (const mxg_seq_piece &o : res) printf(" %u %u %u %u", o.record, o.start, o.end, o.kind);
        printf("\n");
    }
    return 0;
}
