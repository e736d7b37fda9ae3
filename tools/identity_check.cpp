// identity_check.cpp -- the banded edit distance of string pairs (mxg_identity_segments) by the code of the device route run
// serially on the host (ntjoin_amd/csrc/identity.h): the status rules that need no base, then idy_align over two fetchers that
// hand out base classes from the strings, the subject's backwards and complemented for a reverse pair.
//   identity_check FILE     every line of FILE: max_seg reverse QUERY SUBJECT (separated by blanks; QUERY and SUBJECT are the bytes
//                           of the two intervals, at least one each, as they stand in the text: SUBJECT is not yet reversed)
//   stdout: one line "edits status saturated" per pair (status: MXG_IDY_ALIGNED .. MXG_IDY_SKIP_N; edits 0 when skipped)
//   exit status 0; 2: usage / unreadable or malformed file
// A stand-alone host program (c++ -std=c++17 -I include -I ntjoin_amd/csrc tools/identity_check.cpp); tests/test_identity_cpu.py
// builds it plainly and with AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "identity.h"

using namespace mxg;

struct StringFetcher {
    const std::string &s;
    size_t at;
    bool backwards;
    StringFetcher(const std::string &s_, bool b) : s(s_), at(b ? s_.size() - 1 : 0), backwards(b) {}
    uint32_t next()
    {
        const uint32_t c = idy_byte_class((unsigned char)s.at(at));  // (at() checks: a fetch beyond the interval ends the program)
        at = backwards ? at - 1 : at + 1;
        return backwards && c < 4u ? 3u - c : c;
    }
};

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        unsigned long long max_seg = 0, reverse = 0;
        std::string q, s;
        if (!(ls >> max_seg >> reverse >> q >> s) || !max_seg || max_seg > 0xFFFFFFFFull || q.empty() || s.empty() || q.size() > 0xFFFFFFFFull ||
            s.size() > 0xFFFFFFFFull)
            return 2;
        const uint32_t lq = (uint32_t)q.size(), lsub = (uint32_t)s.size();
        uint32_t edits = 0, sat = 0;
        uint32_t st = idy_precheck(lq, lsub, (uint32_t)max_seg);
        if (st == MXG_IDY_ALIGNED) {
            StringFetcher fq(q, false), fs(s, reverse != 0);
            st = idy_align(fq, fs, lq, lsub, &edits, &sat);
            if (st != MXG_IDY_ALIGNED) edits = 0, sat = 0;
        }
        printf("%u %u %u\n", edits, st, sat);
    }
    return 0;
}
