// bisect_check.cpp -- runs the bisections of ntjoin_amd/csrc/bisect.h on the host, on arrays from files, and prints what they
// return.  It decides nothing about right and wrong: tests/test_bisect_cpu.py computes every expected value.  Arrays are raw
// little-endian 64-bit words; the element count is the file's size.  Plain C++: bisect.h is all it includes of the project.
// Build: c++ -std=c++17 -O1 -Wall -Werror -I ntjoin_amd/csrc tools/bisect_check.cpp -o bisect_check
// Usage: bisect_check owner <keys.u64> <queries.u64> <lo> <hi>   per query "a b": a = last_le over [lo, hi) with 32-bit indices,
//                                                                 b = last_where with 64-bit indices and a predicate that ends
//                                                                 the program (exit 4) when it is asked about lo
//        bisect_check first <keys.u64> <queries.u64> <lo> <hi>   per query "a b": a = first_ge, b = first_gt over [lo, hi)
//        bisect_check wrap <lo> <hi> <t> ...                     per t: first_where over 32-bit indices [lo, hi) of the predicate
//                                                                 i >= t, which reads no memory
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bisect.h"

static std::vector<uint64_t> read_u64(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(3);
    }
    std::vector<uint64_t> v;
    uint64_t w;
    while (fread(&w, 8, 1, f) == 1) v.push_back(w);
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    const std::string op = argc > 1 ? argv[1] : "";
    if ((op == "owner" || op == "first") && argc == 6) {
        const std::vector<uint64_t> keys = read_u64(argv[2]), queries = read_u64(argv[3]);
        const uint64_t lo = strtoull(argv[4], nullptr, 10), hi = strtoull(argv[5], nullptr, 10);
        if (lo > hi || hi > keys.size() || hi > 0xFFFFFFFFull) {
            fprintf(stderr, "[%llu, %llu) of %zu keys\n", (unsigned long long)lo, (unsigned long long)hi, keys.size());
            return 3;
        }
        const uint64_t *arr = keys.data();
        for (const uint64_t x : queries) {
            uint64_t a, b;
            if (op == "owner") {
                a = mxg::last_le(arr, (uint32_t)lo, (uint32_t)hi, x);
                b = mxg::last_where(lo, hi, [&](uint64_t i) {
                    if (i == lo) exit(4);
                    return arr[i] <= x;
                });
            } else {
                a = mxg::first_ge(arr, (uint32_t)lo, (uint32_t)hi, x);
                b = mxg::first_gt(arr, lo, hi, x);
            }
            printf("%llu %llu\n", (unsigned long long)a, (unsigned long long)b);
        }
        return 0;
    }
    if (op == "wrap" && argc >= 5) {
        const uint32_t lo = (uint32_t)strtoull(argv[2], nullptr, 0), hi = (uint32_t)strtoull(argv[3], nullptr, 0);
        for (int j = 4; j < argc; ++j) {
            const uint32_t t = (uint32_t)strtoull(argv[j], nullptr, 0);
            printf("%u\n", mxg::first_where(lo, hi, [&](uint32_t i) { return i >= t; }));
        }
        return 0;
    }
    fprintf(stderr, "usage: bisect_check owner|first KEYS QUERIES LO HI | wrap LO HI T...\n");
    return 3;
}
