// nthash_check.cpp -- the device helpers of ntjoin_amd/csrc/nthash_dev.h run on the host against the oracle's direct ntHash
// formula (oracle/mx_oracle.c: mxo_nthash_direct), over the whole range of k the library accepts, with the tables the library
// builds (ntjoin_amd/csrc/nthash_tab.h).
//   nthash_check         prints "<check> <cases>" per check and "OK"; exit status 1 and the first mismatch on stderr otherwise
// A stand-alone host program.  tests/test_nthash_cpu.py copies nthash_dev.h beside the stand-in headers of tools/nthash_shim
// (which give __device__, uint4 and v_alignbit_b32 a host meaning), builds this file against that copy plainly and with
// AddressSanitizer + UndefinedBehaviorSanitizer, and links oracle/mx_oracle.c in.
//
// Every packed buffer is allocated to end exactly 1 KiB behind the byte of its last base -- what include/ntjoin_mx.h promises
// the library about a borrowed buffer (mxg_add_packed) -- and the k-mer hashed from a table is the buffer's last, so the
// sanitized run checks that no helper reads further than that.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "nthash_dev.h"
#include "nthash_tab.h"

#include "mx_oracle.h"

using namespace mxg;

namespace {
constexpr uint32_t K_MAX = 1024, N_OFF = 48;
constexpr size_t PAST_END = 1024;  // bytes readable behind the last base (include/ntjoin_mx.h, mxg_add_packed)
constexpr uint64_t MULTISEED = 0x90b45d39fb6da1faull;

std::mt19937_64 rng(20240607);

std::string random_bases(size_t n)
{
    std::string s(n, 'A');
    for (size_t i = 0; i < n; ++i) s[i] = "ACGT"[rng() & 3u];
    return s;
}
uint32_t code(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; }

// 2 bits a base, base i in bits 2(i & 15) of word i >> 4; the allocation ends PAST_END bytes behind the last base's byte
struct Packed {
    uint32_t *w;
    explicit Packed(const std::string &s)
    {
        const size_t bytes = (s.size() + 3) / 4 + PAST_END;
        w = static_cast<uint32_t *>(malloc(bytes));
        if (!w) abort();
        memset(w, 0, bytes);
        unsigned char *b = reinterpret_cast<unsigned char *>(w);
        for (size_t i = 0; i < s.size(); ++i) b[i >> 2] |= (unsigned char)(code(s[i]) << (2 * (i & 3)));  // (little endian)
    }
    ~Packed() { free(w); }
    Packed(const Packed &) = delete;
    Packed &operator=(const Packed &) = delete;
};

uint64_t fwd(const H2 &h) { return ((uint64_t)h.fhi << 32) | h.flo; }
uint64_t rev(const H2 &h) { return ((uint64_t)h.rhi << 32) | h.rlo; }

[[noreturn]] void fail(const char *what, uint32_t k, uint64_t at, uint64_t got_f, uint64_t got_r, uint64_t want_f, uint64_t want_r)
{
    fprintf(stderr, "MISMATCH %s k=%u at=%llu got=%016llx/%016llx want=%016llx/%016llx\n", what, k, (unsigned long long)at,
            (unsigned long long)got_f, (unsigned long long)got_r, (unsigned long long)want_f, (unsigned long long)want_r);
    exit(1);
}
void expect(const char *what, uint32_t k, uint64_t at, const H2 &h, uint64_t f, uint64_t r)
{
    if (fwd(h) != f || rev(h) != r) fail(what, k, at, fwd(h), rev(h), f, r);
}

void split(uint64_t x, uint32_t &lo, uint32_t &hi) { lo = (uint32_t)x, hi = (uint32_t)(x >> 32); }
uint64_t join(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// ---- every k, 48 first-base offsets: the three initialisers (k = 32: four) and what is derived from a state
uint64_t k_sweep(const std::vector<uint4> &init, const std::vector<uint4> &half)
{
    uint64_t cases = 0;
    for (uint32_t k = 1; k <= K_MAX; ++k) {
        uint4 tab[20];
        nttab::hash_tab(k, tab);
        const uint64_t mult = 1ull ^ ((uint64_t)k * MULTISEED);
        for (uint32_t off = 0; off < N_OFF; ++off) {
            const std::string s = random_bases(off + k);  // the k-mer is the buffer's last
            const Packed p(s);
            uint64_t f = 0, r = 0;
            if (!mxo_nthash_direct(s.data() + off, k, &f, &r)) fail("oracle refused ACGT", k, off, 0, 0, 0, 0);
            H2 h = {0u, 0u, 0u, 0u};
            warm_up(h, p.w, off, k, tab);
            expect("warm_up", k, off, h, f, r);
            h = H2{1u, 2u, 3u, 4u};  // (the table routes overwrite the state)
            init_direct(h, p.w, off, k, init.data(), tab);
            expect("init_direct", k, off, h, f, r);
            h = H2{5u, 6u, 7u, 8u};
            init_pos(h, p.w, off, k, init.data() + 256, tab);
            expect("init_pos", k, off, h, f, r);
            if (k == 32) {
                h = H2{9u, 9u, 9u, 9u};
                init32_half(h, p.w, off, half.data());
                expect("init32_half", k, off, h, f, r);
            }
            const uint64_t v2 = canonical<MXG_VARIANT_V2_SUM>(h), v1 = canonical<MXG_VARIANT_V1_MIN>(h);
            if (v2 != mxo_canonical(f, r, MXO_VARIANT_V2_SUM)) fail("canonical<V2>", k, off, v2, 0, mxo_canonical(f, r, MXO_VARIANT_V2_SUM), 0);
            if (v1 != mxo_canonical(f, r, MXO_VARIANT_V1_MIN)) fail("canonical<V1>", k, off, v1, 0, mxo_canonical(f, r, MXO_VARIANT_V1_MIN), 0);
            if (is_forward(h) != (f <= r)) fail("is_forward", k, off, is_forward(h), 0, f <= r, 0);
            if (ext_hash(v2, mult) != mxo_ext_hash(v2, k)) fail("ext_hash", k, off, ext_hash(v2, mult), 0, mxo_ext_hash(v2, k), 0);
            if (ext_hash(v1, mult) != mxo_ext_hash(v1, k)) fail("ext_hash", k, off, ext_hash(v1, mult), 0, mxo_ext_hash(v1, k), 0);
            ++cases;
        }
    }
    return cases;
}

// ---- nt_step through the step table's outgoing x incoming entries: after every step the state is the new k-mer's direct hash
uint64_t rolling()
{
    const uint32_t ks[] = {1, 31, 32, 33, 64, 1023, 1024};
    const uint32_t STEPS = 2000;
    uint64_t cases = 0;
    bool seen[16] = {};
    for (uint32_t k : ks) {
        uint4 tab[20];
        nttab::hash_tab(k, tab);
        const uint32_t off = 5 + k % 16;
        const std::string s = random_bases(off + k + STEPS);
        const Packed p(s);
        H2 h = {0u, 0u, 0u, 0u};
        warm_up(h, p.w, off, k, tab);
        for (uint32_t i = 0; i < STEPS; ++i) {
            const uint32_t out = code(s[off + i]), in = code(s[off + i + k]);
            if (out != (fetch16(p.w, off + i) & 3u) || in != (fetch16(p.w, off + i + k) & 3u)) fail("fetch16", k, i, out, in, 0, 0);
            nt_step(h, tab[out * 4 + in]);
            seen[out * 4 + in] = true;
            uint64_t f = 0, r = 0;
            mxo_nthash_direct(s.data() + off + i + 1, k, &f, &r);
            expect("nt_step", k, i, h, f, r);
            ++cases;
        }
    }
    for (int e = 0; e < 16; ++e)
        if (!seen[e]) fail("step table entry never used", 0, e, 0, 0, 0, 0);
    return cases;
}

// ---- the rotation helpers against repeated single steps
uint64_t rotations()
{
    uint64_t cases = 0;
    for (int t = 0; t < 200; ++t) {
        const uint64_t x = t == 0 ? 0 : t == 1 ? ~0ull : rng();
        uint32_t lo, hi;
        uint64_t y = x;
        for (int i = 0; i < 4; ++i) y = mxo_srol(y);
        split(x, lo, hi), srol4(lo, hi);
        if (join(lo, hi) != y) fail("srol4", 0, t, join(lo, hi), 0, y, 0);
        sror4(lo, hi);
        if (join(lo, hi) != x) fail("sror4 o srol4", 0, t, join(lo, hi), 0, x, 0);
        y = x;
        for (int i = 0; i < 4; ++i) y = mxo_sror(y);
        split(x, lo, hi), sror4(lo, hi);
        if (join(lo, hi) != y) fail("sror4", 0, t, join(lo, hi), 0, y, 0);
        y = x;
        for (int i = 0; i < 16; ++i) y = mxo_srol(y);
        split(x, lo, hi), srol16(lo, hi);
        if (join(lo, hi) != y) fail("srol16", 0, t, join(lo, hi), 0, y, 0);
        y = x;
        for (uint32_t n = 0; n <= 1100; ++n) {
            split(x, lo, hi), srol_var(lo, hi, n);
            if (join(lo, hi) != y) fail("srol_var", n, t, join(lo, hi), 0, y, 0);
            if (nttab::srol_n(x, n) != y) fail("nttab::srol_n", n, t, nttab::srol_n(x, n), 0, y, 0);
            y = mxo_srol(y);
            ++cases;
        }
    }
    return cases;
}
}  // namespace

int main()
{
    std::vector<uint4> init, half;
    nttab::init_tab(init);
    nttab::half_tab(init, half);
    printf("k_sweep %llu\n", (unsigned long long)k_sweep(init, half));
    printf("rolling %llu\n", (unsigned long long)rolling());
    printf("rotations %llu\n", (unsigned long long)rotations());
    printf("OK\n");
    return 0;
}
