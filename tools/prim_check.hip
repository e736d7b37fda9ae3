// prim_check.hip -- runs ONE of the shared primitives (ntjoin_amd/csrc/scan_kernels.h, scan64_kernels.h, sort_kernels.h, bisect.h) once
// on ONE input and writes what came out.  It decides nothing about right and wrong: tests/test_gpu_primitives.py computes every expected
// value.  Arrays are raw little-endian files; the element count is the file's size.
// Build: ntjoin_amd/csrc/Makefile (it links the library for launch_win_bounds)
// Usage: prim_check scan32 <in.u32> <out.u32> <total.u64>           launch_scan_u32 (n >= 1)
//        prim_check scan64 <in.u64> <out.u64>                       launch_scan_u64, in place (n >= 1)
//        prim_check maxscan64 <in.u64> <out.u64>                    launch_max_scan_u64, in place (n >= 1)
//        prim_check sort <key_bits> <keys.u64> <vals.u32> <keys_out.u64> <vals_out.u32>
//                                                                   launch_radix_sort; prints "buffer: <its return value>" and writes
//                                                                   the buffer that value names
//        prim_check prefix <q> <counts.u32>                         every producer block b publishes counts[b] (count_publish, sup
//                                                                   zeroed before); one wave prints "prefix: <count_prefix(q)>"
//        prim_check owner <keys.u64> <queries.u64> <out.u32>        one thread per query: last_le over all the keys (bisect.h)
//        prim_check first <keys.u64> <queries.u64> <out.u32>        one thread per query q of nq: out[q] = first_ge, out[nq + q] = first_gt
//        prim_check wrap <lo> <hi> <t.u32> <out.u32>                one thread per t: first_where over the 32-bit indices [lo, hi) of
//                                                                   the predicate i >= t, which reads no memory
//        prim_check winbounds <off.u64> <win> <out.u32>             launch_win_bounds (the library's, win_out.hip) over the n + 1 offsets
//                                                                   of a text of off[n] >= 1 bytes in windows of `win` bytes
// Every device array has exactly the size its header documents, between 64 guard bytes in front and 64 behind; after the run the
// guards are read back: "guards: ok", or "guards: changed <array> ..." for every array whose guards differ.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bisect.h"
#include "mxg_internal.h"
#include "scan64_kernels.h"
#include "scan_kernels.h"
#include "sort_kernels.h"

#define CK(x)                                                                                   \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) {                                                                 \
            fprintf(stderr, "%s failed: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); \
            exit(2);                                                                            \
        }                                                                                       \
    } while (0)

using namespace mxg;

constexpr size_t GUARD = 64;
constexpr int GUARD_BYTE = 0xA5, FILL_BYTE = 0xCD;  // (scratch and outputs start as 0xCD..: nothing may count on zeroed memory)

struct Guarded {
    const char *name;
    char *raw = nullptr;
    size_t bytes = 0;
    template <typename T>
    T *as() const { return reinterpret_cast<T *>(raw + GUARD); }
};
static std::vector<Guarded> g_arrays;

static Guarded dev_array(const char *name, size_t bytes, int fill = FILL_BYTE)
{
    Guarded g;
    g.name = name;
    g.bytes = bytes;
    CK(hipMalloc(reinterpret_cast<void **>(&g.raw), bytes + 2 * GUARD));
    CK(hipMemset(g.raw, GUARD_BYTE, GUARD));
    if (bytes) CK(hipMemset(g.raw + GUARD, fill, bytes));
    CK(hipMemset(g.raw + GUARD + bytes, GUARD_BYTE, GUARD));
    g_arrays.push_back(g);
    return g;
}
static void upload(const Guarded &g, const void *src, size_t bytes)
{
    if (bytes) CK(hipMemcpy(g.raw + GUARD, src, bytes, hipMemcpyHostToDevice));
}
static void report_guards()
{
    bool ok = true;
    unsigned char buf[2 * GUARD];
    for (const Guarded &g : g_arrays) {
        CK(hipMemcpy(buf, g.raw, GUARD, hipMemcpyDeviceToHost));
        CK(hipMemcpy(buf + GUARD, g.raw + GUARD + g.bytes, GUARD, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < 2 * GUARD; ++i)
            if (buf[i] != GUARD_BYTE) {
                printf("guards: changed %s (%s byte %zu)\n", g.name, i < GUARD ? "front" : "back", i % GUARD);
                ok = false;
                break;
            }
    }
    if (ok) printf("guards: ok\n");
}

template <typename T>
static std::vector<T> read_file(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(3);
    }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % (long)sizeof(T)) {
        fprintf(stderr, "%s: %ld bytes are no whole number of %zu-byte elements\n", path, bytes, sizeof(T));
        exit(3);
    }
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "short read of %s\n", path);
        exit(3);
    }
    fclose(f);
    return v;
}
static void write_file(const char *path, const void *p, size_t bytes)
{
    FILE *f = fopen(path, "wb");
    if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes) || fclose(f)) {
        fprintf(stderr, "cannot write %s\n", path);
        exit(3);
    }
}
template <typename T>
static void download(const char *path, const T *dev, size_t n)
{
    std::vector<T> v(n);
    if (n) CK(hipMemcpy(v.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost));
    write_file(path, v.data(), n * sizeof(T));
}
static uint32_t count_of(size_t n, const char *what)
{
    if (n >= (1ull << 31)) {
        fprintf(stderr, "%s: %zu elements, the primitives take fewer than 2^31\n", what, n);
        exit(3);
    }
    return (uint32_t)n;
}
static void finish(hipStream_t st)
{
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st));
}

// producer block b publishes counts[b]
static __global__ __launch_bounds__(64) void k_publish(const uint32_t *__restrict__ counts, uint32_t *__restrict__ cnt, uint32_t *__restrict__ sup)
{
    if (threadIdx.x == 0) count_publish(cnt, sup, blockIdx.x, counts[blockIdx.x]);
}
// one wave: the items of producer blocks [0, q)
static __global__ __launch_bounds__(64) void k_prefix(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ sup, uint32_t q, uint32_t *__restrict__ out)
{
    const uint32_t r = count_prefix(cnt, sup, q);
    if (threadIdx.x == 0) out[0] = r;
}

static int run_scan32(char **a)
{
    const std::vector<uint32_t> in = read_file<uint32_t>(a[0]);
    const uint32_t n = count_of(in.size(), a[0]);
    if (n == 0) {
        fprintf(stderr, "scan32: n = 0 is outside launch_scan_u32's contract\n");
        return 3;
    }
    const Guarded d_in = dev_array("in", (size_t)n * 4), d_out = dev_array("out", (size_t)n * 4);
    const Guarded d_bsum = dev_array("bsum", (size_t)((n + TILE - 1) / TILE) * 4), d_total = dev_array("total", 8);
    upload(d_in, in.data(), (size_t)n * 4);
    hipStream_t st = nullptr;
    launch_scan_u32(st, d_in.as<uint32_t>(), n, d_bsum.as<uint32_t>(), d_out.as<uint32_t>(), d_total.as<uint64_t>());
    finish(st);
    download(a[1], d_out.as<uint32_t>(), n);
    download(a[2], d_total.as<uint64_t>(), 1);
    return 0;
}

static int run_scan64(char **a)
{
    const std::vector<uint64_t> in = read_file<uint64_t>(a[0]);
    const uint32_t n = count_of(in.size(), a[0]);
    if (n == 0) {
        fprintf(stderr, "scan64: n = 0 is outside launch_scan_u64's contract\n");
        return 3;
    }
    const Guarded d_a = dev_array("a", (size_t)n * 8), d_tsum = dev_array("tsum", (size_t)((n + PT_TILE - 1) / PT_TILE) * 8);
    upload(d_a, in.data(), (size_t)n * 8);
    hipStream_t st = nullptr;
    launch_scan_u64(st, d_a.as<uint64_t>(), n, d_tsum.as<uint64_t>());
    finish(st);
    download(a[1], d_a.as<uint64_t>(), n);
    return 0;
}

static int run_maxscan64(char **a)
{
    const std::vector<uint64_t> in = read_file<uint64_t>(a[0]);
    const uint32_t n = count_of(in.size(), a[0]);
    if (n == 0) {
        fprintf(stderr, "maxscan64: n = 0 is outside launch_max_scan_u64's contract\n");
        return 3;
    }
    const Guarded d_a = dev_array("a", (size_t)n * 8), d_tmax = dev_array("tmax", (size_t)((n + PT_TILE - 1) / PT_TILE) * 8);
    upload(d_a, in.data(), (size_t)n * 8);
    hipStream_t st = nullptr;
    launch_max_scan_u64(st, d_a.as<uint64_t>(), n, d_tmax.as<uint64_t>());
    finish(st);
    download(a[1], d_a.as<uint64_t>(), n);
    return 0;
}

static int run_sort(char **a)
{
    const uint32_t key_bits = (uint32_t)strtoul(a[0], nullptr, 10);
    const std::vector<uint64_t> keys = read_file<uint64_t>(a[1]);
    const std::vector<uint32_t> vals = read_file<uint32_t>(a[2]);
    const uint32_t n = count_of(keys.size(), a[1]);
    if (vals.size() != keys.size() || key_bits < 1 || key_bits > 64) {
        fprintf(stderr, "sort: %zu keys, %zu values, key_bits %u\n", keys.size(), vals.size(), key_bits);
        return 3;
    }
    const Guarded k0 = dev_array("k0", (size_t)n * 8), v0 = dev_array("v0", (size_t)n * 4), k1 = dev_array("k1", (size_t)n * 8), v1 = dev_array("v1", (size_t)n * 4);
    const Guarded counts = dev_array("counts", rs_count_words(n) * 4), first = dev_array("first", rs_count_words(n) * 4);
    const Guarded bsum = dev_array("bsum", rs_bsum_words(n) * 4), total = dev_array("total", 8);
    upload(k0, keys.data(), (size_t)n * 8);
    upload(v0, vals.data(), (size_t)n * 4);
    hipStream_t st = nullptr;
    const int at = launch_radix_sort(st, k0.as<uint64_t>(), v0.as<uint32_t>(), k1.as<uint64_t>(), v1.as<uint32_t>(), n, key_bits, counts.as<uint32_t>(),
                                     first.as<uint32_t>(), bsum.as<uint32_t>(), total.as<uint64_t>());
    finish(st);
    printf("buffer: %d\n", at);
    download(a[3], (at ? k1 : k0).as<uint64_t>(), n);
    download(a[4], (at ? v1 : v0).as<uint32_t>(), n);
    return 0;
}

static int run_prefix(char **a)
{
    const uint32_t q = (uint32_t)strtoul(a[0], nullptr, 10);
    const std::vector<uint32_t> host = read_file<uint32_t>(a[1]);
    const uint32_t nb = count_of(host.size(), a[1]);
    if (q > nb) {
        fprintf(stderr, "prefix: q = %u of %u producer blocks\n", q, nb);
        return 3;
    }
    const Guarded d_counts = dev_array("counts", (size_t)nb * 4), d_cnt = dev_array("cnt", (size_t)nb * 4);
    const Guarded d_sup = dev_array("sup", (size_t)sup_words(nb) * 4, 0), d_out = dev_array("out", 4);
    upload(d_counts, host.data(), (size_t)nb * 4);
    hipStream_t st = nullptr;
    if (nb) {
        hipLaunchKernelGGL(k_publish, dim3(nb), dim3(64), 0, st, d_counts.as<uint32_t>(), d_cnt.as<uint32_t>(), d_sup.as<uint32_t>());
        finish(st);
    }
    hipLaunchKernelGGL(k_prefix, dim3(1), dim3(64), 0, st, d_cnt.as<uint32_t>(), d_sup.as<uint32_t>(), q, d_out.as<uint32_t>());
    finish(st);
    uint32_t r = 0;
    CK(hipMemcpy(&r, d_out.as<uint32_t>(), 4, hipMemcpyDeviceToHost));
    printf("prefix: %u\n", r);
    return 0;
}

// one thread per query; mode 0: out[q] = last_le, mode 1: out[q] = first_ge and out[nq + q] = first_gt, over keys[0, n)
static __global__ __launch_bounds__(256) void k_bisect(const uint64_t *__restrict__ keys, uint32_t n, const uint64_t *__restrict__ queries, uint32_t nq,
                                                       uint32_t mode, uint32_t *__restrict__ out)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= nq) return;
    const uint64_t x = queries[q];
    if (mode == 0) {
        out[q] = last_le(keys, 0u, n, x);
    } else {
        out[q] = first_ge(keys, 0u, n, x);
        out[nq + q] = first_gt(keys, 0u, n, x);
    }
}
static __global__ __launch_bounds__(256) void k_wrap(uint32_t lo, uint32_t hi, const uint32_t *__restrict__ ts, uint32_t nt, uint32_t *__restrict__ out)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= nt) return;
    const uint32_t t = ts[j];
    out[j] = first_where(lo, hi, [&](uint32_t i) { return i >= t; });
}

static int run_bisect(uint32_t mode, char **a)
{
    const std::vector<uint64_t> keys = read_file<uint64_t>(a[0]), queries = read_file<uint64_t>(a[1]);
    const uint32_t n = count_of(keys.size(), a[0]), nq = count_of(queries.size(), a[1]);
    if (nq == 0) {
        fprintf(stderr, "%s: no queries\n", mode ? "first" : "owner");
        return 3;
    }
    const size_t n_out = (size_t)nq * (mode ? 2 : 1);
    const Guarded d_keys = dev_array("keys", (size_t)n * 8), d_q = dev_array("queries", (size_t)nq * 8), d_out = dev_array("out", n_out * 4);
    upload(d_keys, keys.data(), (size_t)n * 8);
    upload(d_q, queries.data(), (size_t)nq * 8);
    hipStream_t st = nullptr;
    hipLaunchKernelGGL(k_bisect, dim3((nq + 255) / 256), dim3(256), 0, st, d_keys.as<uint64_t>(), n, d_q.as<uint64_t>(), nq, mode, d_out.as<uint32_t>());
    finish(st);
    download(a[2], d_out.as<uint32_t>(), n_out);
    return 0;
}

static int run_wrap(char **a)
{
    const uint32_t lo = (uint32_t)strtoull(a[0], nullptr, 0), hi = (uint32_t)strtoull(a[1], nullptr, 0);
    const std::vector<uint32_t> ts = read_file<uint32_t>(a[2]);
    const uint32_t nt = count_of(ts.size(), a[2]);
    if (nt == 0 || lo > hi) {
        fprintf(stderr, "wrap: %u values, [%u, %u)\n", nt, lo, hi);
        return 3;
    }
    const Guarded d_t = dev_array("t", (size_t)nt * 4), d_out = dev_array("out", (size_t)nt * 4);
    upload(d_t, ts.data(), (size_t)nt * 4);
    hipStream_t st = nullptr;
    hipLaunchKernelGGL(k_wrap, dim3((nt + 255) / 256), dim3(256), 0, st, lo, hi, d_t.as<uint32_t>(), nt, d_out.as<uint32_t>());
    finish(st);
    download(a[3], d_out.as<uint32_t>(), nt);
    return 0;
}

static int run_winbounds(char **a)
{
    const std::vector<uint64_t> off = read_file<uint64_t>(a[0]);
    const uint64_t win = strtoull(a[1], nullptr, 10);
    if (off.size() < 2 || off.back() == 0 || win == 0) {
        fprintf(stderr, "winbounds: %zu offsets, window %llu\n", off.size(), (unsigned long long)win);
        return 3;
    }
    const uint32_t n = count_of(off.size(), a[0]) - 1u;
    const uint32_t n_win = count_of((off[n] + win - 1) / win, "windows");  // (so that off[n] > (n_win - 1) * win)
    const Guarded d_off = dev_array("off", (size_t)(n + 1) * 8), d_bounds = dev_array("bounds", (size_t)n_win * 4);
    upload(d_off, off.data(), (size_t)(n + 1) * 8);
    hipStream_t st = nullptr;
    launch_win_bounds(st, d_off.as<uint64_t>(), n, win, n_win, d_bounds.as<uint32_t>());
    finish(st);
    download(a[2], d_bounds.as<uint32_t>(), n_win);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string op = argc > 1 ? argv[1] : "";
    int rc;
    if (op == "scan32" && argc == 5)
        rc = run_scan32(argv + 2);
    else if (op == "scan64" && argc == 4)
        rc = run_scan64(argv + 2);
    else if (op == "maxscan64" && argc == 4)
        rc = run_maxscan64(argv + 2);
    else if (op == "sort" && argc == 7)
        rc = run_sort(argv + 2);
    else if (op == "prefix" && argc == 4)
        rc = run_prefix(argv + 2);
    else if ((op == "owner" || op == "first") && argc == 5)
        rc = run_bisect(op == "first", argv + 2);
    else if (op == "wrap" && argc == 6)
        rc = run_wrap(argv + 2);
    else if (op == "winbounds" && argc == 5)
        rc = run_winbounds(argv + 2);
    else {
        fprintf(stderr, "usage: prim_check scan32 IN OUT TOTAL | scan64 IN OUT | maxscan64 IN OUT | sort KEY_BITS KEYS VALS KEYS_OUT VALS_OUT | prefix Q COUNTS |\n"
                        "       owner KEYS QUERIES OUT | first KEYS QUERIES OUT | wrap LO HI T OUT | winbounds OFF WIN OUT\n");
        return 3;
    }
    if (rc) return rc;
    report_guards();
    return 0;
}
