// prim_check.hip -- runs ONE of the shared primitives (ntjoin_amd/csrc/scan_kernels.h, scan64_kernels.h, sort_kernels.h) once on ONE
// input and writes what came out.  It decides nothing about right and wrong: tests/test_gpu_primitives.py computes every expected
// value.  Arrays are raw little-endian files; the element count is the file's size.
// Build: hipcc --offload-arch=gfx950 -O3 -I ntjoin_amd/csrc tools/prim_check.hip -o ntjoin_amd/bin/prim_check
// Usage: prim_check scan32 <in.u32> <out.u32> <total.u64>           launch_scan_u32 (n >= 1)
//        prim_check scan64 <in.u64> <out.u64>                       launch_scan_u64, in place (n >= 1)
//        prim_check maxscan64 <in.u64> <out.u64>                    launch_max_scan_u64, in place (n >= 1)
//        prim_check sort <key_bits> <keys.u64> <vals.u32> <keys_out.u64> <vals_out.u32>
//                                                                   launch_radix_sort; prints "buffer: <its return value>" and writes
//                                                                   the buffer that value names
//        prim_check prefix <q> <counts.u32>                         every producer block b publishes counts[b] (count_publish, sup
//                                                                   zeroed before); one wave prints "prefix: <count_prefix(q)>"
// Every device array has exactly the size its header documents, between 64 guard bytes in front and 64 behind; after the run the
// guards are read back: "guards: ok", or "guards: changed <array> ..." for every array whose guards differ.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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
    else {
        fprintf(stderr, "usage: prim_check scan32 IN OUT TOTAL | scan64 IN OUT | maxscan64 IN OUT | sort KEY_BITS KEYS VALS KEYS_OUT VALS_OUT | prefix Q COUNTS\n");
        return 3;
    }
    if (rc) return rc;
    report_guards();
    return 0;
}
