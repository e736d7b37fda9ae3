// ingest.hip -- FASTA text -> 2-bit packed bases + valid-run table ON THE DEVICE, and the TSV text of a sketch formatted
// ON THE DEVICE: the file route of the sketch stage (replaces what `indexlr` does around its hashing loop: reading the
// FASTA with `-t` threads and printing `id \t hash:pos:seq ...`, reference ntJoin:204-205, bin/ntjoin_utils.py:195-202).
//
// Why on the device: a 3 Gbp assembly is 3 GB of text in and 0.4 GB of text out.  One host core parses ~1 GB/s and formats
// ~0.4 GB/s, which made the file route 0.5 Gbp/s while the kernels run at hundreds of Gbp/s.  Here the host only
//   (1) finds the header lines (memchr for '>' over the mmap'ed file, `threads` workers),
//   (2) copies the raw text through pinned staging buffers into HBM (`threads` workers feeding hipMemcpyAsync),
//   (3) adds up ~10^6 per-tile base counts into record lengths and packed offsets,
// and the device classifies every byte (line breaks skipped, ACGTU any case = a base, anything else = an invalid base),
// packs the bases, and reports where validity changes (the run table of SURVEY.md A.3: k-mers over invalid bases do not
// exist).  The raw text stays in HBM, so the k-mer column of the TSV is printed exactly as the file spells it.
//
// A BGZF-compressed file (`bgzip`: bgzf_inflate.h) takes the same route with the compressed bytes: (2) uploads the file as it is,
// k_bgzf_inflate (bgzf.hip) writes the text into the text buffer, and since the host never sees the text, (1) is done by kernels
// here (k_hdr_*) whose header lines come back in one copy.  Plain gzip, and any file the walk or the decoder objects to, is left
// to the host parser and zlib as before.
//
// TSV: entry lengths -> exclusive scan -> every byte of the file has a known offset; the text is produced in windows of
// 64 MiB (MXG_TSV_WIN: fewer, a test knob) that leave through write_windows (win_out.hip); decimals through WinSink (text_dev.h).
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "bgzf_inflate.h"
#include "mxg_internal.h"
#include "scan_kernels.h"
#include "text_dev.h"
#include "text_index.h"

namespace mxg {

uint32_t host_threads(const mxg_handle *h)
{
    uint32_t t = h->cfg.host_threads;
    if (!t) t = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    return std::min(t, 256u);
}

// thread t of an item's block owns text bytes [tile + 16 t, tile + 16 t + 16): -> base codes (2 bits each, in order),
// validity bits, count
__device__ __forceinline__ void classify16(const unsigned char *__restrict__ text, const IngItem it, uint32_t &bits, uint32_t &valid,
                                           uint32_t &cnt)
{
    const uint64_t tile = it.lo & ~(uint64_t)(ING_TILE - 1);
    const uint64_t a0 = tile + 16u * threadIdx.x;
    bits = valid = cnt = 0;
    if (a0 + 16 <= it.lo || a0 >= it.lo + it.len) return;
    const uint4 v = *reinterpret_cast<const uint4 *>(text + a0);  // (the text buffer is padded to whole tiles)
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
        const uint64_t a = a0 + j;
        const uint32_t c = byte_class((w[j >> 2] >> (8u * (j & 3u))) & 255u);
        if (a >= it.lo && a < it.lo + it.len && c != 5u) {
            bits |= (c & 3u) << (2u * cnt);
            valid |= (c < 4u ? 1u : 0u) << cnt;
            ++cnt;
        }
    }
}

__global__ __launch_bounds__(256) void k_ing_count(const unsigned char *__restrict__ text, const IngItem *__restrict__ items,
                                                   uint32_t *__restrict__ item_cnt, uint16_t *__restrict__ item_sub)
{
    __shared__ uint32_t tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    uint32_t bits, valid, cnt;
    classify16(text, items[blockIdx.x], bits, valid, cnt);
    uint32_t s = cnt;  // sum over the 16 threads of a 256-byte sub-tile
    s += (uint32_t)__shfl_xor((int)s, 8, 64);
    s += (uint32_t)__shfl_xor((int)s, 4, 64);
    s += (uint32_t)__shfl_xor((int)s, 2, 64);
    s += (uint32_t)__shfl_xor((int)s, 1, 64);
    if ((threadIdx.x & 15u) == 0) {
        item_sub[(size_t)blockIdx.x * 16u + (threadIdx.x >> 4)] = (uint16_t)s;
        if (s) atomicAdd(&tot, s);
    }
    __syncthreads();
    if (threadIdx.x == 0) item_cnt[blockIdx.x] = tot;
}

struct IngEvent {
    uint64_t at;     // packed base index where validity changes
    uint32_t state;  // new state: 1 = valid
    uint32_t item;
};

__global__ __launch_bounds__(256) void k_ing_pack(const unsigned char *__restrict__ text, const IngItem *__restrict__ items,
                                                  const uint64_t *__restrict__ item_pbase, uint32_t *__restrict__ packed,
                                                  uint8_t *__restrict__ first_valid, uint8_t *__restrict__ last_valid,
                                                  IngEvent *__restrict__ events, uint32_t ev_cap, uint32_t *__restrict__ ev_count)
{
    __shared__ uint32_t sh[256];
    __shared__ uint32_t vb[ING_TILE / 32 + 1];  // validity of the item's bases by local index
    const IngItem it = items[blockIdx.x];
    uint32_t bits, valid, cnt;
    classify16(text, it, bits, valid, cnt);
    if (threadIdx.x <= ING_TILE / 32) vb[threadIdx.x] = 0;
    const bool all_ok = __syncthreads_and(valid == (cnt ? (0xFFFFFFFFu >> (32u - cnt)) : 0u)) != 0;
    const uint32_t l0 = block_exclusive_256(cnt, sh);
    const uint32_t total = sh[255];
    const uint64_t pbase = item_pbase[blockIdx.x];
    if (cnt) {
        const uint64_t g = pbase + l0;
        const uint64_t v = (uint64_t)bits << (2u * ((uint32_t)g & 15u));
        atomicOr(&packed[g >> 4], (uint32_t)v);
        if (v >> 32) atomicOr(&packed[(g >> 4) + 1], (uint32_t)(v >> 32));
    }
    if (all_ok) {  // (block-uniform) the common case: nothing but ACGTU in this tile
        if (threadIdx.x == 0) first_valid[blockIdx.x] = last_valid[blockIdx.x] = total ? 1 : 2;
        return;
    }
    if (cnt) {
        const uint64_t m = (uint64_t)valid << (l0 & 31u);
        atomicOr(&vb[l0 >> 5], (uint32_t)m);
        if (m >> 32) atomicOr(&vb[(l0 >> 5) + 1], (uint32_t)(m >> 32));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        first_valid[blockIdx.x] = total ? (uint8_t)(vb[0] & 1u) : 2;
        last_valid[blockIdx.x] = total ? (uint8_t)((vb[(total - 1) >> 5] >> ((total - 1) & 31u)) & 1u) : 2;
    }
    for (uint32_t u = 0; u < cnt; ++u) {
        const uint32_t i = l0 + u;
        if (i == 0) continue;  // (the host compares an item's first base with the item before it)
        const uint32_t cur = (vb[i >> 5] >> (i & 31u)) & 1u, prev = (vb[(i - 1) >> 5] >> ((i - 1) & 31u)) & 1u;
        if (cur != prev) {
            const uint32_t e = atomicAdd(ev_count, 1u);
            if (e < ev_cap) events[e] = IngEvent{pbase + i, cur, blockIdx.x};
        }
    }
}

static std::string header_token(const unsigned char *p, size_t n)
{
    size_t e = 0;
    while (e < n && p[e] != ' ' && p[e] != '\t' && p[e] != '\r' && p[e] != '\n') ++e;
    return std::string(reinterpret_cast<const char *>(p), e);
}

template <class F> static void parallel_for(uint32_t n_threads, F f)
{
    std::vector<std::thread> th;
    for (uint32_t t = 1; t < n_threads; ++t) th.emplace_back(f, t);
    f(0u);
    for (auto &x : th) x.join();
}

// ---- header lines found on the device (the BGZF route: the text exists only in HBM) ----
// thread t of a block owns text bytes [4096 b + 16 t, + 16): bit j set = byte j is a '>' at the start of a line
__device__ __forceinline__ uint32_t hdr_flags16(const unsigned char *__restrict__ text, uint64_t n)
{
    const uint64_t a0 = (uint64_t)blockIdx.x * ING_TILE + 16u * threadIdx.x;
    if (a0 >= n) return 0u;
    const uint4 v = *reinterpret_cast<const uint4 *>(text + a0);  // (the text buffer is padded to whole tiles)
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t prev = a0 ? text[a0 - 1] : (uint32_t)'\n', f = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
        const uint32_t c = (w[j >> 2] >> (8u * (j & 3u))) & 255u;
        if (c == (uint32_t)'>' && prev == (uint32_t)'\n' && a0 + j < n) f |= 1u << j;
        prev = c;
    }
    return f;
}
__global__ __launch_bounds__(256) void k_hdr_count(const unsigned char *__restrict__ text, uint64_t n, uint32_t *__restrict__ bsum)
{
    __shared__ uint32_t sh[256];
    (void)block_exclusive_256((uint32_t)__popc(hdr_flags16(text, n)), sh);
    if (threadIdx.x == 0) bsum[blockIdx.x] = sh[255];
}
// bsum: exclusive scan of the counts (k_scan_sums) -> the positions in text order
__global__ __launch_bounds__(256) void k_hdr_emit(const unsigned char *__restrict__ text, uint64_t n, const uint32_t *__restrict__ bsum,
                                                  uint64_t n_hdr, uint64_t *__restrict__ at)
{
    __shared__ uint32_t sh[256];
    uint32_t f = hdr_flags16(text, n);
    uint64_t i = (uint64_t)bsum[blockIdx.x] + block_exclusive_256((uint32_t)__popc(f), sh);
    const uint64_t a0 = (uint64_t)blockIdx.x * ING_TILE + 16u * threadIdx.x;
    while (f) {
        const uint32_t j = (uint32_t)__ffs((int)f) - 1u;
        f &= f - 1u;
        if (i < n_hdr) at[i] = a0 + j;
        ++i;
    }
}
// one thread per header line: its '\n' (or the text's end)
__global__ __launch_bounds__(256) void k_hdr_end(const unsigned char *__restrict__ text, uint64_t n, const uint64_t *__restrict__ at, uint64_t n_hdr,
                                                 uint64_t *__restrict__ end)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_hdr) return;
    uint64_t p = at[i] + 1;
    while (p < n && text[p] != '\n') ++p;
    end[i] = p;
}
// ... and its bytes behind the '>' into one buffer, line i at off[i]
__global__ __launch_bounds__(256) void k_hdr_gather(const unsigned char *__restrict__ text, const uint64_t *__restrict__ at,
                                                    const uint64_t *__restrict__ end, const uint64_t *__restrict__ off, uint64_t n_hdr,
                                                    unsigned char *__restrict__ lines)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_hdr) return;
    const uint64_t lo = at[i] + 1, len = end[i] - lo, o = off[i];
    for (uint64_t u = 0; u < len; ++u) lines[o + u] = text[lo + u];
}

struct Hdr {
    uint64_t at, end;  // '>' and its line's '\n' (or the text's end)
};

// a device allocation that failed for want of room: "not for this route" where another route exists
static bool soft_alloc_failure(hipError_t e)
{
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation;
}

// The header lines of a text that lies in HBM (padded to whole tiles), in three steps so that a caller can put work of its own in
// front of the first sync: hdr_scan_alloc; hdr_scan_count enqueues the count and its scan (n_hdr is there once `st` is synchronised,
// which is the caller's to do); hdr_scan_lines brings the lines back (hdr; line r's bytes behind its '>' are lines[line_off[r] ...]).
struct HdrScan {
    DevBuf d_bsum, d_total, d_at, d_end, d_off, d_lines;  // (scratch of one call: freed with the struct)
    uint64_t n_tiles = 0, n_hdr = 0;
};
static hipError_t hdr_scan_alloc(HdrScan &s, uint64_t usz)  // usz below 2^31 tiles
{
    s.n_tiles = (usz + ING_TILE - 1) / ING_TILE;
    hipError_t e = s.d_bsum.ensure(s.n_tiles * 4);
    return e != hipSuccess ? e : s.d_total.ensure(16);
}
static int hdr_scan_count(mxg_handle *h, HdrScan &s, const unsigned char *d_text, uint64_t usz, hipStream_t st)
{
    hipLaunchKernelGGL(k_hdr_count, dim3((uint32_t)s.n_tiles), dim3(256), 0, st, d_text, usz, s.d_bsum.as<uint32_t>());
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(256), 0, st, s.d_bsum.as<uint32_t>(), (uint32_t)s.n_tiles, s.d_total.as<uint64_t>());
    MXG_HIP(h, hipGetLastError());
    MXG_HIP(h, hipMemcpyAsync(&s.n_hdr, s.d_total.p, 8, hipMemcpyDeviceToHost, st));
    return MXG_OK;
}
static int hdr_scan_lines(mxg_handle *h, const char *path, HdrScan &s, const unsigned char *d_text, uint64_t usz, hipStream_t st,
                          std::vector<Hdr> &hdr, std::vector<unsigned char> &lines, std::vector<uint64_t> &line_off);

// The BGZF route between the upload and the work items: the members inflated into d_text, the header lines found there and brought
// back.  MXG_OK, a negative error, or 1: a member's data or CRC is not in order (the host parser and zlib then say what is wrong
// with the file), or no room on the device (the host parser takes the file).
static int bgzf_text_and_headers(mxg_handle *h, const char *path, const BgzfPlan &plan, const unsigned char *d_comp, uint64_t comp_bytes,
                                 unsigned char *d_text, hipStream_t st, bool dbg_io, std::vector<Hdr> &hdr, std::vector<unsigned char> &lines,
                                 std::vector<uint64_t> &line_off)
{
    auto now_s = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now_s();
    const uint64_t usz = plan.usz;
    const size_t n_mem = plan.members.size();
    if (n_mem >= (1ull << 31)) return 1;
    DevBuf d_mem, d_status;  // (scratch of this call: freed when it returns)
    HdrScan scan;
    hipError_t e;
    if ((usz + ING_TILE - 1) / ING_TILE >= (1ull << 31)) return 1;
    if ((e = d_mem.ensure(n_mem * sizeof(BgzfMember))) != hipSuccess || (e = d_status.ensure((n_mem + 1) * 4)) != hipSuccess ||
        (e = hdr_scan_alloc(scan, usz)) != hipSuccess)
        return soft_alloc_failure(e) ? 1 : set_err(h, MXG_EDEVICE, "device allocation failed: %s", hipGetErrorString(e));
    MXG_HIP(h, hipMemcpyAsync(d_mem.p, plan.members.data(), n_mem * sizeof(BgzfMember), hipMemcpyHostToDevice, st));
    int rc = bgzf_inflate_device(h, d_comp, comp_bytes, d_mem.as<BgzfMember>(), (uint32_t)n_mem, d_text, usz, d_status.as<uint32_t>(), st);
    if (rc != MXG_OK) return rc;
    uint32_t fail = 0;
    MXG_HIP(h, hipMemcpyAsync(&fail, d_status.p, 4, hipMemcpyDeviceToHost, st));
    // (the header count does not wait for the verdict: a member that failed left bytes inside its own range of the text, no more)
    if ((rc = hdr_scan_count(h, scan, d_text, usz, st)) != MXG_OK) return rc;
    MXG_HIP(h, hipStreamSynchronize(st));
    const double t_inf = now_s() - t0;  // (the kernel and, beside it, one pass over the text)
    if (fail != 0) return 1;
    if (dbg_io)
        fprintf(stderr, "[mxg] bgzf_inflate members=%llu bytes_in=%llu bytes_out=%llu ms=%.3f\n", (unsigned long long)n_mem,
                (unsigned long long)comp_bytes, (unsigned long long)usz, t_inf * 1e3);
    return hdr_scan_lines(h, path, scan, d_text, usz, st, hdr, lines, line_off);
}

static int hdr_scan_lines(mxg_handle *h, const char *path, HdrScan &s, const unsigned char *d_text, uint64_t usz, hipStream_t st,
                          std::vector<Hdr> &hdr, std::vector<unsigned char> &lines, std::vector<uint64_t> &line_off)
{
    DevBuf &d_bsum = s.d_bsum, &d_at = s.d_at, &d_end = s.d_end, &d_off = s.d_off, &d_lines = s.d_lines;
    const uint64_t n_hdr = s.n_hdr, n_tiles = s.n_tiles;
    auto soft = soft_alloc_failure;
    hipError_t e;
    if (n_hdr >= (1ull << 32)) return set_err(h, MXG_ELIMIT, "too many records in '%s'", path);
    hdr.resize(n_hdr);
    line_off.assign(n_hdr + 1, 0);
    if (!n_hdr) return MXG_OK;
    if ((e = d_at.ensure(n_hdr * 8)) != hipSuccess || (e = d_end.ensure(n_hdr * 8)) != hipSuccess || (e = d_off.ensure(n_hdr * 8)) != hipSuccess)
        return soft(e) ? 1 : set_err(h, MXG_EDEVICE, "device allocation failed: %s", hipGetErrorString(e));
    const uint32_t hb = (uint32_t)((n_hdr + 255) / 256);
    hipLaunchKernelGGL(k_hdr_emit, dim3((uint32_t)n_tiles), dim3(256), 0, st, d_text, usz, d_bsum.as<uint32_t>(), n_hdr, d_at.as<uint64_t>());
    hipLaunchKernelGGL(k_hdr_end, dim3(hb), dim3(256), 0, st, d_text, usz, d_at.as<uint64_t>(), n_hdr, d_end.as<uint64_t>());
    MXG_HIP(h, hipGetLastError());
    std::vector<uint64_t> at(n_hdr), end(n_hdr);
    MXG_HIP(h, hipMemcpyAsync(at.data(), d_at.p, n_hdr * 8, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipMemcpyAsync(end.data(), d_end.p, n_hdr * 8, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    for (uint64_t r = 0; r < n_hdr; ++r) {
        if (at[r] >= usz || end[r] <= at[r] || end[r] > usz || (r && at[r] <= end[r - 1]))
            return set_err(h, MXG_EDEVICE, "internal error: header lines of '%s' out of order", path);
        hdr[r] = Hdr{at[r], end[r]};
        line_off[r + 1] = line_off[r] + (end[r] - at[r] - 1);
    }
    lines.resize(line_off[n_hdr]);
    if (!lines.empty()) {
        if ((e = d_lines.ensure(lines.size())) != hipSuccess)
            return soft(e) ? 1 : set_err(h, MXG_EDEVICE, "device allocation failed: %s", hipGetErrorString(e));
        MXG_HIP(h, hipMemcpyAsync(d_off.p, line_off.data(), n_hdr * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_hdr_gather, dim3(hb), dim3(256), 0, st, d_text, d_at.as<uint64_t>(), d_end.as<uint64_t>(), d_off.as<uint64_t>(), n_hdr,
                           d_lines.as<unsigned char>());
        MXG_HIP(h, hipGetLastError());
        MXG_HIP(h, hipMemcpyAsync(lines.data(), d_lines.p, lines.size(), hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
    }
    return MXG_OK;
}

struct IngestTimes {  // MXG_DEBUG_IO: seconds since t0 at which ingest_text's phases ended
    double t0 = 0, hdr = 0, up = 0, count = 0, pack = 0;
};
enum class IngestRefusal { None, NoRoom, Events };  // why ingest_text answered "not for this route"
static int ingest_text(mxg_handle *h, Assembly *a, const char *path, const std::vector<Hdr> &hdr, const unsigned char *txt,
                       const std::vector<unsigned char> &hdr_lines, const std::vector<uint64_t> &hdr_line_off, uint64_t tsz, unsigned char *d_text,
                       const std::function<int()> &text_ready, IngestTimes &tp, IngestRefusal &why);
static void drop_device_text_if_asked(mxg_handle *h, Assembly *a);

// returns MXG_OK, a negative error, or 1: "not for this route" (the caller falls back to the host parser)
int load_fasta_device(mxg_handle *h, Assembly *a, const char *path, uint32_t n_threads)
{
    n_threads = std::max(1u, std::min(n_threads, 64u));
    const bool dbg_io = getenv("MXG_DEBUG_IO") != nullptr;  // phase timings on stderr
    auto now_s = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tp0 = now_s();
    double tp_alloc = 0, tp_pool = 0;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return set_err(h, MXG_EIO, "cannot open FASTA '%s'", path);
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {  // pipes etc.: the streaming host parser
        close(fd);
        return 1;
    }
    const uint64_t fsz = (uint64_t)sb.st_size;
    unsigned char magic[2] = {0, 0};
    const bool gz = fsz >= 2 && pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
    if (fsz == 0) {  // (the host parser produces the empty assembly)
        close(fd);
        return 1;
    }
    const unsigned char *txt = static_cast<const unsigned char *>(mmap(nullptr, fsz, PROT_READ, MAP_PRIVATE, fd, 0));
    close(fd);
    if (txt == MAP_FAILED) return 1;
    (void)madvise(const_cast<unsigned char *>(txt), fsz, MADV_SEQUENTIAL);
    // (taking a 3 GB mapping apart costs ~25 ms: a handle that runs once -- MXG_FLAG_ONE_SHOT, the CLI -- leaves it to
    // mxg_destroy or, as mxgraph does, to the end of a process nobody waits for)
    struct Unmap {
        const unsigned char *p;
        uint64_t n;
        mxg_handle *keep;
        ~Unmap()
        {
            if (keep) {
                try {
                    keep->kept_maps.emplace_back(const_cast<unsigned char *>(p), (size_t)n);
                    return;
                } catch (...) {
                }
            }
            munmap(const_cast<unsigned char *>(p), n);
        }
    } unmap{txt, fsz, (h->cfg.flags & MXG_FLAG_ONE_SHOT) && !getenv("MXG_UNMAP_EARLY") ? h : nullptr};
    // gzip magic: a chain of BGZF members is inflated on the device (the file below = the compressed bytes, the text = what the
    // trailers add up to); plain gzip, a mixed file, a walk that misses the file's end, no text at all: the host parser and zlib
    BgzfPlan plan;
    const bool bgzf = gz;
    if (gz && (!bgzf_plan(txt, fsz, plan) || plan.usz == 0)) {
        unmap.keep = nullptr;
        return 1;
    }
    const uint64_t tsz = bgzf ? plan.usz : fsz;  // bytes of text
    MXG_HIP(h, hipSetDevice(h->device));

    // ---- (2) raw text -> HBM through pinned staging buffers, started first so that it overlaps the header scan ----
    // A device allocation that fails here (the route keeps ~1 byte per base of text in HBM) is no error: the host parser
    // takes the file instead (return 1; nothing has been committed to `a` that the caller's delete / new does not undo).
    auto dev_fallback = soft_alloc_failure;
    const uint64_t text_alloc = ((tsz + ING_TILE - 1) / ING_TILE + 1) * ING_TILE;
    DevBuf d_comp;  // BGZF: the file's bytes, released as soon as the text is inflated (whole words: the decoder fetches aligned words)
    {
        hipError_t e = a->d_text.ensure(text_alloc);
        if (e == hipSuccess && bgzf) e = d_comp.ensure((fsz + 3) & ~3ull);
        if (e != hipSuccess) return dev_fallback(e) ? 1 : set_err(h, MXG_EDEVICE, "device allocation failed: %s", hipGetErrorString(e));
    }
    unsigned char *d_text = a->d_text.as<unsigned char>();
    unsigned char *d_up = bgzf ? d_comp.as<unsigned char>() : d_text;  // where the file's bytes go
    tp_alloc = now_s() - tp0;
    constexpr uint64_t STAGE = 32ull << 20;
    constexpr int NB = 4;
    // staging resources + the uploader thread: joined and released on every way out of this function (an exception thrown
    // by the host-side section below must not unwind through a joinable std::thread)
    struct Staging {
        unsigned char *buf[NB] = {nullptr, nullptr, nullptr, nullptr};
        hipEvent_t ev[NB] = {nullptr, nullptr, nullptr, nullptr};
        hipStream_t cs = nullptr;
        std::thread uploader;
        void finish()
        {
            if (uploader.joinable()) uploader.join();
        }
        ~Staging()
        {
            finish();
            for (int b = 0; b < NB; ++b)
                if (ev[b]) (void)hipEventDestroy(ev[b]);  // (the buffers are the handle's: pin_pool)
            if (cs) (void)hipStreamDestroy(cs);
        }
    } sg;
    unsigned char **stage = sg.buf;
    hipEvent_t *sev = sg.ev;
    MXG_HIP(h, hipStreamCreateWithFlags(&sg.cs, hipStreamNonBlocking));
    hipStream_t cs = sg.cs;
    static_assert(NB * STAGE <= PIN_POOL_BYTES, "staging buffers come out of the handle's pinned pool");
    {
        // (the pool is pinned piece by piece by a thread of the handle; a staging buffer = a piece: the upload starts with the first)
        static_assert(STAGE == PIN_PIECE_BYTES && NB <= (int)PIN_PIECES, "a staging buffer is one piece of the pinned pool");
        hipError_t e = pin_pool_start(h);
        if (e == hipSuccess) e = pin_pool_wait(h, 1);
        if (e != hipSuccess && (e = pin_pool_start(h)) == hipSuccess) e = pin_pool_wait(h, 1);  // (registering failed: one allocation)
        if (e != hipSuccess) return dev_fallback(e) ? 1 : set_err(h, MXG_EDEVICE, "pinned allocation failed: %s", hipGetErrorString(e));
        unsigned char *pool = static_cast<unsigned char *>(h->pin_pool);
        tp_pool = now_s() - tp0;
        for (int b = 0; b < NB; ++b) {
            stage[b] = pool + (size_t)b * STAGE;
            MXG_HIP(h, hipEventCreateWithFlags(&sev[b], hipEventDisableTiming));
        }
    }
    hipError_t uerr = hipSuccess;
    sg.uploader = std::thread([&]() {
        (void)hipSetDevice(h->device);
        const uint32_t T = std::max(1u, n_threads - 1u);
        uint64_t c = 0;
        uint32_t ring = NB;  // staging buffers in use: all of them, unless pinning stopped part of the way (then what is pinned: >= 1)
        bool used[NB] = {false, false, false, false};
        for (uint64_t off = 0; off < fsz && uerr == hipSuccess; off += STAGE, ++c) {
            if (c < ring && pin_pool_wait(h, (uint32_t)c + 1u) != hipSuccess)  // (its piece of the pool may still be on its way)
                ring = std::max(1u, std::min((uint32_t)c, h->pin_ready.load()));
            const int b = (int)(c % ring);
            if (used[b]) uerr = hipEventSynchronize(sev[b]);
            used[b] = true;
            if (uerr != hipSuccess) break;
            const uint64_t n = std::min(STAGE, fsz - off);
            try {
                parallel_for(T, [&](uint32_t t) {
                    const uint64_t lo = n * t / T, hi = n * (t + 1) / T;
                    memcpy(stage[b] + lo, txt + off + lo, hi - lo);
                });
            } catch (const std::exception &) {  // (no thread to be had: copy alone)
                memcpy(stage[b], txt + off, n);
            }
            if (uerr == hipSuccess) uerr = hipMemcpyAsync(d_up + off, stage[b], n, hipMemcpyHostToDevice, cs);
            if (uerr == hipSuccess) uerr = hipEventRecord(sev[b], cs);
        }
        if (uerr == hipSuccess) uerr = hipMemsetAsync(d_text + tsz, '\n', text_alloc - tsz, cs);
        if (uerr == hipSuccess) uerr = hipStreamSynchronize(cs);
    });

    // ---- (1) header lines: '>' at the start of a line ----
    std::vector<Hdr> hdr;
    std::vector<unsigned char> hdr_lines;  // BGZF: the header lines' bytes as the device gathered them
    std::vector<uint64_t> hdr_line_off;
    double tp_bgzf = 0;
    if (bgzf) {  // (the text has to be there first: upload, inflate, then the header lines by kernels)
        sg.finish();
        if (uerr != hipSuccess) return set_err(h, MXG_EDEVICE, "text upload failed: %s", hipGetErrorString(uerr));
        tp_bgzf = now_s() - tp0;
        const int brc = bgzf_text_and_headers(h, path, plan, d_comp.as<unsigned char>(), fsz, d_text, h->stream, dbg_io, hdr, hdr_lines, hdr_line_off);
        if (brc != MXG_OK) {
            if (brc == 1) unmap.keep = nullptr;
            return brc;
        }
        d_comp.release();
    }
    std::vector<std::vector<Hdr>> found(bgzf ? 0 : n_threads);
    if (!bgzf) parallel_for(n_threads, [&](uint32_t t) {
        const uint64_t lo = fsz * t / n_threads, hi = fsz * (t + 1) / n_threads;
        uint64_t p = lo;
        while (p < hi) {
            const unsigned char *q = static_cast<const unsigned char *>(memchr(txt + p, '>', hi - p));
            if (!q) break;
            const uint64_t at = (uint64_t)(q - txt);
            if (at == 0 || txt[at - 1] == '\n') {
                const unsigned char *nl = static_cast<const unsigned char *>(memchr(q, '\n', fsz - at));
                const uint64_t end = nl ? (uint64_t)(nl - txt) : fsz;
                found[t].push_back(Hdr{at, end});
                p = end + 1;  // (a '>' inside the header line is not a header)
            } else {
                p = at + 1;
            }
        }
    });
    for (auto &v : found)
        for (auto &x : v)
            if (hdr.empty() || x.at > hdr.back().end) hdr.push_back(x);  // (a chunk border inside a header line)
    IngestTimes tp;
    tp.t0 = tp0;
    IngestRefusal why = IngestRefusal::None;
    const int rc = ingest_text(h, a, path, hdr, bgzf ? nullptr : txt, hdr_lines, hdr_line_off, tsz, d_text, [&]() {
        sg.finish();  // the text is in HBM
        tp.up = now_s() - tp0;
        return uerr == hipSuccess ? MXG_OK : set_err(h, MXG_EDEVICE, "text upload failed: %s", hipGetErrorString(uerr));
    }, tp, why);
    if (rc != MXG_OK) return rc;
    a->from_bgzf = bgzf;
    for (const BgzfMember &m : plan.members) {
        a->bgzf_comp_off.push_back(m.in_off - m.head);
        a->bgzf_text_off.push_back(m.out_off);
    }
    if (dbg_io)
        fprintf(stderr, "[mxg] load_fasta_device %s: %.3f s = open + map + text buffer %.3f, first pinned buffer at %.3f, headers + items (beside the "
                        "upload) until %.3f, upload done at %.3f, base counts at %.3f, packed at %.3f, run table at %.3f (%.2f GB)\n", path, now_s() - tp0,
                tp_alloc, tp_pool, tp.hdr, bgzf ? tp_bgzf : tp.up, tp.count, tp.pack, now_s() - tp0, tsz / 1e9);
    drop_device_text_if_asked(h, a);
    return rc;
}

// Everything behind the header lines, for a text that is (or is about to be) in HBM at d_text, padded with '\n' to whole tiles plus
// one: the work items, the base counts, record lengths and the packed layout, the packed bases, the run table.  Header line r is
// txt[hdr[r].at + 1 .. hdr[r].end) where the host has the text, else hdr_lines[hdr_line_off[r] ...].  text_ready is called once,
// after the items are on their way and before the first kernel reads the text.  MXG_OK, a negative error, or 1: "not for this
// route" (why says which limit it was).
static int ingest_text(mxg_handle *h, Assembly *a, const char *path, const std::vector<Hdr> &hdr, const unsigned char *txt,
                       const std::vector<unsigned char> &hdr_lines, const std::vector<uint64_t> &hdr_line_off, uint64_t tsz, unsigned char *d_text,
                       const std::function<int()> &text_ready, IngestTimes &tp, IngestRefusal &why)
{
    const uint32_t k = h->cfg.k, w = h->cfg.w;
    auto now_s = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tp0 = tp.t0;
    auto dev_fallback = [&](hipError_t e) {
        why = IngestRefusal::NoRoom;
        return soft_alloc_failure(e);
    };
    const size_t n_rec = hdr.size();
    if (n_rec >= (1ull << 32)) return set_err(h, MXG_ELIMIT, "too many records in '%s'", path);
    // ---- work items: the tiles every record's sequence text overlaps ----
    std::vector<IngItem> items;
    std::vector<uint64_t> rec_item0(n_rec + 1);
    a->recs.resize(n_rec);
    for (size_t r = 0; r < n_rec; ++r) {
        const uint64_t sb0 = std::min(hdr[r].end + 1, tsz), se = r + 1 < n_rec ? hdr[r + 1].at : tsz;
        a->recs[r].id = header_token(txt ? txt + hdr[r].at + 1 : hdr_lines.data() + hdr_line_off[r], hdr[r].end - hdr[r].at - 1);
        a->recs[r].text_off = sb0;
        rec_item0[r] = items.size();
        for (uint64_t p = sb0; p < se;) {
            const uint64_t tile_end = (p / ING_TILE + 1) * ING_TILE, e = std::min(se, tile_end);
            items.push_back(IngItem{p, (uint32_t)(e - p), (uint32_t)r});
            p = e;
        }
    }
    rec_item0[n_rec] = items.size();
    const size_t n_items = items.size();
    if (n_items >= (1ull << 31)) return set_err(h, MXG_ELIMIT, "'%s' is too large for one handle", path);
    hipStream_t st = h->stream;
    DevBuf &d_items = a->d_ing_items, &d_cnt = a->d_ing_cnt, &d_sub = a->d_ing_sub, &d_pbase = a->d_ing_pbase;
    int rc = MXG_OK;
    if (n_items) {
        hipError_t e;
        if ((e = d_items.ensure(n_items * sizeof(IngItem))) != hipSuccess || (e = d_cnt.ensure(n_items * 4)) != hipSuccess ||
            (e = d_sub.ensure(n_items * 32)) != hipSuccess || (e = d_pbase.ensure(n_items * 8)) != hipSuccess)
            return dev_fallback(e) ? 1 : set_err(h, MXG_EDEVICE, "device allocation failed: %s", hipGetErrorString(e));
        if ((e = hipMemcpyAsync(d_items.p, items.data(), n_items * sizeof(IngItem), hipMemcpyHostToDevice, st)) != hipSuccess)
            return set_err(h, MXG_EDEVICE, "upload failed: %s", hipGetErrorString(e));
    }
    tp.hdr = now_s() - tp0;
    if ((rc = text_ready()) != MXG_OK) return rc;
    std::vector<uint32_t> cnt(n_items);
    if (n_items) {
        hipLaunchKernelGGL(k_ing_count, dim3((uint32_t)n_items), dim3(256), 0, st, d_text, d_items.as<IngItem>(), d_cnt.as<uint32_t>(),
                           d_sub.as<uint16_t>());
        MXG_HIP(h, hipGetLastError());
        MXG_HIP(h, hipMemcpyAsync(cnt.data(), d_cnt.p, n_items * 4, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
    }
    tp.count = now_s() - tp0;
    // ---- (3) record lengths, packed layout (every record starts at a multiple of 16 bases) ----
    std::vector<uint64_t> pbase(n_items);
    uint64_t cur = 0;
    for (size_t r = 0; r < n_rec; ++r) {
        Record &rec = a->recs[r];
        rec.base_off = cur;
        uint64_t len = 0;
        for (uint64_t q = rec_item0[r]; q < rec_item0[r + 1]; ++q) {
            pbase[q] = cur + len;
            len += cnt[q];
        }
        rec.len = len;
        if (len >= (1ull << 32))
            return set_err(h, MXG_ELIMIT, "record '%s' has %llu bases; the engine indexes positions with 32 bits", rec.id.c_str(),
                           (unsigned long long)len);
        a->total_bases += len;
        cur += (len + 15) & ~15ull;
    }
    const size_t pad = 256 + (k + 15) / 16 + 16;  // the hash kernel reads up to one strip + k bases past a run's end
    a->packed_words = cur / 16 + pad;
    {
        const hipError_t e = a->d_packed_own.ensure(a->packed_words * 4);
        if (e != hipSuccess) return dev_fallback(e) ? 1 : set_err(h, MXG_EDEVICE, "device allocation failed: %s", hipGetErrorString(e));
    }
    MXG_HIP(h, hipMemsetAsync(a->d_packed_own.p, 0, a->packed_words * 4, st));
    // changes between valid and invalid bases inside the tiles; MXG_INGEST_EV_CAP: test knob
    const uint32_t EV_CAP = (uint32_t)std::max<uint64_t>(1, knob_u64(h, "MXG_INGEST_EV_CAP", 4u << 20));
    std::vector<uint8_t> fv(n_items), lv(n_items);
    std::vector<IngEvent> events;
    if (n_items) {
        DevBuf d_fv, d_lv, d_ev, d_evn;
        MXG_HIP(h, d_fv.ensure(n_items));
        MXG_HIP(h, d_lv.ensure(n_items));
        MXG_HIP(h, d_ev.ensure((size_t)EV_CAP * sizeof(IngEvent)));
        MXG_HIP(h, d_evn.ensure(16));
        MXG_HIP(h, hipMemsetAsync(d_evn.p, 0, 16, st));
        MXG_HIP(h, hipMemcpyAsync(d_pbase.p, pbase.data(), n_items * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_ing_pack, dim3((uint32_t)n_items), dim3(256), 0, st, d_text, d_items.as<IngItem>(), d_pbase.as<uint64_t>(),
                           a->d_packed_own.as<uint32_t>(), d_fv.as<uint8_t>(), d_lv.as<uint8_t>(), d_ev.as<IngEvent>(), EV_CAP,
                           d_evn.as<uint32_t>());
        MXG_HIP(h, hipGetLastError());
        uint32_t n_ev = 0;
        MXG_HIP(h, hipMemcpyAsync(fv.data(), d_fv.p, n_items, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipMemcpyAsync(lv.data(), d_lv.p, n_items, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipMemcpyAsync(&n_ev, d_evn.p, 4, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
        // more changes than the buffer holds (drafts with scattered N / IUPAC codes): the host parser has no such limit
        if (n_ev > EV_CAP) {
            why = IngestRefusal::Events;
            return 1;
        }
        events.resize(n_ev);
        if (n_ev) {
            MXG_HIP(h, hipMemcpy(events.data(), d_ev.p, (size_t)n_ev * sizeof(IngEvent), hipMemcpyDeviceToHost));
            std::sort(events.begin(), events.end(), [](const IngEvent &x, const IngEvent &y) { return x.at < y.at; });
        }
    }
    a->d_packed = a->d_packed_own.as<uint32_t>();
    tp.pack = now_s() - tp0;
    // ---- the run table: maximal stretches of valid bases holding at least one k-mer ----
    size_t ev_i = 0;
    for (size_t r = 0; r < n_rec; ++r) {
        const Record &rec = a->recs[r];
        std::vector<std::pair<uint32_t, uint32_t>> rec_runs;  // (pos0, n_kmers)
        uint32_t state = 0;
        uint64_t run_start = 0, inv_start = 0;
        auto flip = [&](uint64_t at_rel, uint32_t to) {
            if (to == state) return;
            if (to && at_rel > inv_start) a->inv.emplace_back(rec.base_off + inv_start, rec.base_off + at_rel);
            if (!to) inv_start = at_rel;
            if (to) run_start = at_rel;
            else if (at_rel - run_start >= k) rec_runs.emplace_back((uint32_t)run_start, (uint32_t)(at_rel - run_start - k + 1));
            state = to;
        };
        for (uint64_t q = rec_item0[r]; q < rec_item0[r + 1]; ++q) {
            if (fv[q] == 2) continue;  // no base in this tile
            flip(pbase[q] - rec.base_off, fv[q]);
            while (ev_i < events.size() && events[ev_i].item < q) ++ev_i;  // (cannot happen: events are in item order)
            while (ev_i < events.size() && events[ev_i].item == q) {
                flip(events[ev_i].at - rec.base_off, events[ev_i].state);
                ++ev_i;
            }
            // (the tile's last state follows from its events; lv[] is only a cross-check)
            if (state != lv[q]) return set_err(h, MXG_EDEVICE, "internal error: validity tracking out of step in '%s'", path);
        }
        flip(rec.len, 0);
        if (rec.len > inv_start) a->inv.emplace_back(rec.base_off + inv_start, rec.base_off + rec.len);
        uint64_t nk = 0;
        for (auto &rr : rec_runs) nk += rr.second;
        if (nk >= w && nk > 0) {
            const uint32_t ctg = (uint32_t)a->ctg_rec.size();
            a->ctg_rec.push_back((uint32_t)r);
            a->ctg_nk.push_back((uint32_t)nk);
            a->ctg_run0.push_back((uint32_t)a->runs.size());
            uint32_t kidx = 0;
            for (auto &rr : rec_runs) {
                Run run;
                run.base_off = rec.base_off + rr.first;
                run.n_kmers = rr.second;
                run.contig = ctg;
                run.kidx0 = kidx;
                run.pos0 = rr.first;
                kidx += rr.second;
                a->runs.push_back(run);
            }
            a->total_kmers += nk;
        }
    }
    a->ctg_run0.push_back((uint32_t)a->runs.size());
    a->has_bases = true;
    a->has_text = false;
    a->text_on_device = true;
    a->text_bytes = tsz;
    a->ing_item0.assign(rec_item0.begin(), rec_item0.end());
    return rc;
}

// mxg_add_assembly_text_device: FASTA text that lies in HBM already (another handle's, or a scaffold stage's) becomes this assembly's
// text by one device-to-device copy; header lines by the kernels of the BGZF route, the rest by ingest_text.  There is no host parser
// to hand the text to: what the file route answers with "not for this route" is MXG_ELIMIT / MXG_ENOMEM here.
int load_text_device(mxg_handle *h, Assembly *a, const void *d_src, uint64_t n_bytes)
{
    const char *what = a->name.c_str();
    const bool dbg_io = getenv("MXG_DEBUG_IO") != nullptr;
    auto now_s = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    IngestTimes tp;
    tp.t0 = now_s();
    const uint64_t n_tiles = (n_bytes + ING_TILE - 1) / ING_TILE;
    if (n_tiles >= (1ull << 31)) return set_err(h, MXG_ELIMIT, "mxg_add_assembly_text_device: %llu bytes are too many for one handle", (unsigned long long)n_bytes);
    MXG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const uint64_t text_alloc = (n_tiles + 1) * ING_TILE;  // (as load_fasta_device allocates and pads it)
    HdrScan scan;
    hipError_t e = a->d_text.ensure(text_alloc);
    if (e == hipSuccess && n_bytes) e = hdr_scan_alloc(scan, n_bytes);
    if (e != hipSuccess)
        return soft_alloc_failure(e) ? set_err(h, MXG_ENOMEM, "mxg_add_assembly_text_device: no room on the device for a copy of the text (%llu bytes)",
                                               (unsigned long long)n_bytes)
                                     : set_err(h, MXG_EDEVICE, "device allocation failed: %s", hipGetErrorString(e));
    unsigned char *d_text = a->d_text.as<unsigned char>();
    if (n_bytes) MXG_HIP(h, hipMemcpyAsync(d_text, d_src, n_bytes, hipMemcpyDeviceToDevice, st));
    MXG_HIP(h, hipMemsetAsync(d_text + n_bytes, '\n', text_alloc - n_bytes, st));
    std::vector<Hdr> hdr;
    std::vector<unsigned char> hdr_lines;
    std::vector<uint64_t> hdr_line_off(1, 0);
    int rc = MXG_OK;
    if (n_bytes) {
        if ((rc = hdr_scan_count(h, scan, d_text, n_bytes, st)) != MXG_OK) return rc;
        MXG_HIP(h, hipStreamSynchronize(st));  // (the source is free from here on)
        rc = hdr_scan_lines(h, what, scan, d_text, n_bytes, st, hdr, hdr_lines, hdr_line_off);
    } else {
        MXG_HIP(h, hipStreamSynchronize(st));
    }
    IngestRefusal why = IngestRefusal::NoRoom;
    if (rc == MXG_OK) rc = ingest_text(h, a, what, hdr, nullptr, hdr_lines, hdr_line_off, n_bytes, d_text, []() { return MXG_OK; }, tp, why);
    if (rc == 1)
        return why == IngestRefusal::Events
                   ? set_err(h, MXG_ELIMIT, "mxg_add_assembly_text_device: '%s' has more changes between valid and invalid bases than the device "
                                            "route records (MXG_INGEST_EV_CAP), and text on the device has no host parser to go to", what)
                   : set_err(h, MXG_ENOMEM, "mxg_add_assembly_text_device: no room on the device for the tables of '%s'", what);
    if (rc != MXG_OK) return rc;
    if (dbg_io)
        fprintf(stderr, "[mxg] load_text_device %s: %.3f s = copy + headers + items until %.3f, base counts at %.3f, packed at %.3f, run table at "
                        "%.3f (%.2f GB)\n", what, now_s() - tp.t0, tp.hdr, tp.count, tp.pack, now_s() - tp.t0, n_bytes / 1e9);
    drop_device_text_if_asked(h, a);
    return rc;
}

static void drop_device_text_if_asked(mxg_handle *h, Assembly *a)
{
    if (h->cfg.flags & MXG_FLAG_DROP_SEQ) {  // the caller does not want the text kept: k-mers are then printed from the packed bases
        a->d_text.release();
        a->d_ing_items.release();
        a->d_ing_sub.release();
        a->d_ing_pbase.release();
        a->d_ing_cnt.release();
        a->text_on_device = false;
    }
}

// ======================================================================================================
// TSV text on the device
// ======================================================================================================
struct TsvParams {
    uint64_t n;               // minimizers
    const uint64_t *hash;
    const uint32_t *pos, *rec;
    const uint8_t *fwd;
    uint32_t with_pos, with_strand, with_seq, k;
    const uint64_t *rec_first;   // [n_rec + 1]
    const uint64_t *rec_prefix;  // [n_rec]: bytes of the id columns (and of the lines of records without minimizers) before record r
    const uint32_t *id_off;      // [n_rec + 1] into ids
    const char *ids;
    uint64_t n_rec;
    uint8_t *len;             // [n] entry length incl. its separator
    const uint64_t *off;      // [n + 1] exclusive scan of len
    // k-mer text: the FASTA's own spelling (text in HBM) or decoded from the packed bases
    const unsigned char *text;
    const IngItem *items;
    const uint64_t *item_pbase;
    const uint16_t *item_sub;
    const uint64_t *rec_item0;
    const uint64_t *rec_base;    // [n_rec] packed base offset of record r
    const uint32_t *packed;
    // output window
    char *out;
    uint64_t win_lo, win_hi;
};

__global__ __launch_bounds__(256) void k_tsv_len(const TsvParams p)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n) return;
    uint32_t l = dec_digits(p.hash[i]) + 1u;  // + separator (' ' or the line's '\n')
    if (p.with_pos) l += 1u + dec_digits(p.pos[i]);
    if (p.with_strand) l += 2u;
    if (p.with_seq) l += 1u + p.k;
    p.len[i] = (uint8_t)l;  // (k <= 200 on this route: the host writer takes longer k-mers)
}

// exclusive scan of u8 lengths into u64 offsets: tile sums -> one block scans them (u64) -> tiles add their base
__global__ __launch_bounds__(256) void k_tsv_tile_sum(const uint8_t *__restrict__ len, uint64_t n, uint32_t *__restrict__ tsum)
{
    __shared__ uint32_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * TILE_PER_THREAD;
    uint32_t c = 0;
    for (int u = 0; u < TILE_PER_THREAD; ++u)
        if (base + u < n) c += len[base + u];
    (void)block_exclusive_256(c, sh);
    if (threadIdx.x == 0) tsum[blockIdx.x] = sh[255];
}
__global__ __launch_bounds__(256) void k_tsv_scan_tiles(const uint32_t *__restrict__ tsum, uint32_t n_tiles, uint64_t *__restrict__ tbase,
                                                        uint64_t *__restrict__ total)
{
    __shared__ uint32_t sh[256];
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_tiles; b0 += 256u * 16u) {
        const uint32_t i0 = b0 + threadIdx.x * 16u;
        uint32_t v[16], c = 0;
        for (int u = 0; u < 16; ++u) {
            v[u] = i0 + u < n_tiles ? tsum[i0 + u] : 0u;
            c += v[u];  // (a tile holds at most 1024 x 255 bytes, 4096 tiles per pass: fits 32 bits)
        }
        uint64_t run = carry + block_exclusive_256(c, sh);
        const uint32_t pass = sh[255];
        for (int u = 0; u < 16; ++u) {
            if (i0 + u < n_tiles) tbase[i0 + u] = run;
            run += v[u];
        }
        carry += pass;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(256) void k_tsv_offsets(const uint8_t *__restrict__ len, uint64_t n, const uint64_t *__restrict__ tbase,
                                                     const uint64_t *__restrict__ total, uint64_t *__restrict__ off)
{
    __shared__ uint32_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * TILE_PER_THREAD;
    uint32_t v[TILE_PER_THREAD], c = 0;
    for (int u = 0; u < TILE_PER_THREAD; ++u) {
        v[u] = base + u < n ? len[base + u] : 0u;
        c += v[u];
    }
    uint64_t run = tbase[blockIdx.x] + block_exclusive_256(c, sh);
    for (int u = 0; u < TILE_PER_THREAD; ++u) {
        if (base + u < n) off[base + u] = run;
        run += v[u];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) off[n] = *total;
}

// the tile index as text_of_base (text_index.h) reads it
__device__ __forceinline__ TextIndex tsv_text_index(const TsvParams &p)
{
    return TextIndex{p.text, p.items, p.item_pbase, p.item_sub, p.rec_item0, p.rec_base};
}

__global__ __launch_bounds__(256) void k_tsv_entries(const TsvParams p)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t r = p.rec[i];
    // global offset = everything the id columns before and including this record's take + the entries before this one
    const uint64_t at = p.rec_prefix[r] + (p.id_off[r + 1] - p.id_off[r]) + 1u + p.off[i];
    const uint64_t end = at + p.len[i];
    if (end <= p.win_lo || at >= p.win_hi) return;
    WinSink o{at, p.win_lo, p.win_hi, p.out};
    o.num(p.hash[i]);
    if (p.with_pos) {
        o.ch(':');
        o.num(p.pos[i]);
    }
    if (p.with_strand) {
        o.ch(':');
        o.ch(p.fwd[i] ? '+' : '-');
    }
    if (p.with_seq) {
        o.ch(':');
        if (p.text) {
            uint64_t a = text_of_base(tsv_text_index(p), r, p.pos[i]);
            for (uint32_t u = 0; u < p.k; ++a) {
                const unsigned char b = p.text[a];
                if (b == '\n' || b == '\r') continue;
                o.ch((char)b);
                ++u;
            }
        } else {
            const uint64_t b0 = p.rec_base[r] + p.pos[i];
            for (uint32_t u = 0; u < p.k; ++u) {
                const uint64_t g = b0 + u;
                o.ch("ACGT"[(p.packed[g >> 4] >> (2u * ((uint32_t)g & 15u))) & 3u]);
            }
        }
    }
    o.ch(i + 1 == p.rec_first[r + 1] ? '\n' : ' ');
}

// one thread per record: its id, the tab, and the line break of a record without minimizers
__global__ __launch_bounds__(256) void k_tsv_ids(const TsvParams p)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= p.n_rec) return;
    const uint64_t f = p.rec_first[r];
    const uint64_t at = p.rec_prefix[r] + p.off[f];
    const uint32_t l = p.id_off[r + 1] - p.id_off[r];
    if (at + l + 2u <= p.win_lo || at >= p.win_hi) return;
    WinSink o{at, p.win_lo, p.win_hi, p.out};
    for (uint32_t u = 0; u < l; ++u) o.ch(p.ids[p.id_off[r] + u]);
    o.ch('\t');
    if (p.rec_first[r + 1] == f) o.ch('\n');
}

// The sequences of a device-ingested assembly as the file spells them, line breaks removed, for the host writer: record r's bases
// are seq[rec_off[r]], seq[rec_off[r] + 1], ...  (The whole text comes over at once: host memory of the file's size next to `seq`.)
int fetch_device_text(mxg_handle *h, Assembly *a, std::string &seq, std::vector<uint64_t> &rec_off)
{
    const size_t n_rec = a->recs.size();
    rec_off.assign(n_rec + 1, 0);
    seq.clear();
    if (!a->text_on_device || a->ing_item0.size() != n_rec + 1)
        return set_err(h, MXG_EINVAL, "assembly '%s' holds no text on the device", a->name.c_str());
    const size_t n_items = a->ing_item0[n_rec];
    std::vector<IngItem> items(n_items);
    std::vector<unsigned char> text(a->text_bytes);
    MXG_HIP(h, hipSetDevice(h->device));
    if (n_items) MXG_HIP(h, hipMemcpyAsync(items.data(), a->d_ing_items.p, n_items * sizeof(IngItem), hipMemcpyDeviceToHost, h->stream));
    if (!text.empty()) MXG_HIP(h, hipMemcpyAsync(text.data(), a->d_text.p, text.size(), hipMemcpyDeviceToHost, h->stream));
    MXG_HIP(h, hipStreamSynchronize(h->stream));
    seq.reserve(a->total_bases);
    for (size_t r = 0; r < n_rec; ++r) {
        rec_off[r] = seq.size();
        for (uint64_t q = a->ing_item0[r]; q < a->ing_item0[r + 1]; ++q) {
            if (items[q].lo + items[q].len > text.size()) return set_err(h, MXG_EDEVICE, "internal error: text item out of range");
            for (uint64_t at = items[q].lo; at < items[q].lo + items[q].len; ++at)
                if (text[at] != '\n' && text[at] != '\r') seq.push_back((char)text[at]);
        }
    }
    rec_off[n_rec] = seq.size();
    return MXG_OK;
}

int write_tsv_device(mxg_handle *h, Assembly *a, const char *path, int with_pos, int with_strand, int with_seq)
{
    if (!a->has_sketch) return set_err(h, MXG_EINVAL, "assembly '%s' has no sketch yet (call mxg_sketch)", a->name.c_str());
    const uint32_t k = h->cfg.k;
    const bool dbg_io = getenv("MXG_DEBUG_IO") != nullptr;  // timings on stderr
    auto now_s = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now_s();
    double t_tables = 0;
    MXG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    int rc;
    if (with_strand && (rc = ensure_strand(h, a)) != MXG_OK) return rc;
    const uint64_t n = a->n_mx, n_rec = a->recs.size();
    // record table: first minimizer of every record (from the record column, 4 bytes per minimizer over PCIe)
    std::vector<uint32_t> h_rec(n);
    if (n) MXG_HIP(h, hipMemcpyAsync(h_rec.data(), a->d_rec.p, n * 4, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    const double t_rec = now_s() - t_begin;  // (the record column on the host)
    std::vector<uint64_t> rec_first(n_rec + 1, 0);
    for (uint64_t i = 0; i < n; ++i) rec_first[h_rec[i] + 1]++;
    for (uint64_t r = 0; r < n_rec; ++r) rec_first[r + 1] += rec_first[r];
    const uint64_t r_lo = std::min<uint64_t>(a->shard_lo, n_rec), r_hi = std::min<uint64_t>(a->shard_hi, n_rec);
    (void)r_lo;
    (void)r_hi;  // (sharded loads go through the host writer)
    std::vector<uint64_t> rec_prefix(n_rec), rec_base(n_rec);
    std::vector<uint32_t> id_off(n_rec + 1);
    std::string ids;
    uint64_t pre = 0;
    for (uint64_t r = 0; r < n_rec; ++r) {
        rec_prefix[r] = pre;
        id_off[r] = (uint32_t)ids.size();
        ids += a->recs[r].id;
        pre += a->recs[r].id.size() + 1 + (rec_first[r + 1] == rec_first[r] ? 1 : 0);
        rec_base[r] = a->recs[r].base_off;
    }
    id_off[n_rec] = (uint32_t)ids.size();
    if (ids.size() >= (1ull << 32)) return set_err(h, MXG_ELIMIT, "record ids too long");
    const double t_host = now_s() - t_begin - t_rec;  // (the record tables)
    DevBuf d_first, d_prefix, d_idoff, d_ids, d_len, d_off, d_tsum, d_tbase, d_total, d_recbase;
    auto up = [&](DevBuf &b, const void *src, size_t bytes) -> int {
        MXG_HIP(h, b.ensure(std::max<size_t>(bytes, 16)));
        if (bytes) MXG_HIP(h, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st));
        return MXG_OK;
    };
    if ((rc = up(d_first, rec_first.data(), (n_rec + 1) * 8)) != MXG_OK) return rc;
    if ((rc = up(d_prefix, rec_prefix.data(), n_rec * 8)) != MXG_OK) return rc;
    if ((rc = up(d_idoff, id_off.data(), (n_rec + 1) * 4)) != MXG_OK) return rc;
    if ((rc = up(d_ids, ids.data(), ids.size())) != MXG_OK) return rc;
    if ((rc = up(d_recbase, rec_base.data(), n_rec * 8)) != MXG_OK) return rc;
    const uint32_t n_tiles = (uint32_t)((n + TILE - 1) / TILE);
    MXG_HIP(h, d_len.ensure(std::max<uint64_t>(n, 16)));
    MXG_HIP(h, d_off.ensure((n + 1) * 8));
    MXG_HIP(h, d_tsum.ensure(std::max<size_t>((size_t)n_tiles * 4, 16)));
    MXG_HIP(h, d_tbase.ensure(std::max<size_t>((size_t)n_tiles * 8, 16)));
    MXG_HIP(h, d_total.ensure(16));
    TsvParams p;
    memset(&p, 0, sizeof p);
    p.n = n;
    p.hash = a->d_hash.as<uint64_t>();
    p.pos = a->d_pos.as<uint32_t>();
    p.rec = a->d_rec.as<uint32_t>();
    p.fwd = a->d_fwd.as<uint8_t>();
    p.with_pos = with_pos;
    p.with_strand = with_strand;
    p.with_seq = with_seq;
    p.k = k;
    p.rec_first = d_first.as<uint64_t>();
    p.rec_prefix = d_prefix.as<uint64_t>();
    p.id_off = d_idoff.as<uint32_t>();
    p.ids = d_ids.as<char>();
    p.n_rec = n_rec;
    p.len = d_len.as<uint8_t>();
    p.off = d_off.as<uint64_t>();
    p.rec_base = d_recbase.as<uint64_t>();
    p.packed = a->d_packed;
    if (a->text_on_device) {
        DevBuf &d_item0 = a->d_ing_item0;
        if (!d_item0.p) {
            if ((rc = up(d_item0, a->ing_item0.data(), a->ing_item0.size() * 8)) != MXG_OK) return rc;
        }
        p.text = a->d_text.as<unsigned char>();
        p.items = a->d_ing_items.as<IngItem>();
        p.item_pbase = a->d_ing_pbase.as<uint64_t>();
        p.item_sub = a->d_ing_sub.as<uint16_t>();
        p.rec_item0 = d_item0.as<uint64_t>();
    }
    uint64_t total_entries = 0;
    const double t_up = now_s() - t_begin - t_rec - t_host;  // (their upload, the arrays of the lengths)
    if (n) {
        hipLaunchKernelGGL(k_tsv_len, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, p);
        hipLaunchKernelGGL(k_tsv_tile_sum, dim3(n_tiles), dim3(256), 0, st, d_len.as<uint8_t>(), n, d_tsum.as<uint32_t>());
        hipLaunchKernelGGL(k_tsv_scan_tiles, dim3(1), dim3(256), 0, st, d_tsum.as<uint32_t>(), n_tiles, d_tbase.as<uint64_t>(),
                           d_total.as<uint64_t>());
        hipLaunchKernelGGL(k_tsv_offsets, dim3(n_tiles), dim3(256), 0, st, d_len.as<uint8_t>(), n, d_tbase.as<uint64_t>(),
                           d_total.as<uint64_t>(), d_off.as<uint64_t>());
        MXG_HIP(h, hipGetLastError());
        MXG_HIP(h, hipMemcpyAsync(&total_entries, d_total.p, 8, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
    } else {
        MXG_HIP(h, hipMemsetAsync(d_off.p, 0, 8, st));
    }
    const uint64_t total = pre + total_entries;
    t_tables = now_s() - t_begin;
    OutFile of;
    if (!of.open(path)) return set_err(h, MXG_EIO, "cannot open '%s' for writing", path);
    // MXG_TSV_WIN (test knob): bytes of text per window, 1 .. a half of the pinned pool
    const uint64_t WIN = std::max<uint64_t>(1, std::min<uint64_t>(knob_u64(h, "MXG_TSV_WIN", PIN_HALF), PIN_HALF));
    const WinFill fill = [&](uint64_t, unsigned char *d_win, uint64_t lo, uint64_t hi) -> int {
        p.out = reinterpret_cast<char *>(d_win);
        p.win_lo = lo;
        p.win_hi = hi;
        if (n) hipLaunchKernelGGL(k_tsv_entries, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, p);
        if (n_rec) hipLaunchKernelGGL(k_tsv_ids, dim3((uint32_t)((n_rec + 255) / 256)), dim3(256), 0, st, p);
        MXG_HIP(h, hipGetLastError());
        return MXG_OK;
    };
    WinTimes tw;
    rc = write_windows(h, of, total, WIN, 0, fill, "mxg_write_tsv", &tw);
    const bool closed = of.close();
    if (dbg_io)
        fprintf(stderr, "[mxg] write_tsv_device %s: %.3f s = tables %.3f (record column to the host %.3f, record tables %.3f, uploads + allocations %.3f, lengths + offsets %.3f) + buffers %.3f + waiting for the device %.3f + writing %.3f (%llu MB)\n",
                a->name.c_str(), now_s() - t_begin, t_tables, t_rec, t_host, t_up, t_tables - t_rec - t_host - t_up, tw.buffers, tw.dev_wait, tw.put,
                (unsigned long long)(total >> 20));
    if (rc != MXG_OK) return rc;
    if (!closed) return set_err(h, MXG_EIO, "write error on '%s'", path);
    of.complete = true;
    return MXG_OK;
}

}  // namespace mxg
