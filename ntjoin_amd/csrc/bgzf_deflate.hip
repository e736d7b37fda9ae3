// bgzf_deflate.hip -- text on the device written as a BGZF file: the counterpart of bgzf.hip.  A window of text in device memory
// becomes a chain of members (bgzf_deflate.h: at most P <= 65 280 bytes of text each, literals only), the members are packed side
// by side, and only the compressed bytes cross host memory (scaffold.hip: the scaffold FASTA; mxg_bgzf_write: any host bytes).
//
//   k_bgzf_deflate  ONE MEMBER PER WORK-GROUP of 256 threads.
//       pass 1  the member's text is read once, coalesced, into histograms in LDS: 16 tables per block of the member (a table per
//               lane mod 16: four letters carry almost all counts, one table would serialise every atomic of a wave), summed by
//               symbol; two lanes in two waves then build the blocks' codes and headers (bgzf_build: the text the host compiles).
//       pass 2  thread t owns text bytes [255 t, 255 t + 255).  It adds up their code lengths (and takes their CRC), an exclusive
//               scan over the group gives its first bit, and it packs its codes through a 64-bit accumulator into the member's
//               image in LDS: the image starts out zero, whole words are stored, the first and the last word of a thread are ORed
//               in with LDS atomics.  The image (64 KiB, over the histograms' place) leaves with 16-byte stores into the member's
//               slot of P + 31 bytes, rounded up to 16.
//       CRC-32  each thread's piece by the table, the pieces shifted by x^(8 x bytes behind them) mod P and XORed over the group.
//   k_bgzf_pack     the members' sizes are scanned (scan_kernels.h) and every member is copied to its place in the packed chain,
//               as aligned words of the destination put together from two words of the slot.
// The packed window starts with 16 bytes {u64 bytes, u32 stored members, u32 0} that travel to the host in front of the data.
// The host side (bgzf_write_windows) is a sequence of its own made of the parts of the window protocol (win_out.hip).
#include <algorithm>
#include <numeric>

#include "bgzf_deflate.h"
#include "mxg_internal.h"
#include "scan_kernels.h"

namespace mxg {

constexpr uint32_t BGZF_IMG_WORDS = 16384;  // the member's image: 64 KiB
constexpr uint32_t BGZF_HIST_TABS = 16;     // histogram tables per block of the member
constexpr uint32_t BGZF_SHARE = 255;        // text bytes per thread
static_assert(BGZF_MAX_PAYLOAD + BGZF_SLACK <= 4 * BGZF_IMG_WORDS, "a member fits its image");
static_assert(BGZF_MAX_BLOCKS * BGZF_HIST_TABS * BGZF_NSYM <= BGZF_IMG_WORDS, "the histograms fit the image's place");
static_assert(BGZF_SHARE * 256 == BGZF_MAX_PAYLOAD && BGZF_SHARE * 128 == BGZF_SPLIT, "256 shares a member, 128 a block");

struct BgzfWinHead {  // in front of a packed window
    uint64_t bytes;
    uint32_t stored, pad;
};
static_assert(sizeof(BgzfWinHead) == 16, "the packed chain starts 16-byte aligned");

// the text's bytes by aligned words (the window's allocation ends on whole words beyond the text)
struct BgzfTextSrc {
    const unsigned char *p;
    uint32_t have = 0xFFFFFFFFu, word = 0;
    __device__ __forceinline__ uint32_t byte(uint32_t i)
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p) + i;
        const uint32_t w = (uint32_t)(a >> 2);
        if (w != have) {
            word = *reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
            have = w;
        }
        return (word >> (8u * ((uint32_t)a & 3u))) & 255u;
    }
};

__device__ __forceinline__ void bgzf_or_bits(uint32_t *img, uint32_t pos, uint32_t v, uint32_t n)  // n <= 16 bits at bit `pos`
{
    const uint32_t i = pos >> 5, sh = pos & 31u;
    if (i < BGZF_IMG_WORDS) atomicOr(&img[i], v << sh);
    if (sh + n > 32u && i + 1u < BGZF_IMG_WORDS) atomicOr(&img[i + 1u], v >> (32u - sh));
}

__global__ __launch_bounds__(256) void k_bgzf_deflate(const unsigned char *__restrict__ text, uint64_t n_text, uint32_t P,
                                                      unsigned char *__restrict__ slots, uint32_t slot_bytes, uint32_t *__restrict__ sizes,
                                                      BgzfWinHead *__restrict__ head)
{
    __shared__ __attribute__((aligned(16))) uint32_t img[BGZF_IMG_WORDS];
    __shared__ BgzfEnc enc[BGZF_MAX_BLOCKS];
    __shared__ BgzfMemberPlan plan;
    __shared__ uint32_t crc_tab[256];
    __shared__ uint32_t sh[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t lo = (uint64_t)blockIdx.x * P;
    if (lo >= n_text) return;  // (the grid is the members of the window: never taken)
    const uint32_t n = (uint32_t)min((uint64_t)P, n_text - lo);
    const unsigned char *src = text + lo;
    // ---- pass 1: histograms
    for (uint32_t i = tid; i < BGZF_MAX_BLOCKS * BGZF_HIST_TABS * BGZF_NSYM; i += 256u) img[i] = 0;
    crc_tab[tid] = bgzf_crc32_entry(tid);
    __syncthreads();
    {
        uint32_t *tab0 = img + (tid & (BGZF_HIST_TABS - 1u)) * BGZF_NSYM;
        const bool aligned = (reinterpret_cast<uintptr_t>(src) & 3u) == 0;
        for (uint32_t i = 4u * tid; i < n; i += 1024u) {
            uint32_t *tab = tab0 + (i >= BGZF_SPLIT ? BGZF_HIST_TABS * BGZF_NSYM : 0u);  // (BGZF_SPLIT is a multiple of 4)
            if (aligned && i + 4u <= n) {
                const uint32_t w = *reinterpret_cast<const uint32_t *>(src + i);
                atomicAdd(&tab[w & 255u], 1u);
                atomicAdd(&tab[(w >> 8) & 255u], 1u);
                atomicAdd(&tab[(w >> 16) & 255u], 1u);
                atomicAdd(&tab[w >> 24], 1u);
            } else {
                for (uint32_t u = i; u < min(n, i + 4u); ++u) atomicAdd(&tab[src[u]], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t b = 0; b < BGZF_MAX_BLOCKS; ++b) {
        uint32_t f = 0;
        for (uint32_t u = 0; u < BGZF_HIST_TABS; ++u) f += img[(b * BGZF_HIST_TABS + u) * BGZF_NSYM + tid];
        enc[b].freq[tid] = f;
    }
    __syncthreads();
    for (uint32_t i = tid; i < BGZF_IMG_WORDS / 4u; i += 256u) reinterpret_cast<uint4 *>(img)[i] = make_uint4(0, 0, 0, 0);
    if (tid == 0 || (tid == 64u && n > BGZF_SPLIT)) bgzf_build(enc[tid >> 6]);
    __syncthreads();
    if (tid == 0) {
        bgzf_plan_member(enc, n, plan);
        bgzf_put_member_header(img, BGZF_HEAD + plan.deflate_bytes + BGZF_TRAIL);
        if (plan.stored) {
            unsigned char *d = reinterpret_cast<unsigned char *>(img) + BGZF_HEAD;
            d[0] = 1;
            d[1] = (unsigned char)n, d[2] = (unsigned char)(n >> 8);
            d[3] = (unsigned char)~n, d[4] = (unsigned char)(~n >> 8);
        } else {
            for (uint32_t b = 0; b < plan.n_blocks; ++b) {
                BgzfBitW w{img, BGZF_IMG_WORDS, 8u * BGZF_HEAD + plan.bit0[b]};
                bgzf_put_block_header(enc[b], w, b + 1u == plan.n_blocks ? 1u : 0u);
            }
        }
    }
    __syncthreads();
    // ---- pass 2: the thread's share
    const uint32_t b0 = min(n, tid * BGZF_SHARE), b1 = min(n, b0 + BGZF_SHARE);
    const uint32_t blk = tid >> 7;  // (shares of threads 128 .. 255 start at BGZF_SPLIT)
    const uint32_t *code = enc[blk].code;
    const bool stored = plan.stored != 0;
    BgzfTextSrc ts{src};
    uint32_t bits = 0, crc = tid == 0 ? 0xFFFFFFFFu : 0u;
    for (uint32_t i = b0; i < b1; ++i) {
        const uint32_t c = ts.byte(i);
        bits += code[c] >> 16;
        crc = crc_tab[(crc ^ c) & 255u] ^ (crc >> 8);
    }
    const uint32_t excl = block_exclusive_256(bits, sh);
    if (stored) {
        unsigned char *d = reinterpret_cast<unsigned char *>(img) + BGZF_HEAD + 5u;
        for (uint32_t i = tid; i < n; i += 256u) d[i] = src[i];
    } else {
        // the first bit: behind the member's header, the blocks' headers up to this thread's block and the end-of-block code of the
        // first block for a thread of the second
        uint32_t pos = 8u * BGZF_HEAD + enc[0].hdr_bits + excl;
        if (blk) pos += (enc[0].code[256] >> 16) + enc[1].hdr_bits;
        uint32_t wi = pos >> 5, have = pos & 31u;
        uint64_t acc = 0;
        bool first = true;
        for (uint32_t i = b0; i < b1; ++i) {
            const uint32_t c = code[ts.byte(i)];
            acc |= (uint64_t)(c & 0xFFFFu) << have;
            have += c >> 16;
            if (have >= 32u) {
                if (wi < BGZF_IMG_WORDS) {
                    if (first) atomicOr(&img[wi], (uint32_t)acc);
                    else img[wi] = (uint32_t)acc;
                }
                first = false;
                ++wi;
                acc >>= 32;
                have -= 32u;
            }
        }
        if (have && (uint32_t)acc && wi < BGZF_IMG_WORDS) atomicOr(&img[wi], (uint32_t)acc);
        if (tid < plan.n_blocks) {  // the end-of-block codes: the last bits of their blocks
            const uint32_t c = enc[tid].code[256];
            bgzf_or_bits(img, 8u * BGZF_HEAD + plan.bit0[tid] + enc[tid].hdr_bits + enc[tid].data_bits - (c >> 16), c & 0xFFFFu, c >> 16);
        }
    }
    // ---- CRC-32 of the text
    crc = bgzf_crc_shift(crc, n - b1);
    for (int o = 32; o > 0; o >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, o, 64);
    __syncthreads();  // (the scan's words are read; the image is complete but for the trailer)
    if ((tid & 63u) == 0) sh[tid >> 6] = crc;
    __syncthreads();
    const uint32_t size = BGZF_HEAD + plan.deflate_bytes + BGZF_TRAIL;
    if (tid == 0) {
        const uint32_t c = (sh[0] ^ sh[1] ^ sh[2] ^ sh[3]) ^ 0xFFFFFFFFu;
        unsigned char *d = reinterpret_cast<unsigned char *>(img) + BGZF_HEAD + plan.deflate_bytes;
        for (uint32_t u = 0; u < 4; ++u) {
            d[u] = (unsigned char)(c >> (8u * u));
            d[4u + u] = (unsigned char)(n >> (8u * u));
        }
        sizes[blockIdx.x] = size;
        if (stored) atomicAdd(&head->stored, 1u);
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(slots + (uint64_t)blockIdx.x * slot_bytes);  // (slot_bytes is a multiple of 16, >= size)
    for (uint32_t i = tid; i < (size + 15u) / 16u; i += 256u) dst[i] = reinterpret_cast<const uint4 *>(img)[i];
}

// member m of the window: sizes[m] bytes from its slot to offs[m] of the packed chain
__global__ __launch_bounds__(256) void k_bgzf_pack(const unsigned char *__restrict__ slots, uint32_t slot_bytes, const uint32_t *__restrict__ sizes,
                                                   const uint32_t *__restrict__ offs, unsigned char *__restrict__ out, uint64_t out_bytes)
{
    const uint32_t tid = threadIdx.x, size = min(sizes[blockIdx.x], slot_bytes);
    const uint64_t off = offs[blockIdx.x];
    if (off + size > out_bytes) return;  // (the chain's room is the sum of the slots: never taken)
    const unsigned char *src = slots + (uint64_t)blockIdx.x * slot_bytes;  // 16-byte aligned
    unsigned char *dst = out + off;
    const uint32_t head = min(size, (uint32_t)((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
    if (tid < head) dst[tid] = src[tid];
    const uint32_t nw = (size - head) / 4u;
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(src);
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
    const uint32_t a = 8u * (head & 3u);  // (source byte head + 4 w: the same place in its word for every w)
    for (uint32_t w = tid; w < nw; w += 256u) {
        const uint32_t s = (head >> 2) + w;
        uint32_t v = sw[s];
        if (a) v = v >> a | sw[s + 1u] << (32u - a);  // (word s + 1 holds source byte head + 4 w + 3 < size)
        dw[w] = v;
    }
    const uint32_t done = head + 4u * nw;
    if (tid < size - done) dst[done + tid] = src[done + tid];
}

namespace {
enum { ZB_SLOTS, ZB_SIZES, ZB_OUT };
constexpr size_t PIN_DATA = PIN_HALF - 4096;  // a half's last 4 KiB take the window's head
}  // namespace

uint32_t bgzf_payload(const mxg_handle *h)
{
    const uint64_t p = knob_u64(h, "MXG_BGZF_PAYLOAD", BGZF_MAX_PAYLOAD);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(p, 1), BGZF_MAX_PAYLOAD);
}

// Text bytes per window of a BGZF file with P bytes a member: `want`, and no more than what fits a half of the pinned pool when
// every member is a stored one, rounded down to whole units of lcm(tile, P) -- so that member j of the file holds its text bytes
// [j P, j P + P) whatever the window -- and at least one unit.
uint64_t bgzf_window_bytes(uint64_t want, uint32_t tile, uint32_t P)
{
    const uint64_t unit = std::lcm<uint64_t>(tile, P);
    want = std::min<uint64_t>(want, PIN_DATA / (P + BGZF_SLACK) * P);
    return std::max<uint64_t>(unit, want / unit * unit);
}

// A BGZF file of `total` bytes of text through `of`, window by window, from the parts of the plain window loop (win_out.hip: the
// fill, WinBufs, copy_pieces, OutFile::put) in a sequence of its own: the members of a window are deflated and packed on the
// device behind the fill, the window's head comes over first and says how many bytes to fetch, and the host writes them at the
// running offset while the device forms the next window.  The end-of-file marker follows the last member.
int bgzf_write_windows(mxg_handle *h, OutFile &of, uint64_t total, uint64_t WIN, uint32_t P, const WinFill &fill, const char *who,
                       std::vector<uint64_t> *member_off)
{
    hipStream_t st = h->stream;
    DevBuf *Z = h->zbuf;
    const bool dbg_io = getenv("MXG_DEBUG_IO") != nullptr;
    uint64_t file_off = 0, n_members = 0, n_stored = 0;
    double ms = 0;
    auto put = [&](const char *p, uint64_t bytes) -> bool {  // ... at the running offset
        const bool ok = of.put(p, bytes, file_off, host_threads(h));
        file_off += bytes;
        return ok;
    };
    if (total) {
        const uint64_t win_bytes = std::min(WIN, total);  // (the largest window)
        const uint64_t win_members = (win_bytes + P - 1) / P;
        const uint32_t slot = (P + BGZF_SLACK + 15u) / 16u * 16u;
        const uint64_t out_room = win_members * slot;
        if (out_room >= (1ull << 32)) return set_err(h, MXG_ELIMIT, "%s: a window of %llu members does not fit 32-bit offsets", who, (unsigned long long)win_members);
        const uint32_t n_tiles = (uint32_t)((win_members + TILE - 1) / TILE);
        MXG_HIP(h, Z[ZB_SLOTS].ensure(out_room));
        MXG_HIP(h, Z[ZB_SIZES].ensure((2 * win_members + n_tiles + 4) * 4));
        MXG_HIP(h, Z[ZB_OUT].ensure(sizeof(BgzfWinHead) + out_room + 16));
        WinBufs wb(h);
        int rc = wb.init(win_bytes + 16, 4, dbg_io ? 4 : 0);
        if (rc != MXG_OK) return rc;
        char **pin = wb.pin;
        hipEvent_t *ev_head = wb.ev, *ev_data = wb.ev + 2, *ev_t0 = wb.ev + 4, *ev_t1 = wb.ev + 6;  // (the last four: MXG_DEBUG_IO)
        unsigned char *d_out = Z[ZB_OUT].as<unsigned char>();
        uint32_t *d_sizes = Z[ZB_SIZES].as<uint32_t>(), *d_offs = d_sizes + win_members, *d_bsum = d_offs + win_members;
        const uint64_t n_win = (total + WIN - 1) / WIN;
        auto members_of = [&](uint64_t c) { return (uint32_t)((std::min(total, (c + 1) * WIN) - c * WIN + P - 1) / P); };
        auto enqueue = [&](uint64_t c) -> int {  // window c: text, members, packed chain, its head on the way to the host
            const int b = (int)(c & 1);
            const uint64_t lo = c * WIN, hi = std::min(total, lo + WIN);
            const uint32_t m = members_of(c);
            unsigned char *d_win = h->tsv_win[b].as<unsigned char>();
            const int rc = fill(c, d_win, lo, hi);
            if (rc != MXG_OK) return rc;
            if (dbg_io) MXG_HIP(h, hipEventRecord(ev_t0[b], st));
            MXG_HIP(h, hipMemsetAsync(d_out, 0, sizeof(BgzfWinHead), st));
            hipLaunchKernelGGL(k_bgzf_deflate, dim3(m), dim3(256), 0, st, d_win, hi - lo, P, Z[ZB_SLOTS].as<unsigned char>(), slot, d_sizes,
                               reinterpret_cast<BgzfWinHead *>(d_out));
            MXG_HIP(h, hipGetLastError());
            launch_scan_u32(st, d_sizes, m, d_bsum, d_offs, reinterpret_cast<uint64_t *>(d_out));
            hipLaunchKernelGGL(k_bgzf_pack, dim3(m), dim3(256), 0, st, Z[ZB_SLOTS].as<unsigned char>(), slot, d_sizes, d_offs,
                               d_out + sizeof(BgzfWinHead), out_room);
            MXG_HIP(h, hipGetLastError());
            if (dbg_io) MXG_HIP(h, hipEventRecord(ev_t1[b], st));
            MXG_HIP(h, hipMemcpyAsync(pin[b] + PIN_DATA, d_out, sizeof(BgzfWinHead), hipMemcpyDeviceToHost, st));
            MXG_HIP(h, hipEventRecord(ev_head[b], st));
            return MXG_OK;
        };
        // bytes [at, at + n) of the packed chain to the half's start (n <= PIN_DATA)
        auto fetch = [&](int b, uint64_t at, uint64_t n) { return copy_pieces(h, pin[b], d_out + sizeof(BgzfWinHead) + at, n); };
        if ((rc = enqueue(0)) != MXG_OK) return rc;
        for (uint64_t c = 0; c < n_win; ++c) {
            const int b = (int)(c & 1);
            if (hipEventSynchronize(ev_head[b]) != hipSuccess) return set_err(h, MXG_EDEVICE, "%s: the device failed while forming '%s'", who, of.path.c_str());
            BgzfWinHead wh;
            memcpy(&wh, pin[b] + PIN_DATA, sizeof wh);
            if (wh.bytes > out_room) return set_err(h, MXG_EDEVICE, "%s: a window of '%s' came back with an impossible size", who, of.path.c_str());
            if (dbg_io) {
                float t = 0;
                if (hipEventElapsedTime(&t, ev_t0[b], ev_t1[b]) == hipSuccess) ms += t;
            }
            if (member_off) {  // (the .gzi: where the window's members lie in its chain, in front of the next window's scan)
                const uint32_t m = members_of(c);
                std::vector<uint32_t> offs(m);
                MXG_HIP(h, hipMemcpyAsync(offs.data(), d_offs, (size_t)m * 4, hipMemcpyDeviceToHost, st));
                MXG_HIP(h, hipStreamSynchronize(st));
                for (uint32_t j = 0; j < m; ++j) member_off->push_back(file_off + offs[j]);
            }
            n_members += members_of(c);
            n_stored += wh.stored;
            bool ok = true;
            if (wh.bytes <= PIN_DATA) {  // the device forms the next window while this one is written
                if ((rc = fetch(b, 0, wh.bytes)) != MXG_OK) return rc;
                MXG_HIP(h, hipEventRecord(ev_data[b], st));
                if (c + 1 < n_win && (rc = enqueue(c + 1)) != MXG_OK) return rc;
                if (hipEventSynchronize(ev_data[b]) != hipSuccess) return set_err(h, MXG_EDEVICE, "%s: the device failed while forming '%s'", who, of.path.c_str());
                ok = put(pin[b], wh.bytes);
            } else {  // (a test's payload size that makes lcm(tile, P) a window of hundreds of MB: piece by piece, nothing alongside)
                for (uint64_t at = 0; at < wh.bytes && ok; at += PIN_DATA) {
                    const uint64_t nb = std::min<uint64_t>(PIN_DATA, wh.bytes - at);
                    if ((rc = fetch(b, at, nb)) != MXG_OK) return rc;
                    MXG_HIP(h, hipStreamSynchronize(st));
                    ok = put(pin[b], nb);
                }
                if (ok && c + 1 < n_win && (rc = enqueue(c + 1)) != MXG_OK) return rc;
            }
            if (!ok) return set_err(h, MXG_EIO, "write error on '%s'", of.path.c_str());
        }
    }
    unsigned char eof[BGZF_EOF_BYTES];
    bgzf_deflate_member_host(nullptr, 0, eof);
    if (!put(reinterpret_cast<const char *>(eof), BGZF_EOF_BYTES)) return set_err(h, MXG_EIO, "write error on '%s'", of.path.c_str());
    if (dbg_io)
        fprintf(stderr, "[mxg] bgzf_deflate members=%llu bytes_in=%llu bytes_out=%llu stored=%llu ms=%.3f\n", (unsigned long long)n_members,
                (unsigned long long)total, (unsigned long long)file_off, (unsigned long long)n_stored, ms);
    return MXG_OK;
}

// host bytes -> a BGZF file (mxg_bgzf_write)
int bgzf_write(mxg_handle *h, const void *data, uint64_t n, const char *path)
{
    MXG_HIP(h, hipSetDevice(h->device));
    const uint32_t P = bgzf_payload(h);
    const uint64_t WIN = bgzf_window_bytes(PIN_HALF, 1u, P);
    OutFile of;
    if (!of.open(path)) return set_err(h, MXG_EIO, "cannot open '%s' for writing", path);
    hipStream_t st = h->stream;
    const WinFill fill = [&](uint64_t, unsigned char *d_win, uint64_t lo, uint64_t hi) -> int {
        // (pageable memory: the copy returns when the bytes have left `data`)
        MXG_HIP(h, hipMemcpyAsync(d_win, static_cast<const unsigned char *>(data) + lo, hi - lo, hipMemcpyHostToDevice, st));
        return MXG_OK;
    };
    const int rc = bgzf_write_windows(h, of, n, WIN, P, fill, "mxg_bgzf_write");
    if (rc != MXG_OK) return rc;
    MXG_HIP(h, hipStreamSynchronize(st));
    if (!of.close()) return set_err(h, MXG_EIO, "mxg_bgzf_write: write error while closing '%s'", path);
    of.complete = true;
    return MXG_OK;
}

}  // namespace mxg
