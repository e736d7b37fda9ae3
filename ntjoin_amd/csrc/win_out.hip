// win_out.hip -- how text formed on the device reaches a file: the one window protocol of the device writers (ingest.hip: TSV;
// scaffold.hip: FASTA; pathtext.hip: .path and AGP; bgzf_deflate.hip builds its own sequence from the same parts).
//
// A file of `total` bytes is cut into windows of WIN bytes.  The handle owns two device windows (tsv_win) and a pinned pool whose
// two halves take a window each.  For window c the writer's fill enqueues the kernels that form bytes [c WIN, c WIN + WIN) in
// device window c & 1; the bytes are copied to half c & 1 of the pool and an event is recorded behind the copy.  The host enqueues
// window c + 1 BEFORE it waits for window c's event, so the device forms the next window while the host puts this one into the
// file (OutFile::put, out_file.h: parts side by side at the window's offset of a regular file, in order into anything else).
#include <algorithm>
#include <chrono>

#include "bisect.h"
#include "mxg_internal.h"

namespace mxg {

int WinBufs::init(size_t win_bytes, uint32_t n_plain, uint32_t n_timed)
{
    unsigned char *pool = nullptr;
    MXG_HIP(h, pin_pool_get(h, &pool));
    for (int b = 0; b < 2; ++b) {
        MXG_HIP(h, h->tsv_win[b].ensure(win_bytes));
        pin[b] = reinterpret_cast<char *>(pool) + (size_t)b * PIN_HALF;
    }
    for (uint32_t e = 0; e < n_plain; ++e) MXG_HIP(h, hipEventCreateWithFlags(&ev[e], hipEventDisableTiming));
    for (uint32_t e = n_plain; e < n_plain + n_timed; ++e) MXG_HIP(h, hipEventCreate(&ev[e]));
    return MXG_OK;
}

WinBufs::~WinBufs()
{
    (void)hipStreamSynchronize(h->stream);
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
}

int copy_pieces(mxg_handle *h, char *dst_pinned, const void *src_dev, uint64_t n)
{
    // (the pool is pinned in pieces, each registered with HIP on its own: no copy may reach across two of them)
    for (uint64_t done = 0; done < n; done += PIN_PIECE_BYTES)
        MXG_HIP(h, hipMemcpyAsync(dst_pinned + done, static_cast<const char *>(src_dev) + done, std::min<uint64_t>(PIN_PIECE_BYTES, n - done),
                                  hipMemcpyDeviceToHost, h->stream));
    return MXG_OK;
}

// bounds[c] = the item whose text holds byte c * win of the file (off: [n + 1] offsets, off[n] = the file's size > c * win)
__global__ __launch_bounds__(256) void k_win_bounds(const uint64_t *__restrict__ off, uint32_t n, uint64_t win, uint32_t n_win,
                                                    uint32_t *__restrict__ bounds)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n_win) return;
    const uint64_t target = (uint64_t)c * win;
    bounds[c] = last_le(off, 0u, n, target);  // off[0] = 0 <= target < off[n]
}

void launch_win_bounds(hipStream_t st, const uint64_t *off, uint32_t n, uint64_t WIN, uint32_t n_win, uint32_t *bounds)
{
    hipLaunchKernelGGL(k_win_bounds, dim3((n_win + 255) / 256), dim3(256), 0, st, off, n, WIN, n_win, bounds);
}

int write_windows(mxg_handle *h, OutFile &of, uint64_t total, uint64_t WIN, uint64_t base, const WinFill &fill, const char *who, WinTimes *times)
{
    if (!total) return MXG_OK;
    auto now_s = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    WinTimes tm;
    const double t_begin = now_s();
    WinBufs wb(h);
    int rc = wb.init(WIN, 2);
    tm.buffers = now_s() - t_begin;
    const uint64_t n_win = (total + WIN - 1) / WIN;
    auto enqueue = [&](uint64_t c) -> int {
        const int b = (int)(c & 1);
        const uint64_t lo = c * WIN, hi = std::min(total, lo + WIN);
        int rc = fill(c, h->tsv_win[b].as<unsigned char>(), lo, hi);
        if (rc == MXG_OK) rc = copy_pieces(h, wb.pin[b], h->tsv_win[b].p, hi - lo);
        if (rc != MXG_OK) return rc;
        MXG_HIP(h, hipEventRecord(wb.ev[b], h->stream));
        return MXG_OK;
    };
    if (rc == MXG_OK) rc = enqueue(0);
    for (uint64_t c = 0; c < n_win && rc == MXG_OK; ++c) {
        if (c + 1 < n_win && (rc = enqueue(c + 1)) != MXG_OK) break;  // the device forms the next window while this one is written
        const int b = (int)(c & 1);
        const double tw0 = now_s();
        if (hipEventSynchronize(wb.ev[b]) != hipSuccess) {
            rc = set_err(h, MXG_EDEVICE, "%s: the device failed while forming '%s'", who, of.path.c_str());
            break;
        }
        const double tw1 = now_s();
        const uint64_t bytes = std::min(total, (c + 1) * WIN) - c * WIN;
        const bool ok = of.put(wb.pin[b], bytes, base + c * WIN, host_threads(h));
        tm.dev_wait += tw1 - tw0;
        tm.put += now_s() - tw1;
        if (!ok) rc = set_err(h, MXG_EIO, "write error on '%s'", of.path.c_str());
    }
    if (times) *times = tm;
    return rc;
}

}  // namespace mxg
