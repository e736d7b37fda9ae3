// fai.hip -- FASTA indexes written from what the handle holds (row f9): <fasta>.fai as `samtools faidx` writes it (the reference's
// `%.fai: %` rule, ntJoin:152-153, 207-208) for a loaded assembly (mxg_write_fai) and for the files mxg_write_scaffolds writes
// (MXG_SCAF_FAI), and the .gzi of a BGZF file.  The contract is in include/ntjoin_mx.h and, executable, in tests/_fai_restatement.py.
//
// The line structure of a loaded assembly comes from one pass over its text in the work items of the ingest (text_index.h); no lane
// and no block walks a record -- a scaffold file holds records of hundreds of Mbp on one line:
//   k_fai_items      one block per item, lane t its 16 bytes: the bytes' classes -> the lane's summary (fai_scan.h; 16 bases are the
//                    common case and cost no combine), the 256 summaries folded in order in LDS -> the item's summary.
//   k_fai_tile_agg   256 items a block: their summaries folded with the segmented operator (an item that begins a record forgets what
//   k_fai_tile_scan  is in front of it); one block turns the tiles' totals into what precedes every tile;
//   k_fai_rows       scans its tile again behind that: the value at a record's last item is the record's summary -> its row
//                    {length, offset, line bases, line width, first offending line}; the lowest refused record goes into one word.
// Only that word (and the refused row) come to the host before the file is opened.  The rows stay on the device for the formatter:
//   k_fai_len        bytes of every row's line (CountSink, text_dev.h) -> the shared 64-bit exclusive scan (scan64_kernels.h) gives
//                    every line its place;
//   k_win_bounds     (win_out.hip) per window the row that holds its first byte;  k_fai_emit  the bytes of a window (WinSink).
// Output leaves window by window through write_windows (win_out.hip); MXG_FAI_WIN sets the bytes per window.
// The rows of a scaffold file need no text: every record is one line, {name, len, offset, len, len + 1} with offset the exclusive
// scan of header bytes + len + 1 (k_fai_scaf_rows).  The .gzi is host code over OutFile.
#include <algorithm>
#include <chrono>
#include <string>
#include <unordered_set>

#include "fai_scan.h"
#include "mxg_internal.h"
#include "scan64_kernels.h"
#include "text_dev.h"
#include "text_index.h"

namespace mxg {

enum { FB_SUMS, FB_AGG, FB_EXCL, FB_ROWS, FB_ORG, FB_RLEN, FB_VERDICT, FB_IDOFF, FB_IDS, FB_KEEP, FB_OFF, FB_TSUM, FB_BOUNDS, FB_IV, FB_BUF_COUNT };
static_assert(FB_BUF_COUNT <= 16, "mxg_handle::faibuf too small");

// inclusive scan of one summary per thread over a block of 256 with the segmented operator; afterwards sh[t] holds thread t's
// result (all threads call)
__device__ __forceinline__ FaiSum fai_block_inclusive(FaiSum v, FaiSum *sh)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        FaiSum u;
        if (t >= o) u = sh[t - o];
        __syncthreads();
        if (t >= o) {
            v = fai_seg_combine(u, v);
            sh[t] = v;
        }
        __syncthreads();
    }
    return v;
}

#define FAI_LDS(name) \
    __shared__ __attribute__((aligned(16))) unsigned char name##_raw[256 * sizeof(FaiSum)]; \
    FaiSum *name = reinterpret_cast<FaiSum *>(name##_raw)

__global__ __launch_bounds__(256) void k_fai_items(const unsigned char *__restrict__ text, uint64_t text_bytes, const IngItem *__restrict__ items,
                                                   const uint64_t *__restrict__ rec_item0, FaiSum *__restrict__ sums)
{
    FAI_LDS(sh);
    const IngItem it = items[blockIdx.x];
    const uint64_t tile = it.lo & ~(uint64_t)(ING_TILE - 1);
    const uint64_t a0 = tile + 16u * threadIdx.x;
    const uint64_t lo = max(a0, it.lo), hi = min(a0 + 16u, it.lo + it.len);
    FaiSum s;
    bool plain = true;  // nothing but bases in the lane's bytes
    if (lo < hi) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + a0);  // (the text buffer is padded to whole tiles)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t n_base = 0;
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j) {
            const uint32_t b = (w[j >> 2] >> (8u * (j & 3u))) & 255u;
            if (a0 + j >= lo && a0 + j < hi && b >= 0x21u && b <= 0x7Eu) ++n_base;
        }
        plain = n_base == (uint32_t)(hi - lo);
        if (plain) {
            s = fai_bases(n_base);
        } else {
            uint32_t prev = a0 ? text[a0 - 1] : (uint32_t)'\n';
            const uint32_t behind = a0 + 16u < text_bytes ? text[a0 + 16u] : 0u;
            for (uint32_t j = 0; j < 16; ++j) {
                const uint64_t a = a0 + j;
                const uint32_t b = (w[j >> 2] >> (8u * (j & 3u))) & 255u;
                uint32_t next = j < 15u ? (w[(j + 1u) >> 2] >> (8u * ((j + 1u) & 3u))) & 255u : behind;
                if (a + 1 >= text_bytes) next = 0u;
                if (a >= lo && a < hi) s = fai_combine(s, fai_byte(fai_byte_class(prev, b, next), a));
                prev = b;
            }
        }
    }
    if (__syncthreads_and(plain ? 1 : 0)) {  // (block-uniform) an item inside a line
        s = fai_bases(it.len);
    } else {
        (void)fai_block_inclusive(s, sh);  // (no lane's summary begins a record: the plain operator)
        s = sh[255];
    }
    if (threadIdx.x == 0) {
        s.seg = blockIdx.x == rec_item0[it.rec] ? 1u : 0u;
        sums[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void k_fai_tile_agg(const FaiSum *__restrict__ sums, uint64_t n_items, FaiSum *__restrict__ agg)
{
    FAI_LDS(sh);
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    FaiSum v;
    if (i < n_items) v = sums[i];
    v = fai_block_inclusive(v, sh);
    if (threadIdx.x == 255) agg[blockIdx.x] = v;
}

// excl[t] = the tiles in front of tile t folded, by ONE block
__global__ __launch_bounds__(256) void k_fai_tile_scan(const FaiSum *__restrict__ agg, uint32_t n_tiles, FaiSum *__restrict__ excl)
{
    FAI_LDS(sh);
    FaiSum carry;
    for (uint32_t base = 0; base < n_tiles; base += 256) {
        const uint32_t i = base + threadIdx.x;
        FaiSum v;
        if (i < n_tiles) v = agg[i];
        (void)fai_block_inclusive(v, sh);
        if (i < n_tiles) excl[i] = threadIdx.x ? fai_seg_combine(carry, sh[threadIdx.x - 1]) : carry;
        carry = fai_seg_combine(carry, sh[255]);
        __syncthreads();  // (sh is free for the next round)
    }
}

__global__ __launch_bounds__(256) void k_fai_rows_init(const uint64_t *__restrict__ org, uint64_t n_rec, FaiRow *__restrict__ rows)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rec) return;
    FaiRow row;  // (a record without text: NAME 0 OFFSET 0 0)
    row.offset = org[r];
    rows[r] = row;
}

__global__ __launch_bounds__(256) void k_fai_rows(const FaiSum *__restrict__ sums, const FaiSum *__restrict__ excl, const IngItem *__restrict__ items,
                                                  uint64_t n_items, const uint64_t *__restrict__ org, const uint64_t *__restrict__ rec_len,
                                                  uint64_t n_rec, FaiRow *__restrict__ rows, unsigned long long *__restrict__ verdict)
{
    FAI_LDS(sh);
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    FaiSum v;
    if (i < n_items) v = sums[i];
    v = fai_block_inclusive(v, sh);
    if (i >= n_items) return;
    const uint32_t r = items[i].rec;
    if (i + 1 < n_items && items[i + 1].rec == r) return;  // (not the record's last item)
    FaiRow row = fai_finish(fai_seg_combine(excl[blockIdx.x], v), org[r], (uint64_t)r + 1 == n_rec);
    if (row.err_at == FAI_NONE && row.length != rec_len[r]) row.err_at = FAI_INTERNAL;
    rows[r] = row;
    if (row.err_at != FAI_NONE) atomicMin(verdict, (unsigned long long)r);
}

// ---- the formatter ----
enum : uint32_t { FAI_NAME_ID = 0, FAI_NAME_NTJOIN = 1, FAI_NAME_INTERVAL = 2 };
struct FaiFmt {
    const FaiRow *rows;
    uint64_t *off;           // [n + 1] bytes of the rows' lines, then their offsets
    const uint64_t *id_off;  // [ids + 1] into ids
    const char *ids;
    const uint32_t *iv;      // FAI_NAME_INTERVAL: {record, lo, hi} of row i
    const uint8_t *keep;     // (may be null) 0: row i gets no line
    uint32_t n, name_kind;
};

template <class Sink> __device__ __forceinline__ void fai_line(const FaiFmt &q, uint32_t i, Sink &o)
{
    if (q.name_kind == FAI_NAME_NTJOIN) {
        o.lit("ntJoin", 6u);
        o.num(i);
    } else {
        const uint32_t r = q.name_kind == FAI_NAME_INTERVAL ? q.iv[3u * i] : i;
        o.bytes(q.ids + q.id_off[r], q.id_off[r + 1] - q.id_off[r]);
        if (q.name_kind == FAI_NAME_INTERVAL) {
            o.ch(':');
            o.num(q.iv[3u * i + 1u]);
            o.ch('-');
            o.num(q.iv[3u * i + 2u]);
        }
    }
    const FaiRow row = q.rows[i];
    o.ch('\t');
    o.num(row.length);
    o.ch('\t');
    o.num(row.offset);
    o.ch('\t');
    o.num(row.linebases);
    o.ch('\t');
    o.num(row.linewidth);
    o.ch('\n');
}

__global__ __launch_bounds__(256) void k_fai_len(const FaiFmt q)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > q.n) return;
    CountSink c;
    if (i < q.n && (!q.keep || q.keep[i])) fai_line(q, i, c);
    q.off[i] = c.n;  // (entry n: 0, so that the exclusive sums end with the total)
}

// rows [i0, i1): what their lines have inside the window [lo, hi) of the file
__global__ __launch_bounds__(256) void k_fai_emit(const FaiFmt q, uint32_t i0, uint32_t i1, uint64_t lo, uint64_t hi, char *__restrict__ out)
{
    const uint32_t i = i0 + blockIdx.x * 256u + threadIdx.x;
    if (i >= i1) return;
    const uint64_t f_lo = q.off[i], f_hi = q.off[i + 1];
    if (f_hi <= lo || f_lo >= hi || f_lo == f_hi) return;
    WinSink w{f_lo, lo, hi, out};
    fai_line(q, i, w);
}

// rows of a file whose records are one line each: in[i] = {sequence bytes, header bytes}; tmp: [n] scratch
__global__ __launch_bounds__(256) void k_fai_scaf_sizes(const uint64_t *__restrict__ in, uint32_t n, uint64_t *__restrict__ tmp)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) tmp[i] = in[2u * i] + in[2u * i + 1u] + 1u;  // header line, sequence, its line end
}
__global__ __launch_bounds__(256) void k_fai_scaf_rows(const uint64_t *__restrict__ in, uint32_t n, const uint64_t *__restrict__ tmp,
                                                       FaiRow *__restrict__ rows)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    FaiRow row;
    row.length = row.linebases = in[2u * i];
    row.linewidth = row.length + 1u;
    row.offset = tmp[i] + in[2u * i + 1u];
    rows[i] = row;
}

static int fai_scan_u64(mxg_handle *h, uint64_t *d_a, uint32_t n)  // d_a[0 .. n) -> exclusive sums, in place (scan64_kernels.h)
{
    const uint32_t n_tiles = (n + PT_TILE - 1) / PT_TILE;
    MXG_HIP(h, h->faibuf[FB_TSUM].ensure((size_t)n_tiles * 8));
    launch_scan_u64(h->stream, d_a, n, h->faibuf[FB_TSUM].as<uint64_t>());
    MXG_HIP(h, hipGetLastError());
    return MXG_OK;
}

// the lines of rows [0, q.n) (q.rows, names and keep in place; q.off is set here) into `of`; *bytes = the file's size
static int fai_emit_rows(mxg_handle *h, FaiFmt q, OutFile &of, const char *who, uint64_t *bytes)
{
    hipStream_t st = h->stream;
    DevBuf *B = h->faibuf;
    *bytes = 0;
    if (!q.n) return MXG_OK;
    const size_t cnt = (size_t)q.n + 1;
    MXG_HIP(h, B[FB_OFF].ensure(cnt * 8));
    q.off = B[FB_OFF].as<uint64_t>();
    hipLaunchKernelGGL(k_fai_len, dim3((uint32_t)((cnt + 255) / 256)), dim3(256), 0, st, q);
    MXG_HIP(h, hipGetLastError());
    int rc;
    if ((rc = fai_scan_u64(h, q.off, q.n + 1)) != MXG_OK) return rc;
    uint64_t total = 0;
    MXG_HIP(h, hipMemcpyAsync(&total, q.off + q.n, 8, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    *bytes = total;
    if (!total) return MXG_OK;
    const uint64_t WIN = std::max<uint64_t>(1, std::min<uint64_t>(knob_u64(h, "MXG_FAI_WIN", PIN_HALF), PIN_HALF));
    const uint64_t n_win = (total + WIN - 1) / WIN;
    if (n_win >= 0xFFFFFFFFull) return set_err(h, MXG_ELIMIT, "%s: %llu windows of MXG_FAI_WIN bytes for '%s'", who, (unsigned long long)n_win, of.path.c_str());
    std::vector<uint32_t> bounds(n_win);
    MXG_HIP(h, B[FB_BOUNDS].ensure(n_win * 4));
    // bounds[c] = the row whose line holds byte c * WIN of the file
    launch_win_bounds(st, q.off, q.n, WIN, (uint32_t)n_win, B[FB_BOUNDS].as<uint32_t>());
    MXG_HIP(h, hipGetLastError());
    MXG_HIP(h, hipMemcpyAsync(bounds.data(), B[FB_BOUNDS].p, n_win * 4, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    const WinFill fill = [&](uint64_t c, unsigned char *d_win, uint64_t lo, uint64_t hi) -> int {
        // (the row that holds byte hi holds byte hi - 1 or follows the row that does; rows without a line lie in between)
        const uint32_t i0 = bounds[c], i1 = c + 1 < n_win ? std::min(q.n, bounds[c + 1] + 1) : q.n;
        hipLaunchKernelGGL(k_fai_emit, dim3((i1 - i0 + 255) / 256), dim3(256), 0, st, q, i0, i1, lo, hi, reinterpret_cast<char *>(d_win));
        MXG_HIP(h, hipGetLastError());
        return MXG_OK;
    };
    return write_windows(h, of, total, WIN, 0, fill, who);
}

// every record's id, one behind the other, on the device
static int fai_upload_ids(mxg_handle *h, const Assembly *a, FaiFmt &q)
{
    const size_t n_rec = a->recs.size();
    std::vector<uint64_t> id_off(n_rec + 1, 0);
    std::string ids;
    for (size_t r = 0; r < n_rec; ++r) {
        ids += a->recs[r].id;
        id_off[r + 1] = ids.size();
    }
    DevBuf *B = h->faibuf;
    MXG_HIP(h, B[FB_IDOFF].ensure((n_rec + 1) * 8));
    MXG_HIP(h, B[FB_IDS].ensure(ids.size() + 16));
    // (pageable memory: the copies return when the bytes have left the vectors)
    MXG_HIP(h, hipMemcpyAsync(B[FB_IDOFF].p, id_off.data(), (n_rec + 1) * 8, hipMemcpyHostToDevice, h->stream));
    if (!ids.empty()) MXG_HIP(h, hipMemcpyAsync(B[FB_IDS].p, ids.data(), ids.size(), hipMemcpyHostToDevice, h->stream));
    MXG_HIP(h, hipStreamSynchronize(h->stream));
    q.id_off = B[FB_IDOFF].as<uint64_t>(), q.ids = B[FB_IDS].as<char>();
    return MXG_OK;
}

int write_gzi(mxg_handle *h, OutFile &of, const std::vector<uint64_t> &comp_off, const std::vector<uint64_t> &text_off)
{
    // little-endian: the count, then {compressed offset, text offset} of every member that holds text but the first
    const size_t n = comp_off.size() > 1 ? comp_off.size() - 1 : 0;
    std::vector<unsigned char> img(8 + 16 * n);
    auto le64 = [&](size_t at, uint64_t v) {
        for (uint32_t u = 0; u < 8; ++u) img[at + u] = (unsigned char)(v >> (8u * u));
    };
    le64(0, n);
    for (size_t j = 0; j < n; ++j) {
        le64(8 + 16 * j, comp_off[j + 1]);
        le64(16 + 16 * j, text_off[j + 1]);
    }
    if (!of.put(reinterpret_cast<const char *>(img.data()), img.size(), 0, host_threads(h))) return set_err(h, MXG_EIO, "write error on '%s'", of.path.c_str());
    return MXG_OK;
}

int write_fai_records(mxg_handle *h, const Assembly *a, OutFile &of, const std::vector<FaiOutRec> &recs, bool ntjoin_names)
{
    const char *who = "mxg_write_scaffolds";
    if (recs.size() >= (1ull << 31)) return set_err(h, MXG_ELIMIT, "%s: %llu records for '%s'", who, (unsigned long long)recs.size(), of.path.c_str());
    const uint32_t n = (uint32_t)recs.size();
    uint64_t bytes = 0;
    if (!n) return MXG_OK;
    hipStream_t st = h->stream;
    DevBuf *B = h->faibuf;
    std::vector<uint64_t> in(2 * (size_t)n);
    std::vector<uint32_t> iv(3 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        in[2 * (size_t)i] = recs[i].len, in[2 * (size_t)i + 1] = recs[i].header_bytes;
        iv[3 * (size_t)i] = recs[i].rec, iv[3 * (size_t)i + 1] = recs[i].lo, iv[3 * (size_t)i + 2] = recs[i].hi;
    }
    FaiFmt q{};
    q.n = n, q.name_kind = ntjoin_names ? FAI_NAME_NTJOIN : FAI_NAME_INTERVAL;
    int rc;
    if (!ntjoin_names && (rc = fai_upload_ids(h, a, q)) != MXG_OK) return rc;
    MXG_HIP(h, B[FB_RLEN].ensure((size_t)n * 16));
    MXG_HIP(h, B[FB_ORG].ensure((size_t)n * 8 + 8));
    MXG_HIP(h, B[FB_ROWS].ensure((size_t)n * sizeof(FaiRow)));
    MXG_HIP(h, B[FB_IV].ensure((size_t)n * 12));
    MXG_HIP(h, hipMemcpyAsync(B[FB_RLEN].p, in.data(), (size_t)n * 16, hipMemcpyHostToDevice, st));
    MXG_HIP(h, hipMemcpyAsync(B[FB_IV].p, iv.data(), (size_t)n * 12, hipMemcpyHostToDevice, st));
    const dim3 grid((n + 255) / 256);
    uint64_t *tmp = B[FB_ORG].as<uint64_t>();
    hipLaunchKernelGGL(k_fai_scaf_sizes, grid, dim3(256), 0, st, B[FB_RLEN].as<uint64_t>(), n, tmp);
    MXG_HIP(h, hipGetLastError());
    if ((rc = fai_scan_u64(h, tmp, n)) != MXG_OK) return rc;
    hipLaunchKernelGGL(k_fai_scaf_rows, grid, dim3(256), 0, st, B[FB_RLEN].as<uint64_t>(), n, tmp, B[FB_ROWS].as<FaiRow>());
    MXG_HIP(h, hipGetLastError());
    MXG_HIP(h, hipStreamSynchronize(st));  // (in and iv have left the host)
    q.rows = B[FB_ROWS].as<FaiRow>();
    q.iv = B[FB_IV].as<uint32_t>();
    return fai_emit_rows(h, q, of, who, &bytes);
}

int write_fai(mxg_handle *h, Assembly *a, int assembly, const char *fai_path, const char *gzi_path)
{
    if (a->holds_pieces || a->shard_lo != 0 || a->shard_hi < a->recs.size())
        return set_err(h, MXG_EINVAL, "mxg_write_fai: assembly %d holds a shard or pieces of its file, not the whole text", assembly);
    if (!(a->text_on_device && a->d_text.p) || a->ing_item0.size() != a->recs.size() + 1)
        return set_err(h, MXG_EINVAL, "mxg_write_fai: assembly %d: the handle does not hold the file's text on the device (a minimizer table from a "
                       "TSV, side-car or arrays, packed bases, MXG_HOST_INGEST=1, plain gzip, a pipe, text dropped by MXG_FLAG_DROP_SEQ or "
                       "released by a one-shot handle): the index is made from the text of the FASTA", assembly);
    if (gzi_path && !a->from_bgzf)
        return set_err(h, MXG_EINVAL, "mxg_write_fai: assembly %d did not come from a BGZF file: it has no .gzi", assembly);
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n_rec = a->recs.size();
    const uint64_t n_items = a->ing_item0.back();
    if (n_rec >= (1ull << 31)) return set_err(h, MXG_ELIMIT, "mxg_write_fai: %llu records (fewer than 2^31)", (unsigned long long)n_rec);
    MXG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    DevBuf *B = h->faibuf;
    FaiFmt q{};
    q.n = (uint32_t)n_rec, q.name_kind = FAI_NAME_ID;
    std::vector<uint8_t> keep(n_rec, 1);
    if (n_rec) {
        // ---- the rows
        if (!a->d_ing_item0.p) {
            MXG_HIP(h, a->d_ing_item0.ensure(a->ing_item0.size() * 8));
            MXG_HIP(h, hipMemcpyAsync(a->d_ing_item0.p, a->ing_item0.data(), a->ing_item0.size() * 8, hipMemcpyHostToDevice, st));
        }
        std::vector<uint64_t> org(n_rec), rlen(n_rec);
        for (size_t r = 0; r < n_rec; ++r) org[r] = a->recs[r].text_off, rlen[r] = a->recs[r].len;
        const uint32_t n_tiles = (uint32_t)((n_items + 255) / 256);
        MXG_HIP(h, B[FB_ORG].ensure(n_rec * 8));
        MXG_HIP(h, B[FB_RLEN].ensure(n_rec * 8));
        MXG_HIP(h, B[FB_ROWS].ensure(n_rec * sizeof(FaiRow)));
        MXG_HIP(h, B[FB_VERDICT].ensure(8));
        MXG_HIP(h, B[FB_SUMS].ensure((size_t)n_items * sizeof(FaiSum) + 16));
        MXG_HIP(h, B[FB_AGG].ensure((size_t)n_tiles * sizeof(FaiSum) + 16));
        MXG_HIP(h, B[FB_EXCL].ensure((size_t)n_tiles * sizeof(FaiSum) + 16));
        MXG_HIP(h, hipMemcpyAsync(B[FB_ORG].p, org.data(), n_rec * 8, hipMemcpyHostToDevice, st));
        MXG_HIP(h, hipMemcpyAsync(B[FB_RLEN].p, rlen.data(), n_rec * 8, hipMemcpyHostToDevice, st));
        MXG_HIP(h, hipMemsetAsync(B[FB_VERDICT].p, 0xFF, 8, st));
        FaiRow *rows = B[FB_ROWS].as<FaiRow>();
        hipLaunchKernelGGL(k_fai_rows_init, dim3((uint32_t)((n_rec + 255) / 256)), dim3(256), 0, st, B[FB_ORG].as<uint64_t>(), (uint64_t)n_rec, rows);
        // MXG_DEBUG_IO: the device time of the pass over the text and its scan (what DESIGN.md 4l sets the report's passes against)
        hipEvent_t ev_rows[2] = {};
        const bool dbg_rows = getenv("MXG_DEBUG_IO") != nullptr && hipEventCreate(&ev_rows[0]) == hipSuccess && hipEventCreate(&ev_rows[1]) == hipSuccess;
        if (dbg_rows) (void)hipEventRecord(ev_rows[0], st);
        if (n_items) {
            FaiSum *sums = B[FB_SUMS].as<FaiSum>(), *agg = B[FB_AGG].as<FaiSum>(), *excl = B[FB_EXCL].as<FaiSum>();
            const IngItem *items = a->d_ing_items.as<IngItem>();
            hipLaunchKernelGGL(k_fai_items, dim3((uint32_t)n_items), dim3(256), 0, st, a->d_text.as<unsigned char>(), a->text_bytes, items,
                               a->d_ing_item0.as<uint64_t>(), sums);
            hipLaunchKernelGGL(k_fai_tile_agg, dim3(n_tiles), dim3(256), 0, st, sums, n_items, agg);
            hipLaunchKernelGGL(k_fai_tile_scan, dim3(1), dim3(256), 0, st, agg, n_tiles, excl);
            hipLaunchKernelGGL(k_fai_rows, dim3(n_tiles), dim3(256), 0, st, sums, excl, items, n_items, B[FB_ORG].as<uint64_t>(),
                               B[FB_RLEN].as<uint64_t>(), (uint64_t)n_rec, rows, B[FB_VERDICT].as<unsigned long long>());
        }
        MXG_HIP(h, hipGetLastError());
        if (dbg_rows) (void)hipEventRecord(ev_rows[1], st);
        unsigned long long bad = 0;
        MXG_HIP(h, hipMemcpyAsync(&bad, B[FB_VERDICT].p, 8, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
        if (dbg_rows) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, ev_rows[0], ev_rows[1]);
            fprintf(stderr, "[mxg] fai items=%llu rows_ms=%.3f\n", (unsigned long long)n_items, ms);
        }
        for (hipEvent_t e : ev_rows)
            if (e) (void)hipEventDestroy(e);
        if (bad != ~0ull) {  // (nothing has been opened)
            if (bad >= n_rec) return set_err(h, MXG_EDEVICE, "internal error: mxg_write_fai: no record %llu", bad);
            FaiRow row;
            MXG_HIP(h, hipMemcpy(&row, rows + bad, sizeof(FaiRow), hipMemcpyDeviceToHost));
            const Record &rec = a->recs[bad];
            if (row.err_at == FAI_INTERNAL)
                return set_err(h, MXG_EDEVICE, "internal error: mxg_write_fai: record '%s' has %llu bases in its lines and %llu in the handle",
                               rec.id.c_str(), (unsigned long long)row.length, (unsigned long long)rec.len);
            return set_err(h, MXG_EINVAL, "mxg_write_fai: record '%s': the line at byte %llu of the text is not what its first line (at byte %llu) "
                           "makes of it -- lines of one width, a last one no longer, no empty line inside, nothing but printable characters "
                           "(samtools faidx: different line length in sequence)", rec.id.c_str(), (unsigned long long)row.err_at,
                           (unsigned long long)rec.text_off);
        }
        // ---- names: the first record of a name is the one the index knows
        std::unordered_set<std::string> seen;
        bool any_dup = false;
        for (size_t r = 0; r < n_rec; ++r)
            if (!seen.insert(a->recs[r].id).second) {
                keep[r] = 0, any_dup = true;
                fprintf(stderr, "[mxg] mxg_write_fai: ignoring duplicate sequence \"%s\" at byte offset %llu\n", a->recs[r].id.c_str(),
                        (unsigned long long)a->recs[r].text_off);
            }
        int rc;
        if ((rc = fai_upload_ids(h, a, q)) != MXG_OK) return rc;
        if (any_dup) {
            MXG_HIP(h, B[FB_KEEP].ensure(n_rec));
            MXG_HIP(h, hipMemcpy(B[FB_KEEP].p, keep.data(), n_rec, hipMemcpyHostToDevice));
            q.keep = B[FB_KEEP].as<uint8_t>();
        }
        q.rows = rows;
    }
    // ---- nothing is refused from here on: the files
    OutFile of, gz;
    if (!of.open(fai_path)) return set_err(h, MXG_EIO, "cannot open '%s' for writing", fai_path);
    if (gzi_path && !gz.open(gzi_path)) return set_err(h, MXG_EIO, "cannot open '%s' for writing", gzi_path);
    uint64_t bytes = 0;
    int rc;
    if ((rc = fai_emit_rows(h, q, of, "mxg_write_fai", &bytes)) != MXG_OK) return rc;
    if (gzi_path && (rc = write_gzi(h, gz, a->bgzf_comp_off, a->bgzf_text_off)) != MXG_OK) return rc;
    MXG_HIP(h, hipStreamSynchronize(st));
    const bool c_of = of.close(), c_gz = gz.close();
    if (!(c_of && c_gz)) return set_err(h, MXG_EIO, "mxg_write_fai: write error while closing the output files");
    of.complete = gz.complete = true;
    if (getenv("MXG_DEBUG_IO"))
        fprintf(stderr, "[mxg] fai records=%llu bytes=%llu ms=%.3f\n", (unsigned long long)n_rec, (unsigned long long)bytes,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return MXG_OK;
}

}  // namespace mxg
