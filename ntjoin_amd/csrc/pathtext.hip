// pathtext.hip -- the .path file and the AGP of all paths, formatted on the device (row f8): what the reference's print_scaffolds
// writes per path with Python strings (bin/ntjoin_assemble.py:605-610), what write_agp (:346-376) parses back out of that string with
// two regular expressions per component, and write_agp_unassigned (:379-404); the coordinates are PathNode.get_adjusted_start /
// get_adjusted_end (bin/path_node.py:41-61).  The contract is in include/ntjoin_mx.h (mxg_write_paths) and, executable, in
// tests/_path_text_restatement.py.
//
// The unit of work is a node.  Its text is a FRAGMENT of either file: in the .path file `[ntJoin<p>\t]id ori:s-e` and ` <gap>N ` or,
// behind a path's last node, the line end; in the AGP its W line and, unless it is the last node, the N line of the gap behind it.
// One formatter per fragment (pt_path_frag, pt_agp_frag) runs twice over a sink (text_dev.h): CountSink adds up the bytes, WinSink
// stores those that fall into the window at hand -- the two passes cannot disagree about a length.
//
//   k_pt_nodes   per node: its path (bisection over path_first), the strips of an end node, the adjusted interval [s, e), the
//                refusals (the lowest offending node wins, through one atomicMin), and the length of its components e - s + gap.
//   scan         an exclusive 64-bit sum over all nodes (tile sums -> one block over the tile sums -> tiles).  The scan segmented by
//                path is the difference of two entries: at = 1 + S[i] - S[path_first[p]], modulo 2^64, so a path may lie in any
//                number of tiles and the sum over ALL paths may wrap; part = 2 j + 1 for node j of its path.
//   k_pt_len     per node: bytes of its two fragments from decimal digit counts (they need `at`, hence the second pass);
//                two more scans turn them into file offsets.
//   k_win_bounds per window: the node that holds the window's first byte (bisection over the offsets; win_out.hip).
//   k_pt_emit    per node of a window: the fragment's bytes that fall into [lo, hi).  A long id is a loop of one lane.
// Output leaves window by window through write_windows (win_out.hip); MXG_PATH_WIN sets the bytes per window.
// The first line of the .path file and the AGP's unassigned lines (one per interval, from the handle's copy of the last
// mxg_write_scaffolds' intervals) are the host's.
#include <algorithm>
#include <string>

#include "bisect.h"
#include "mxg_internal.h"
#include "scan64_kernels.h"
#include "text_dev.h"

namespace mxg {

enum { PT_NODES, PT_FIRST, PT_LEAD, PT_TAIL, PT_IDOFF, PT_IDS, PT_SUM, PT_POFF, PT_AOFF, PT_TSUM, PT_ERR, PT_BOUNDS, PT_BUF_COUNT };
static_assert(PT_BUF_COUNT <= 16, "mxg_handle::ptbuf too small");
enum : uint32_t { PT_BAD_SEGMENT = 1, PT_BAD_END_ADJUST = 2, PT_BAD_RECORD = 3, PT_BAD_INTERVAL = 4 };

struct PtParams {
    const mxg_scaffold_node *nodes;
    const uint64_t *path_first;  // [n_paths + 1]
    const uint32_t *lead, *tail;  // [n_paths]
    const uint64_t *id_off;      // [n_rec + 1] into ids
    const char *ids;
    uint64_t *sum;   // [n + 1] component lengths, then their exclusive sums
    uint64_t *poff;  // [n + 1] bytes of the .path fragments, then their offsets
    uint64_t *aoff;  // [n + 1] the same for the AGP
    unsigned long long *err;  // (node << 3 | reason) of the lowest node refused
    uint64_t n_paths;
    uint32_t n, n_rec;
};

struct PtNode {
    uint64_t p;       // the node's path
    uint32_t j, m;    // node j of m
    int64_t s, e;     // the adjusted interval
    uint32_t gap, rec, reverse, bad;
};

__device__ __forceinline__ PtNode pt_node(const PtParams &q, uint32_t i)
{
    PtNode nd;
    const uint64_t lo = last_le(q.path_first, (uint64_t)0, q.n_paths, i);  // path_first[lo] <= i < path_first[lo + 1]
    const uint64_t f0 = q.path_first[lo], f1 = q.path_first[lo + 1];
    nd.p = lo, nd.j = (uint32_t)(i - f0), nd.m = (uint32_t)(f1 - f0);
    const mxg_scaffold_node in = q.nodes[i];
    nd.gap = in.gap_size, nd.rec = in.record, nd.reverse = in.reverse ? 1u : 0u, nd.bad = 0, nd.s = 0, nd.e = 0;
    if (in.record >= q.n_rec) nd.bad = PT_BAD_RECORD;
    else if (in.start >= in.end) nd.bad = PT_BAD_SEGMENT;
    else if (in.end_adjust > in.end - in.start) nd.bad = PT_BAD_END_ADJUST;
    if (nd.bad) return nd;
    int64_t start = in.start, end = in.end;
    if (nd.j == 0) {  // join_sequences :413-436: the first node loses the lead at its left in output orientation
        if (nd.reverse) end -= q.lead[lo]; else start += q.lead[lo];
    }
    if (nd.j + 1 == nd.m) {
        if (nd.reverse) start += q.tail[lo]; else end -= q.tail[lo];
    }
    const int64_t L = end - start, ea = in.end_adjust ? (int64_t)in.end_adjust : L, sa = in.start_adjust;
    nd.s = nd.reverse ? start + (L - ea) : start + sa;
    nd.e = nd.reverse ? end - sa : end - (L - ea);
    if (nd.s < 0 || nd.s >= nd.e) nd.bad = PT_BAD_INTERVAL;
    return nd;
}

// a record's id into either sink (text_dev.h)
template <class Sink> __device__ __forceinline__ void pt_id(const PtParams &q, uint32_t r, Sink &o)
{
    o.bytes(q.ids + q.id_off[r], q.id_off[r + 1] - q.id_off[r]);
}

#define PT_LIT(o, s) (o).lit(s, (uint32_t)sizeof(s) - 1u)

template <class Sink> __device__ __forceinline__ void pt_path_frag(const PtParams &q, const PtNode &nd, Sink &o)
{
    if (nd.j == 0) {
        PT_LIT(o, "ntJoin");
        o.num(nd.p);
        o.ch('\t');
    }
    pt_id(q, nd.rec, o);
    o.ch(nd.reverse ? '-' : '+');
    o.ch(':');
    o.num((uint64_t)nd.s);
    o.ch('-');
    o.num((uint64_t)nd.e);
    if (nd.j + 1 < nd.m) {
        o.ch(' ');
        o.num(nd.gap);
        PT_LIT(o, "N ");
    } else {
        o.ch('\n');  // (the last node's gap is left out, whatever it is)
    }
}

template <class Sink> __device__ __forceinline__ void pt_agp_frag(const PtParams &q, const PtNode &nd, uint64_t at, Sink &o)
{
    const uint64_t n = (uint64_t)(nd.e - nd.s), part = 2ull * nd.j + 1;
    PT_LIT(o, "ntJoin");
    o.num(nd.p);
    o.ch('\t');
    o.num(at);
    o.ch('\t');
    o.num(at + n - 1);
    o.ch('\t');
    o.num(part);
    PT_LIT(o, "\tW\t");
    pt_id(q, nd.rec, o);
    o.ch('\t');
    o.num((uint64_t)nd.s + 1);
    o.ch('\t');
    o.num((uint64_t)nd.e);
    o.ch('\t');
    o.ch(nd.reverse ? '-' : '+');
    o.ch('\n');
    if (nd.j + 1 == nd.m) return;
    const uint64_t at2 = at + n;  // (>= 2: a gap of 0 writes at2 - 1 as its end, as the reference does)
    PT_LIT(o, "ntJoin");
    o.num(nd.p);
    o.ch('\t');
    o.num(at2);
    o.ch('\t');
    o.num(at2 + nd.gap - 1);
    o.ch('\t');
    o.num(part + 1);
    PT_LIT(o, "\tN\t");
    o.num(nd.gap);
    PT_LIT(o, "\tscaffold\tyes\talign_genus\n");
}

__global__ __launch_bounds__(256) void k_pt_nodes(const PtParams q)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > q.n) return;
    uint64_t c = 0;
    if (i < q.n) {
        const PtNode nd = pt_node(q, i);
        if (nd.bad) atomicMin(q.err, (unsigned long long)i << 3 | nd.bad);
        else c = (uint64_t)(nd.e - nd.s) + nd.gap;
    }
    q.sum[i] = c;  // (entry n: 0, so that the exclusive sums end with the total)
}

__global__ __launch_bounds__(256) void k_pt_len(const PtParams q)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > q.n) return;
    CountSink pc, ac;
    if (i < q.n) {
        const PtNode nd = pt_node(q, i);
        pt_path_frag(q, nd, pc);
        pt_agp_frag(q, nd, 1 + q.sum[i] - q.sum[i - nd.j], ac);
    }
    q.poff[i] = pc.n;
    q.aoff[i] = ac.n;
}

// nodes [i0, i1): what their fragments have inside the window [lo, hi) of the .path file (agp = 0) or the AGP (agp = 1)
__global__ __launch_bounds__(256) void k_pt_emit(const PtParams q, uint32_t agp, uint32_t i0, uint32_t i1, uint64_t lo, uint64_t hi,
                                                 char *__restrict__ out)
{
    const uint32_t i = i0 + blockIdx.x * 256u + threadIdx.x;
    if (i >= i1) return;
    const uint64_t *off = agp ? q.aoff : q.poff;
    const uint64_t f_lo = off[i], f_hi = off[i + 1];
    if (f_hi <= lo || f_lo >= hi) return;
    const PtNode nd = pt_node(q, i);
    WinSink w{f_lo, lo, hi, out};
    if (agp) pt_agp_frag(q, nd, 1 + q.sum[i] - q.sum[i - nd.j], w);
    else pt_path_frag(q, nd, w);
}

static int pt_scan(mxg_handle *h, uint64_t *d_a, uint32_t n)  // d_a[0 .. n) -> exclusive sums, in place
{
    launch_scan_u64(h->stream, d_a, n, h->ptbuf[PT_TSUM].as<uint64_t>());
    MXG_HIP(h, hipGetLastError());
    return MXG_OK;
}

// the fragments of one file into `of` behind its first `base` bytes, window by window
static int pt_emit_file(mxg_handle *h, const PtParams &q, uint32_t agp, uint64_t total, OutFile &of, uint64_t base, uint64_t WIN)
{
    if (!total) return MXG_OK;
    hipStream_t st = h->stream;
    const uint64_t n_win = (total + WIN - 1) / WIN;
    if (n_win >= 0xFFFFFFFFull) return set_err(h, MXG_ELIMIT, "mxg_write_paths: %llu windows of MXG_PATH_WIN bytes for '%s'", (unsigned long long)n_win, of.path.c_str());
    std::vector<uint32_t> bounds(n_win);
    MXG_HIP(h, h->ptbuf[PT_BOUNDS].ensure(n_win * 4));
    // bounds[c] = the node whose fragment holds byte c * WIN of the file
    launch_win_bounds(st, agp ? q.aoff : q.poff, q.n, WIN, (uint32_t)n_win, h->ptbuf[PT_BOUNDS].as<uint32_t>());
    MXG_HIP(h, hipGetLastError());
    MXG_HIP(h, hipMemcpyAsync(bounds.data(), h->ptbuf[PT_BOUNDS].p, n_win * 4, hipMemcpyDeviceToHost, st));
    MXG_HIP(h, hipStreamSynchronize(st));
    const WinFill fill = [&](uint64_t c, unsigned char *d_win, uint64_t lo, uint64_t hi) -> int {
        // (the node that holds byte hi holds byte hi - 1 or follows the node that does)
        const uint32_t i0 = bounds[c], i1 = c + 1 < n_win ? std::min(q.n, bounds[c + 1] + 1) : q.n;
        hipLaunchKernelGGL(k_pt_emit, dim3((i1 - i0 + 255) / 256), dim3(256), 0, st, q, agp, i0, i1, lo, hi, reinterpret_cast<char *>(d_win));
        MXG_HIP(h, hipGetLastError());
        return MXG_OK;
    };
    return write_windows(h, of, total, WIN, base, fill, "mxg_write_paths");
}

int write_paths(mxg_handle *h, Assembly *a, int assembly, const mxg_scaffold_node *nodes, const uint64_t *path_first, uint64_t n_paths,
                const uint32_t *lead_strip, const uint32_t *tail_strip, const char *first_line, const char *path_file, const char *agp_file,
                uint32_t flags)
{
    const uint64_t n_nodes = n_paths ? path_first[n_paths] : 0;
    if (n_nodes >= (1ull << 31)) return set_err(h, MXG_ELIMIT, "mxg_write_paths: %llu nodes (fewer than 2^31)", (unsigned long long)n_nodes);
    if (path_first[0] != 0) return set_err(h, MXG_EINVAL, "mxg_write_paths: path_first[0] is %llu, not 0", (unsigned long long)path_first[0]);
    for (uint64_t p = 0; p < n_paths; ++p) {
        const uint64_t lo = path_first[p], hi = path_first[p + 1];
        if (hi < lo || hi > n_nodes) return set_err(h, MXG_EINVAL, "mxg_write_paths: path_first is not increasing at path %llu", (unsigned long long)p);
        if (hi - lo < 2)
            return set_err(h, MXG_EINVAL, "mxg_write_paths: path %llu has %llu node(s); a path has at least two (the reference leaves shorter ones out)",
                           (unsigned long long)p, (unsigned long long)(hi - lo));
    }
    const bool with_un = (flags & MXG_PATHS_AGP_UNASSIGNED) != 0;
    if (with_un && h->scaf_iv_asm != assembly)
        return set_err(h, MXG_EINVAL, "mxg_write_paths: MXG_PATHS_AGP_UNASSIGNED needs the unassigned intervals of assembly %d, which only an "
                       "mxg_write_scaffolds of this handle that computed the unassigned side leaves behind", assembly);
    const size_t n_rec = a->recs.size();
    const uint32_t n = (uint32_t)n_nodes;
    MXG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    DevBuf *B = h->ptbuf;
    PtParams q{};
    uint64_t path_bytes = 0, agp_bytes = 0;
    if (n) {
        // ---- nodes, strips and ids on the device
        std::vector<uint64_t> id_off(n_rec + 1, 0);
        std::string ids;
        for (size_t r = 0; r < n_rec; ++r) {
            ids += a->recs[r].id;
            id_off[r + 1] = ids.size();
        }
        const size_t cnt = (size_t)n + 1, n_tiles = (cnt + PT_TILE - 1) / PT_TILE;
        MXG_HIP(h, B[PT_NODES].ensure((size_t)n * sizeof(mxg_scaffold_node)));
        MXG_HIP(h, B[PT_FIRST].ensure((n_paths + 1) * 8));
        MXG_HIP(h, B[PT_LEAD].ensure(n_paths * 4));
        MXG_HIP(h, B[PT_TAIL].ensure(n_paths * 4));
        MXG_HIP(h, B[PT_IDOFF].ensure((n_rec + 1) * 8));
        MXG_HIP(h, B[PT_IDS].ensure(ids.size() + 16));
        MXG_HIP(h, B[PT_SUM].ensure(cnt * 8));
        MXG_HIP(h, B[PT_POFF].ensure(cnt * 8));
        MXG_HIP(h, B[PT_AOFF].ensure(cnt * 8));
        MXG_HIP(h, B[PT_TSUM].ensure(n_tiles * 8));
        MXG_HIP(h, B[PT_ERR].ensure(8));
        MXG_HIP(h, hipMemcpyAsync(B[PT_NODES].p, nodes, (size_t)n * sizeof(mxg_scaffold_node), hipMemcpyHostToDevice, st));
        MXG_HIP(h, hipMemcpyAsync(B[PT_FIRST].p, path_first, (n_paths + 1) * 8, hipMemcpyHostToDevice, st));
        if (lead_strip) MXG_HIP(h, hipMemcpyAsync(B[PT_LEAD].p, lead_strip, n_paths * 4, hipMemcpyHostToDevice, st));
        else MXG_HIP(h, hipMemsetAsync(B[PT_LEAD].p, 0, n_paths * 4, st));
        if (tail_strip) MXG_HIP(h, hipMemcpyAsync(B[PT_TAIL].p, tail_strip, n_paths * 4, hipMemcpyHostToDevice, st));
        else MXG_HIP(h, hipMemsetAsync(B[PT_TAIL].p, 0, n_paths * 4, st));
        MXG_HIP(h, hipMemcpyAsync(B[PT_IDOFF].p, id_off.data(), (n_rec + 1) * 8, hipMemcpyHostToDevice, st));
        if (!ids.empty()) MXG_HIP(h, hipMemcpyAsync(B[PT_IDS].p, ids.data(), ids.size(), hipMemcpyHostToDevice, st));
        MXG_HIP(h, hipMemsetAsync(B[PT_ERR].p, 0xFF, 8, st));
        q.nodes = B[PT_NODES].as<mxg_scaffold_node>();
        q.path_first = B[PT_FIRST].as<uint64_t>();
        q.lead = B[PT_LEAD].as<uint32_t>(), q.tail = B[PT_TAIL].as<uint32_t>();
        q.id_off = B[PT_IDOFF].as<uint64_t>(), q.ids = B[PT_IDS].as<char>();
        q.sum = B[PT_SUM].as<uint64_t>(), q.poff = B[PT_POFF].as<uint64_t>(), q.aoff = B[PT_AOFF].as<uint64_t>();
        q.err = B[PT_ERR].as<unsigned long long>();
        q.n_paths = n_paths, q.n = n, q.n_rec = (uint32_t)std::min<size_t>(n_rec, 0xFFFFFFFFull);
        // ---- intervals and refusals; component sums; fragment lengths; file offsets
        const dim3 grid((uint32_t)((cnt + 255) / 256));
        hipLaunchKernelGGL(k_pt_nodes, grid, dim3(256), 0, st, q);
        MXG_HIP(h, hipGetLastError());
        unsigned long long err = 0;
        MXG_HIP(h, hipMemcpyAsync(&err, q.err, 8, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
        if (err != ~0ull) {  // (a refused node has no interval to take lengths of: nothing beyond this point runs)
            const uint64_t i = err >> 3;
            const uint64_t p = (uint64_t)(std::upper_bound(path_first, path_first + n_paths + 1, i) - path_first) - 1;
            const unsigned long long up = p, un = i - path_first[p];
            const mxg_scaffold_node &in = nodes[i];
            switch (err & 7u) {
            case PT_BAD_RECORD: return set_err(h, MXG_EINVAL, "mxg_write_paths: path %llu node %llu: no record %u", up, un, in.record);
            case PT_BAD_SEGMENT: return set_err(h, MXG_EINVAL, "mxg_write_paths: path %llu node %llu: [%u, %u) is not a segment", up, un, in.start, in.end);
            case PT_BAD_END_ADJUST:
                return set_err(h, MXG_EINVAL, "mxg_write_paths: path %llu node %llu: end_adjust %u is beyond the segment's %u bases", up, un,
                               in.end_adjust, in.end - in.start);
            default:
                return set_err(h, MXG_EINVAL, "mxg_write_paths: path %llu node %llu: the adjusted interval is empty or inverted after the cuts "
                               "(start_adjust %u, end_adjust %u) and the strips", up, un, in.start_adjust, in.end_adjust);
            }
        }
        int rc;
        if ((rc = pt_scan(h, q.sum, n + 1)) != MXG_OK) return rc;
        hipLaunchKernelGGL(k_pt_len, grid, dim3(256), 0, st, q);
        MXG_HIP(h, hipGetLastError());
        if ((rc = pt_scan(h, q.poff, n + 1)) != MXG_OK) return rc;
        if ((rc = pt_scan(h, q.aoff, n + 1)) != MXG_OK) return rc;
        MXG_HIP(h, hipMemcpyAsync(&path_bytes, q.poff + n, 8, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipMemcpyAsync(&agp_bytes, q.aoff + n, 8, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
    }
    // ---- nothing is refused from here on: the files
    const uint64_t WIN = std::max<uint64_t>(1, std::min<uint64_t>(knob_u64(h, "MXG_PATH_WIN", PIN_HALF), PIN_HALF));
    OutFile pf, af;
    if (!pf.open(path_file)) return set_err(h, MXG_EIO, "cannot open '%s' for writing", path_file);
    if (agp_file && !af.open(agp_file)) return set_err(h, MXG_EIO, "cannot open '%s' for writing", agp_file);
    const std::string head = std::string(first_line ? first_line : "") + "\n";
    if (!pf.put(head.data(), head.size(), 0, host_threads(h))) return set_err(h, MXG_EIO, "write error on '%s'", path_file);
    int rc;
    if ((rc = pt_emit_file(h, q, 0u, path_bytes, pf, head.size(), WIN)) != MXG_OK) return rc;
    if (agp_file) {
        if ((rc = pt_emit_file(h, q, 1u, agp_bytes, af, 0, WIN)) != MXG_OK) return rc;
        if (with_un) {  // write_agp_unassigned :379-404: every interval that keeps text behind its strips
            std::string un;
            for (const mxg_handle::ScafInterval &iv : h->scaf_iv) {
                const int64_t len = (int64_t)iv.hi - iv.lo - iv.lead - iv.tail;
                if (len <= 0) continue;
                const std::string &id = a->recs[iv.rec].id;
                const uint64_t first = (uint64_t)iv.lo + 1 + iv.lead;
                un += id + ":" + std::to_string(iv.lo) + "-" + std::to_string(iv.hi) + "\t1\t" + std::to_string(len) + "\t1\tW\t" + id + "\t" +
                      std::to_string(first) + "\t" + std::to_string(first + (uint64_t)len - 1) + "\t+\n";
            }
            if (!af.put(un.data(), un.size(), agp_bytes, host_threads(h))) return set_err(h, MXG_EIO, "write error on '%s'", agp_file);
        }
    }
    const bool c_pf = pf.close(), c_af = af.close();
    if (!(c_pf && c_af)) return set_err(h, MXG_EIO, "mxg_write_paths: write error while closing the output files");
    pf.complete = af.complete = true;
    return MXG_OK;
}

}  // namespace mxg
