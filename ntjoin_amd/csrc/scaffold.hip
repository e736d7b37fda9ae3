// scaffold.hip -- the scaffold FASTA of all paths and the unassigned rest, written from the text the handle holds (row f6):
// what the reference's print_scaffolds loop does per path with Python strings after reading the target FASTA a second time
// (bin/ntjoin_assemble.py:580-613; get_fasta_segment :327-332, get_adjusted_sequence :519-527, join_sequences :407-439), and
// what print_unassigned (:628-658) does with `bedtools complement` and `bedtools getfasta`.  The contract is in
// include/ntjoin_mx.h (mxg_write_scaffolds) and, executable, in tests/_scaffold_restatement.py.
//
// The unit of work is a byte of output.  The host turns nodes and intervals into a PIECE TABLE {output offset, kind, source}:
// header literals, runs of N, and stretches of a record's text read forwards or backwards (reverse complement); offsets are
// prefix sums of the pieces' lengths, so every output byte has a known place before anything is written.
//
//   k_scaf_ends  one wave per end to strip (two per path, two per unassigned interval): from the end's first base inwards, 64
//                text bytes per step, a ballot finds the first byte that is neither N/n nor a line end.  An N run of megabases
//                is a loop of one wave.  The counts go back to the host, which shortens the first and last text pieces (and
//                refuses a path whose first or last text part is N throughout) before the offsets are laid out.
//   k_scaf_emit  one work-group per tile of SCAF_TILE OUTPUT bytes.  It finds its first piece by bisection and walks the
//                pieces that reach into the tile.  A text piece locates its first source byte (text_of_base over the tile
//                index of a device-ingested file; offset arithmetic for host-ingested text), then streams chunks of 4096
//                source bytes, 16 per thread in one load; line ends are squeezed out by ranking the kept bytes (a count per
//                thread, an exclusive scan over the group), and the bytes go through a 256-entry table in LDS (identity,
//                complement, each with or without case folding) into the tile's image in LDS.  The reverse direction reads the
//                chunks mirrored.  The image leaves with 16-byte stores.
// Output leaves window by window through write_windows (win_out.hip); MXG_SCAF_WIN sets the window size.  With MXG_SCAF_BGZF the
// windows are deflated on the device into BGZF members on their way out (bgzf_deflate.hip) and the host writes the compressed bytes.
#include <algorithm>
#include <string>

#include "bisect.h"
#include "mxg_internal.h"
#include "scan_kernels.h"
#include "text_index.h"

namespace mxg {

constexpr uint32_t SCAF_TILE = 8192;   // output bytes per work-group of k_scaf_emit
constexpr uint32_t SCAF_CHUNK = 4096;  // source bytes per step of a text piece (16 per thread)
enum : uint32_t { SP_LIT = 0, SP_FILL = 1, SP_FWD = 2, SP_REV = 3 };
enum { SC_PIECES, SC_LITS, SC_ORG, SC_ENDS, SC_CNT, SC_BUF_COUNT };
static_assert(SC_BUF_COUNT <= 8, "mxg_handle::scbuf too small");

struct ScafPiece {
    uint64_t out;  // offset of the piece's first output byte; it ends where the next piece begins
    uint64_t src;  // SP_LIT: offset into the literals; SP_FWD / SP_REV: base of the record that gives the first output byte
    uint32_t rec;
    uint32_t kind;
};

struct ScafEnd {
    uint32_t rec, lo, hi;  // bases [lo, hi) of the record
    uint32_t from_high;    // 0: count N from lo upwards, 1: from hi - 1 downwards
};

struct ScafText {
    const unsigned char *text;
    uint64_t text_bytes;      // bytes that may be read (the allocation, whole chunks)
    TextIndex ix;             // indexed: the file's text with line ends and its tile index
    const uint64_t *rec_org;  // flat: offset of every record's base 0 in text
    uint32_t indexed;
};

__device__ __forceinline__ uint64_t scaf_byte(const ScafText &t, uint32_t r, uint64_t pos)
{
    return t.indexed ? text_of_base(t.ix, r, (uint32_t)pos) : t.rec_org[r] + pos;
}

__global__ __launch_bounds__(64) void k_scaf_ends(const ScafText t, const ScafEnd *__restrict__ ends, uint32_t *__restrict__ count)
{
    const ScafEnd e = ends[blockIdx.x];
    const uint32_t lane = threadIdx.x, len = e.hi - e.lo;
    uint64_t a = scaf_byte(t, e.rec, e.from_high ? e.hi - 1 : e.lo);  // (every lane: the same loads)
    uint32_t cnt = 0;
    while (cnt < len) {
        unsigned char b = '>';  // (outside the text: stops the walk)
        if (e.from_high) {
            if (a >= lane) b = t.text[a - lane];
        } else if (a + lane < t.text_bytes) {
            b = t.text[a + lane];
        }
        const bool is_n = (b | 0x20u) == 'n';
        const bool skip = t.indexed && (b == '\n' || b == '\r');
        const uint64_t stop = __ballot(!is_n && !skip), ns = __ballot(is_n);
        if (stop) {
            const uint32_t f = (uint32_t)__ffsll((unsigned long long)stop) - 1u;
            cnt += (uint32_t)__popcll(ns & ((1ull << f) - 1ull));
            break;
        }
        cnt += (uint32_t)__popcll(ns);
        if (e.from_high) {
            if (a < 64) break;
            a -= 64;
        } else {
            a += 64;
        }
    }
    if (lane == 0) count[blockIdx.x] = min(cnt, len);  // (a run of N may go on beyond the range)
}

__device__ __forceinline__ unsigned char scaf_complement(unsigned char c)
{
    const char *from = "ACGTUNMRWSYKVHDBacgtunmrwsykvhdb", *to = "TGCAANKYWSRMBDHVtgcaankywsrmbdhv";
    for (uint32_t u = 0; u < 32; ++u)
        if ((unsigned char)from[u] == c) return (unsigned char)to[u];
    return c;
}

__global__ __launch_bounds__(256) void k_scaf_emit(const ScafText t, const ScafPiece *__restrict__ pieces, uint32_t n_pieces,
                                                   const unsigned char *__restrict__ lits, uint32_t fold, unsigned char *__restrict__ out,
                                                   uint64_t win_lo, uint64_t win_hi)
{
    __shared__ __attribute__((aligned(16))) unsigned char tile[SCAF_TILE];
    __shared__ unsigned char tab[512];  // [0, 256): forward, [256, 512): complement
    __shared__ uint32_t sh[256];
    __shared__ uint64_t s_a;
    const uint32_t tid = threadIdx.x;
    {
        const unsigned char c = (unsigned char)tid, cc = scaf_complement(c);
        tab[tid] = fold && c >= 'a' && c <= 'z' ? c - 32 : c;
        tab[256 + tid] = fold && cc >= 'a' && cc <= 'z' ? cc - 32 : cc;
    }
    const uint64_t t_lo = win_lo + (uint64_t)blockIdx.x * SCAF_TILE, t_hi = min(win_hi, t_lo + SCAF_TILE);
    // the last piece that begins at or before t_lo (pieces[0].out = 0; pieces of no length are passed over)
    const uint32_t first = last_where(0u, n_pieces, [&](uint32_t i) { return pieces[i].out <= t_lo; });
    __syncthreads();
    for (uint32_t pi = first; pi < n_pieces; ++pi) {
        const ScafPiece pc = pieces[pi];
        if (pc.out >= t_hi) break;
        const uint64_t o_lo = max(pc.out, t_lo), o_hi = min(pieces[pi + 1].out, t_hi);  // (pieces[n_pieces].out = the file's size)
        if (o_lo >= o_hi) continue;
        const uint32_t n = (uint32_t)(o_hi - o_lo), at = (uint32_t)(o_lo - t_lo);
        const uint64_t d = o_lo - pc.out;  // output bytes of the piece in front of this tile
        if (pc.kind == SP_LIT) {
            for (uint32_t u = tid; u < n; u += 256) tile[at + u] = lits[pc.src + d + u];
            continue;
        }
        if (pc.kind == SP_FILL) {
            for (uint32_t u = tid; u < n; u += 256) tile[at + u] = 'N';
            continue;
        }
        const bool rev = pc.kind == SP_REV;
        if (tid == 0) s_a = scaf_byte(t, pc.rec, rev ? pc.src - d : pc.src + d);
        __syncthreads();
        const uint64_t a = s_a;  // source byte of output byte o_lo
        const unsigned char *map = tab + (rev ? 256 : 0);
        uint64_t chunk = a & ~(uint64_t)(SCAF_CHUNK - 1);
        uint32_t done = 0;
        while (done < n && chunk < t.text_bytes) {  // (the text is allocated in whole chunks)
            // thread order = output order: forwards thread 0 holds the chunk's lowest bytes, backwards its highest
            const uint64_t b0 = chunk + 16u * (rev ? 255u - tid : tid);
            uint32_t w[4] = {0, 0, 0, 0}, keep = 0;
            if (rev ? b0 <= a : b0 + 16 > a) {
                const uint4 v = *reinterpret_cast<const uint4 *>(t.text + b0);
                w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
#pragma unroll
                for (uint32_t j = 0; j < 16; ++j) {
                    const uint32_t b = (w[j >> 2] >> (8u * (j & 3u))) & 255u;
                    const bool in = rev ? b0 + j <= a : b0 + j >= a;
                    if (in && !(t.indexed && (b == '\n' || b == '\r'))) keep |= 1u << j;
                }
            }
            uint32_t pos = done + block_exclusive_256((uint32_t)__popc(keep), sh);
            const uint32_t total = sh[255];
#pragma unroll
            for (uint32_t u = 0; u < 16; ++u) {
                const uint32_t j = rev ? 15u - u : u;
                if ((keep >> j & 1u) && pos < n) tile[at + pos] = map[(w[j >> 2] >> (8u * (j & 3u))) & 255u];
                pos += keep >> j & 1u;
            }
            done += total;  // (block-uniform)
            if (rev) {
                if (chunk == 0) break;
                chunk -= SCAF_CHUNK;
            } else {
                chunk += SCAF_CHUNK;
            }
        }
        __syncthreads();  // s_a and sh are free for the next piece
    }
    __syncthreads();
    const uint32_t len = (uint32_t)(t_hi - t_lo);
    unsigned char *dst = out + (t_lo - win_lo);  // (a multiple of SCAF_TILE into a device allocation: 16-byte aligned)
    for (uint32_t u = 16u * tid; u < len; u += 16u * 256u) {
        if (u + 16 <= len) {
            *reinterpret_cast<uint4 *>(dst + u) = *reinterpret_cast<const uint4 *>(tile + u);
        } else {
            for (uint32_t v = u; v < len; ++v) dst[v] = tile[v];
        }
    }
}

namespace {

struct PieceTable {
    std::vector<ScafPiece> pieces;
    std::string lits;
    uint64_t total = 0;
    void add(uint32_t kind, uint64_t len, uint64_t src = 0, uint32_t rec = 0)
    {
        if (!len) return;
        pieces.push_back(ScafPiece{total, src, rec, kind});
        total += len;
    }
    void literal(const std::string &s)
    {
        add(SP_LIT, s.size(), lits.size());
        lits += s;
    }
    // o's pieces behind this table's, their offsets moved (before o gets its end piece: scaf_emit_file)
    void append(const PieceTable &o)
    {
        for (const ScafPiece &pc : o.pieces) pieces.push_back(ScafPiece{pc.out + total, pc.kind == SP_LIT ? pc.src + lits.size() : pc.src, pc.rec, pc.kind});
        lits += o.lits;
        total += o.total;
    }
};

}  // namespace

// the table's bytes into `of`, window by window
// (bgzf_P: 0, or the file is a BGZF file of that many text bytes a member, deflated on the device: bgzf_deflate.hip)
// (member_off, if given: where every BGZF member that holds text starts in the file)
// (report: MXG_SCAF_REPORT -- every window goes through report.hip's passes behind k_scaf_emit; n_records: the file's)
static int scaf_emit_file(mxg_handle *h, const ScafText &t, PieceTable &pt, uint32_t fold, OutFile &of, uint64_t WIN, uint32_t bgzf_P,
                          std::vector<uint64_t> *member_off = nullptr, bool report = false, uint64_t n_records = 0)
{
    hipStream_t st = h->stream;
    DevBuf *B = h->scbuf;
    const uint64_t total = pt.total;
    const size_t n_pieces = pt.pieces.size();
    if (n_pieces >= 0xFFFFFFFFull) return set_err(h, MXG_ELIMIT, "mxg_write_scaffolds: too many pieces of output for one call");
    const char *who = "mxg_write_scaffolds";
    if (report) {  // the piece table as the report reads it: where sequence is, and where a header begins
        std::vector<RepSeg> segs;
        segs.reserve(n_pieces + 1);
        for (const ScafPiece &pc : pt.pieces)
            segs.push_back(RepSeg{pc.out, pc.kind != SP_LIT ? 0u : pt.lits[pc.src] == '>' ? 2u : 1u, 0u});
        if (total) segs.push_back(RepSeg{total, 1u, 0u});
        const int rc = report_file_begin(h, segs, n_records);
        if (rc != MXG_OK) return rc;
    }
    if (!total) return bgzf_P ? bgzf_write_windows(h, of, 0, WIN, bgzf_P, WinFill(), who) : MXG_OK;
    pt.pieces.push_back(ScafPiece{total, 0, 0, SP_LIT});  // (the end of the last piece)
    MXG_HIP(h, B[SC_PIECES].ensure((n_pieces + 1) * sizeof(ScafPiece)));
    MXG_HIP(h, B[SC_LITS].ensure(pt.lits.size() + 16));
    MXG_HIP(h, hipMemcpyAsync(B[SC_PIECES].p, pt.pieces.data(), (n_pieces + 1) * sizeof(ScafPiece), hipMemcpyHostToDevice, st));
    if (!pt.lits.empty()) MXG_HIP(h, hipMemcpyAsync(B[SC_LITS].p, pt.lits.data(), pt.lits.size(), hipMemcpyHostToDevice, st));
    const WinFill fill = [&](uint64_t, unsigned char *d_win, uint64_t lo, uint64_t hi) -> int {
        hipLaunchKernelGGL(k_scaf_emit, dim3((uint32_t)((hi - lo + SCAF_TILE - 1) / SCAF_TILE)), dim3(256), 0, st, t, B[SC_PIECES].as<ScafPiece>(),
                           (uint32_t)n_pieces, B[SC_LITS].as<unsigned char>(), fold, d_win, lo, hi);
        MXG_HIP(h, hipGetLastError());
        return report ? report_file_window(h, d_win, lo, hi) : MXG_OK;
    };
    if (bgzf_P) return bgzf_write_windows(h, of, total, bgzf_window_bytes(WIN, SCAF_TILE, bgzf_P), bgzf_P, fill, who, member_off);
    return write_windows(h, of, total, WIN, 0, fill, who);
}

// MXG_SCAF_KEEP: the combined table (the assigned file's pieces, then the unassigned file's) emitted straight into the handle's
// resident buffer: SCAF_TILE alignment holds for the whole buffer, the unassigned part needs no unaligned copy.  fold applies to the
// first fold_end bytes only (the assigned file's): the tiles from the one that holds byte fold_end on are emitted unfolded first, then
// the tiles up to fold_end folded -- the tile both reach into is written twice, its first fold_end % SCAF_TILE bytes last.
static int scaf_emit_keep(mxg_handle *h, const ScafText &t, PieceTable &pt, uint32_t fold, uint64_t fold_end)
{
    hipStream_t st = h->stream;
    DevBuf *B = h->scbuf;
    const uint64_t total = pt.total;
    const size_t n_pieces = pt.pieces.size();
    if (n_pieces >= 0xFFFFFFFFull) return set_err(h, MXG_ELIMIT, "mxg_write_scaffolds: too many pieces of output for one call");
    MXG_HIP(h, h->scaf_keep.ensure((total + SCAF_TILE - 1) / SCAF_TILE * SCAF_TILE + SCAF_TILE));
    if (!total) return MXG_OK;
    pt.pieces.push_back(ScafPiece{total, 0, 0, SP_LIT});  // (the end of the last piece)
    MXG_HIP(h, B[SC_PIECES].ensure((n_pieces + 1) * sizeof(ScafPiece)));
    MXG_HIP(h, B[SC_LITS].ensure(pt.lits.size() + 16));
    MXG_HIP(h, hipMemcpyAsync(B[SC_PIECES].p, pt.pieces.data(), (n_pieces + 1) * sizeof(ScafPiece), hipMemcpyHostToDevice, st));
    if (!pt.lits.empty()) MXG_HIP(h, hipMemcpyAsync(B[SC_LITS].p, pt.lits.data(), pt.lits.size(), hipMemcpyHostToDevice, st));
    unsigned char *d_keep = h->scaf_keep.as<unsigned char>();
    auto emit = [&](uint64_t lo, uint64_t hi, uint32_t f) {  // lo: a multiple of SCAF_TILE
        if (lo >= hi) return;
        hipLaunchKernelGGL(k_scaf_emit, dim3((uint32_t)((hi - lo + SCAF_TILE - 1) / SCAF_TILE)), dim3(256), 0, st, t, B[SC_PIECES].as<ScafPiece>(),
                           (uint32_t)n_pieces, B[SC_LITS].as<unsigned char>(), f, d_keep + lo, lo, hi);
    };
    if (fold && fold_end) {
        emit(fold_end / SCAF_TILE * SCAF_TILE, total, 0u);
        emit(0, std::min(fold_end, total), 1u);
    } else {
        emit(0, total, 0u);
    }
    MXG_HIP(h, hipGetLastError());
    MXG_HIP(h, hipStreamSynchronize(st));  // (the piece table is the caller's)
    return MXG_OK;
}

int write_scaffolds(mxg_handle *h, Assembly *a, int assembly, const mxg_scaffold_node *nodes, const uint64_t *path_first, uint64_t n_paths,
                    int32_t overlap_gap, uint32_t flags, const char *assigned_fa, const char *unassigned_fa, const char *unassigned_bed,
                    uint32_t *lead_strip, uint32_t *tail_strip, uint64_t *n_unassigned)
{
    const uint64_t n_nodes = n_paths ? path_first[n_paths] : 0;
    const bool keep = (flags & MXG_SCAF_KEEP) != 0;
    h->scaf_keep_valid = false;  // (the kept text of the call before holds until this one)
    if (!assigned_fa && (flags & (MXG_SCAF_BGZF | MXG_SCAF_FAI | MXG_SCAF_REPORT)))
        return set_err(h, MXG_EINVAL, "mxg_write_scaffolds: MXG_SCAF_BGZF, MXG_SCAF_FAI and MXG_SCAF_REPORT need assigned_fa, the file they are about");
    if (n_nodes >= (1ull << 31)) return set_err(h, MXG_ELIMIT, "mxg_write_scaffolds: %llu nodes (fewer than 2^31)", (unsigned long long)n_nodes);
    const bool indexed = a->text_on_device && a->d_text.p;
    if (a->holds_pieces || a->shard_lo != 0 || a->shard_hi < a->recs.size())
        return set_err(h, MXG_EINVAL, "mxg_write_scaffolds: assembly %d holds a shard or pieces of its file, not the whole text", assembly);
    if (!indexed && !(a->has_text && a->has_bases))
        return set_err(h, MXG_EINVAL, "mxg_write_scaffolds: assembly %d holds no text (a minimizer table from a TSV, side-car or arrays, packed bases "
                       "handed over on the device, text dropped by MXG_FLAG_DROP_SEQ or released by a one-shot handle): the scaffolds are "
                       "cut from the text of the FASTA", assembly);
    const bool overlap = overlap_gap >= 0;
    const size_t n_rec = a->recs.size();
    // ---- the nodes' text parts [x, y) in output orientation and their Ns; everything checked before any launch
    struct Part {
        uint32_t x, y, fill;
    };
    std::vector<Part> part(n_nodes);
    if (n_paths && path_first[0] != 0)  // (every node belongs to a path: the unassigned side reads them all)
        return set_err(h, MXG_EINVAL, "mxg_write_scaffolds: path_first[0] is %llu, not 0", (unsigned long long)path_first[0]);
    for (uint64_t p = 0; p < n_paths; ++p) {
        const uint64_t lo = path_first[p], hi = path_first[p + 1];
        if (hi < lo || hi > n_nodes) return set_err(h, MXG_EINVAL, "mxg_write_scaffolds: path_first is not increasing at path %llu", (unsigned long long)p);
        if (hi - lo < 2)
            return set_err(h, MXG_EINVAL, "mxg_write_scaffolds: path %llu has %llu node(s); a path has at least two (the reference leaves "
                           "shorter ones out)", (unsigned long long)p, (unsigned long long)(hi - lo));
        for (uint64_t i = lo; i < hi; ++i) {
            const mxg_scaffold_node &in = nodes[i];
            const unsigned long long up = p, un = i - lo;
            if (in.record >= n_rec) return set_err(h, MXG_EINVAL, "mxg_write_scaffolds: path %llu node %llu: no record %u", up, un, in.record);
            const Record &rec = a->recs[in.record];
            if (in.start >= in.end || in.end > rec.len)
                return set_err(h, MXG_EINVAL, "mxg_write_scaffolds: path %llu node %llu: [%u, %u) is not a segment of record '%s' (%llu bases)", up,
                               un, in.start, in.end, rec.id.c_str(), (unsigned long long)rec.len);
            const uint32_t L = in.end - in.start;
            Part &q = part[i];
            q.x = 0, q.y = L, q.fill = in.gap_size;
            if (overlap) {
                if (in.end_adjust > L)
                    return set_err(h, MXG_EINVAL, "mxg_write_scaffolds: path %llu node %llu: end_adjust %u is beyond the segment's %u bases", up, un,
                                   in.end_adjust, L);
                q.y = in.end_adjust ? in.end_adjust : L;
                q.x = std::min(in.start_adjust, q.y);
                if (in.gap_size && q.y != L) q.fill = (uint32_t)overlap_gap;
            }
            if ((i == lo || i + 1 == hi) && q.x >= q.y)
                return set_err(h, MXG_EINVAL, "mxg_write_scaffolds: path %llu node %llu: the %s piece of a path has no text left after its cuts", up, un,
                               i == lo ? "first" : "last");
        }
    }
    // ---- unassigned: per record the complement of the union of the nodes' ranges
    struct Iv {
        uint32_t rec, lo, hi;
    };
    std::vector<Iv> gaps;
    const bool want_un = unassigned_fa || unassigned_bed || n_unassigned || keep;
    if (want_un) {
        std::vector<Iv> used(n_nodes);
        for (uint64_t i = 0; i < n_nodes; ++i) used[i] = Iv{nodes[i].record, nodes[i].start, nodes[i].end};
        std::sort(used.begin(), used.end(), [](const Iv &x, const Iv &y) { return x.rec != y.rec ? x.rec < y.rec : x.lo < y.lo; });
        size_t u = 0;
        for (size_t r = 0; r < n_rec; ++r) {
            uint64_t at = 0;
            for (; u < used.size() && used[u].rec == r; ++u) {
                if (used[u].lo > at) gaps.push_back(Iv{(uint32_t)r, (uint32_t)at, used[u].lo});
                at = std::max<uint64_t>(at, used[u].hi);
            }
            if (a->recs[r].len > at) gaps.push_back(Iv{(uint32_t)r, (uint32_t)at, (uint32_t)a->recs[r].len});
        }
    }
    // ---- the text on the device
    MXG_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    DevBuf *B = h->scbuf;
    ScafText t{};
    std::vector<uint64_t> org(n_rec);
    if (indexed) {
        if (!a->d_ing_item0.p) {
            MXG_HIP(h, a->d_ing_item0.ensure(a->ing_item0.size() * 8));
            MXG_HIP(h, hipMemcpyAsync(a->d_ing_item0.p, a->ing_item0.data(), a->ing_item0.size() * 8, hipMemcpyHostToDevice, st));
        }
        for (size_t r = 0; r < n_rec; ++r) org[r] = a->recs[r].base_off;
        t.text_bytes = ((a->text_bytes + ING_TILE - 1) / ING_TILE + 1) * ING_TILE;  // (as load_fasta_device allocates and pads it)
    } else {
        t.text_bytes = (a->text.size() / SCAF_CHUNK + 2) * SCAF_CHUNK;
        if (!a->flat_text_on_device) {  // once per assembly
            MXG_HIP(h, a->d_text.ensure(t.text_bytes));
            MXG_HIP(h, hipMemsetAsync(a->d_text.p, '>', t.text_bytes, st));
            if (!a->text.empty()) MXG_HIP(h, hipMemcpyAsync(a->d_text.p, a->text.data(), a->text.size(), hipMemcpyHostToDevice, st));
            a->flat_text_on_device = true;
        }
        for (size_t r = 0; r < n_rec; ++r) org[r] = a->recs[r].text_off;
    }
    MXG_HIP(h, B[SC_ORG].ensure(n_rec * 8 + 16));
    if (n_rec) MXG_HIP(h, hipMemcpyAsync(B[SC_ORG].p, org.data(), n_rec * 8, hipMemcpyHostToDevice, st));
    t.text = a->d_text.as<unsigned char>();
    t.indexed = indexed ? 1u : 0u;
    t.rec_org = B[SC_ORG].as<uint64_t>();
    if (indexed)
        t.ix = TextIndex{t.text, a->d_ing_items.as<IngItem>(), a->d_ing_pbase.as<uint64_t>(), a->d_ing_sub.as<uint16_t>(),
                         a->d_ing_item0.as<uint64_t>(), t.rec_org};
    // ---- the ends to strip: [2 p] / [2 p + 1] = left of path p's first piece / right of its last, then two per interval
    const size_t n_ends = 2 * (size_t)n_paths + 2 * gaps.size();
    std::vector<ScafEnd> ends(n_ends);
    auto fwd_range = [&](uint64_t i, bool from_left) {  // the text part of node i in the record's coordinates
        const mxg_scaffold_node &in = nodes[i];
        const Part &q = part[i];
        if (in.reverse) return ScafEnd{in.record, in.end - q.y, in.end - q.x, from_left ? 1u : 0u};
        return ScafEnd{in.record, in.start + q.x, in.start + q.y, from_left ? 0u : 1u};
    };
    for (uint64_t p = 0; p < n_paths; ++p) {
        ends[2 * p] = fwd_range(path_first[p], true);
        ends[2 * p + 1] = fwd_range(path_first[p + 1] - 1, false);
    }
    for (size_t g = 0; g < gaps.size(); ++g) {
        ends[2 * n_paths + 2 * g] = ScafEnd{gaps[g].rec, gaps[g].lo, gaps[g].hi, 0u};
        ends[2 * n_paths + 2 * g + 1] = ScafEnd{gaps[g].rec, gaps[g].lo, gaps[g].hi, 1u};
    }
    std::vector<uint32_t> cnt(n_ends);
    if (n_ends) {
        if (n_ends >= 0x7FFFFFFFull) return set_err(h, MXG_ELIMIT, "mxg_write_scaffolds: too many ends to strip for one call");
        MXG_HIP(h, B[SC_ENDS].ensure(n_ends * sizeof(ScafEnd)));
        MXG_HIP(h, B[SC_CNT].ensure(n_ends * 4));
        MXG_HIP(h, hipMemcpyAsync(B[SC_ENDS].p, ends.data(), n_ends * sizeof(ScafEnd), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_scaf_ends, dim3((uint32_t)n_ends), dim3(64), 0, st, t, B[SC_ENDS].as<ScafEnd>(), B[SC_CNT].as<uint32_t>());
        MXG_HIP(h, hipGetLastError());
        MXG_HIP(h, hipMemcpyAsync(cnt.data(), B[SC_CNT].p, n_ends * 4, hipMemcpyDeviceToHost, st));
        MXG_HIP(h, hipStreamSynchronize(st));
    }
    for (uint64_t p = 0; p < n_paths; ++p)
        for (int side = 0; side < 2; ++side) {
            const ScafEnd &e = ends[2 * p + side];
            if (cnt[2 * p + side] >= e.hi - e.lo)
                return set_err(h, MXG_EINVAL, "mxg_write_scaffolds: path %llu: the text of its %s piece is N throughout (the reference asserts there)",
                               (unsigned long long)p, side ? "last" : "first");
        }
    // ---- nothing is refused from here on: the files
    const uint64_t WIN = std::max<uint64_t>(SCAF_TILE, std::min<uint64_t>(knob_u64(h, "MXG_SCAF_WIN", PIN_HALF), PIN_HALF) /
                                                           SCAF_TILE * SCAF_TILE);
    const uint32_t bgzf_P = flags & MXG_SCAF_BGZF ? bgzf_payload(h) : 0u;
    // MXG_SCAF_FAI: <file>.fai beside either FASTA and, for BGZF files, <file>.gzi (fai.hip)
    const bool with_fai = (flags & MXG_SCAF_FAI) != 0;
    // MXG_SCAF_REPORT: the report of either FASTA from its windows (report.hip); the record lengths are the piece table's
    const bool with_rep = (flags & MXG_SCAF_REPORT) != 0;
    std::vector<uint64_t> rep_len;
    if (with_rep) h->rep_scaf[0].valid = h->rep_scaf[1].valid = false;
    struct IndexFiles {
        OutFile fai, gzi;
        std::vector<FaiOutRec> recs;
        std::vector<uint64_t> member_off;
    } ix_fa, ix_ufa;
    auto open_index = [&](IndexFiles &ix, const char *fasta) -> int {
        const std::string fai = std::string(fasta) + ".fai", gzi = std::string(fasta) + ".gzi";
        if (!ix.fai.open(fai.c_str())) return set_err(h, MXG_EIO, "cannot open '%s' for writing", fai.c_str());
        if (bgzf_P && !ix.gzi.open(gzi.c_str())) return set_err(h, MXG_EIO, "cannot open '%s' for writing", gzi.c_str());
        return MXG_OK;
    };
    // the index of a FASTA written: its rows, and the .gzi from where the members went (member j holds text [j P, j P + P))
    auto write_index = [&](IndexFiles &ix, bool ntjoin_names) -> int {
        int rc = write_fai_records(h, a, ix.fai, ix.recs, ntjoin_names);
        if (rc != MXG_OK || !bgzf_P) return rc;
        std::vector<uint64_t> text_off(ix.member_off.size());
        for (size_t j = 0; j < text_off.size(); ++j) text_off[j] = (uint64_t)j * bgzf_P;
        return write_gzi(h, ix.gzi, ix.member_off, text_off);
    };
    OutFile fa, ufa, bed;
    if (assigned_fa && !fa.open(assigned_fa)) return set_err(h, MXG_EIO, "cannot open '%s' for writing", assigned_fa);
    if (unassigned_fa && !ufa.open(unassigned_fa)) return set_err(h, MXG_EIO, "cannot open '%s' for writing", unassigned_fa);
    if (unassigned_bed && !bed.open(unassigned_bed)) return set_err(h, MXG_EIO, "cannot open '%s' for writing", unassigned_bed);
    int rc;
    if (with_fai && (rc = open_index(ix_fa, assigned_fa)) != MXG_OK) return rc;
    if (with_fai && unassigned_fa && (rc = open_index(ix_ufa, unassigned_fa)) != MXG_OK) return rc;
    PieceTable kept;  // MXG_SCAF_KEEP: both files' pieces in one table
    std::vector<mxg_seq_piece> kp;  // ... and what their records are made of (mxg_scaffold_pieces)
    std::vector<uint64_t> kp_first(1, 0);
    std::vector<std::string> kp_id;
    uint64_t kept_fold_end = 0;
    {
        PieceTable pt;
        pt.pieces.reserve(2 * n_nodes + 2 * n_paths + 1);
        for (uint64_t p = 0; p < n_paths; ++p) {
            const uint64_t lo = path_first[p], hi = path_first[p + 1];
            const uint32_t lead = cnt[2 * p], tail_text = cnt[2 * p + 1];
            const uint64_t head0 = pt.total;
            pt.literal(">ntJoin" + std::to_string(p) + "\n");
            const uint64_t seq0 = pt.total;
            for (uint64_t i = lo; i < hi; ++i) {
                const mxg_scaffold_node &in = nodes[i];
                uint32_t x = part[i].x, y = part[i].y, fill = part[i].fill;
                if (i == lo) x += lead;
                if (i + 1 == hi) {  // (the Ns behind the last piece go first, then those of its text)
                    y -= tail_text;
                    if (tail_strip) tail_strip[p] = fill + tail_text;
                    fill = 0;
                }
                if (y > x) {
                    if (in.reverse) pt.add(SP_REV, y - x, (uint64_t)in.end - 1 - x, in.record);
                    else pt.add(SP_FWD, y - x, (uint64_t)in.start + x, in.record);
                    if (keep && in.reverse) kp.push_back(mxg_seq_piece{in.record, in.end - y, in.end - x, MXG_PIECE_REV});
                    if (keep && !in.reverse) kp.push_back(mxg_seq_piece{in.record, in.start + x, in.start + y, MXG_PIECE_FWD});
                }
                pt.add(SP_FILL, fill);
                if (keep && fill) kp.push_back(mxg_seq_piece{0, 0, fill, MXG_PIECE_GAP});
            }
            if (keep) {
                kp_first.push_back(kp.size());
                kp_id.push_back("ntJoin" + std::to_string(p));
            }
            if (with_fai) ix_fa.recs.push_back(FaiOutRec{pt.total - seq0, (uint32_t)(seq0 - head0), 0u, 0u, 0u});
            if (with_rep) rep_len.push_back(pt.total - seq0);
            pt.literal("\n");
            if (lead_strip) lead_strip[p] = lead;
        }
        if (keep) {
            kept.append(pt);
            kept_fold_end = pt.total;
        }
        if (assigned_fa && (rc = scaf_emit_file(h, t, pt, flags & MXG_SCAF_FOLD_CASE ? 1u : 0u, fa, WIN, bgzf_P, with_fai ? &ix_fa.member_off : nullptr,
                                                with_rep, n_paths)) != MXG_OK)
            return rc;
        if (with_rep && (rc = report_file_end(h, MXG_REPORT_ASSIGNED, std::move(rep_len), assigned_fa)) != MXG_OK) return rc;
        if (with_fai && (rc = write_index(ix_fa, true)) != MXG_OK) return rc;
    }
    uint64_t n_un = 0;
    h->scaf_lead.assign(gaps.size(), 0);  // what mxg_scaffold_strips hands out: per interval of the BED
    h->scaf_tail.assign(gaps.size(), 0);
    {
        PieceTable pt;
        for (size_t g = 0; g < gaps.size(); ++g) {
            const Iv &iv = gaps[g];
            const uint32_t len = iv.hi - iv.lo, lead = cnt[2 * n_paths + 2 * g], tail = cnt[2 * n_paths + 2 * g + 1];
            h->scaf_lead[g] = lead;
            h->scaf_tail[g] = lead >= len ? 0 : tail;  // (N throughout: all of it counts as the lead)
            if (lead >= len) continue;  // N throughout: in the BED only
            ++n_un;
            if (!unassigned_fa && !keep) continue;
            const uint64_t head0 = pt.total;
            pt.literal(">" + a->recs[iv.rec].id + ":" + std::to_string(iv.lo) + "-" + std::to_string(iv.hi) + "\n");
            if (with_fai) ix_ufa.recs.push_back(FaiOutRec{(uint64_t)len - lead - tail, (uint32_t)(pt.total - head0), iv.rec, iv.lo, iv.hi});
            if (with_rep) rep_len.push_back((uint64_t)len - lead - tail);
            pt.add(SP_FWD, len - lead - tail, (uint64_t)iv.lo + lead, iv.rec);
            pt.literal("\n");
            if (keep) {
                kp.push_back(mxg_seq_piece{iv.rec, iv.lo + lead, iv.hi - tail, MXG_PIECE_FWD});
                kp_first.push_back(kp.size());
                kp_id.push_back(a->recs[iv.rec].id + ":" + std::to_string(iv.lo) + "-" + std::to_string(iv.hi));
            }
        }
        if (keep) kept.append(pt);
        if (with_rep) rep_len.shrink_to_fit();
        if (unassigned_fa && (rc = scaf_emit_file(h, t, pt, 0u, ufa, WIN, bgzf_P, with_fai ? &ix_ufa.member_off : nullptr, with_rep, rep_len.size())) !=
                                 MXG_OK)
            return rc;
        if (with_rep && unassigned_fa && (rc = report_file_end(h, MXG_REPORT_UNASSIGNED, std::move(rep_len), unassigned_fa)) != MXG_OK) return rc;
        if (with_fai && unassigned_fa && (rc = write_index(ix_ufa, false)) != MXG_OK) return rc;
    }
    if (want_un) {  // the intervals with their strips: what mxg_write_paths makes the AGP's unassigned lines of
        h->scaf_iv.resize(gaps.size());
        for (size_t g = 0; g < gaps.size(); ++g) h->scaf_iv[g] = {gaps[g].rec, gaps[g].lo, gaps[g].hi, h->scaf_lead[g], h->scaf_tail[g]};
        h->scaf_iv_asm = assembly;
    }
    if (unassigned_bed) {
        for (const Iv &iv : gaps) fprintf(bed.f, "%s\t%u\t%u\n", a->recs[iv.rec].id.c_str(), iv.lo, iv.hi);
        if (ferror(bed.f)) return set_err(h, MXG_EIO, "write error on '%s'", unassigned_bed);
    }
    if (keep && (rc = scaf_emit_keep(h, t, kept, flags & MXG_SCAF_FOLD_CASE ? 1u : 0u, kept_fold_end)) != MXG_OK) return rc;
    MXG_HIP(h, hipStreamSynchronize(st));
    const bool c_fa = fa.close(), c_ufa = ufa.close(), c_bed = bed.close();
    const bool c_fai = ix_fa.fai.close(), c_gzi = ix_fa.gzi.close(), c_ufai = ix_ufa.fai.close(), c_ugzi = ix_ufa.gzi.close();
    const bool c_ix = c_fai && c_gzi && c_ufai && c_ugzi;
    if (!(c_fa && c_ufa && c_bed && c_ix)) return set_err(h, MXG_EIO, "mxg_write_scaffolds: write error while closing the output files");
    fa.complete = ufa.complete = bed.complete = true;
    ix_fa.fai.complete = ix_fa.gzi.complete = ix_ufa.fai.complete = ix_ufa.gzi.complete = true;
    if (n_unassigned) *n_unassigned = n_un;
    if (keep) {
        h->scaf_keep_bytes = kept.total;
        h->scaf_keep_asm = assembly;
        h->scaf_keep_pieces.swap(kp);
        h->scaf_keep_first.swap(kp_first);
        h->scaf_keep_id.swap(kp_id);
        h->scaf_keep_valid = true;
    }
    return MXG_OK;
}

}  // namespace mxg
