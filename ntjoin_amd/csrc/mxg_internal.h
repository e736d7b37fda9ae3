// mxg_internal.h -- internal structures of libntjoin_mx.so (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <sys/stat.h>

#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "join_plan.h"
#include "ntjoin_mx.h"
#include "out_file.h"

namespace mxg {

// ---- device-side tables ------------------------------------------------------------------------
// One maximal run of valid (ACGTU) bases that holds at least one k-mer, inside an ELIGIBLE contig
// (a record with >= w valid k-mers; shorter records have no window and yield no minimizer,
// SURVEY.md A.3).  Windows are taken over the concatenation of a contig's runs (valid k-mers only).
struct Run {
    uint64_t base_off;  // global base index (into the packed array) of the run's first base
    uint32_t n_kmers;   // run_len - k + 1
    uint32_t contig;    // eligible-contig index
    uint32_t kidx0;     // contig-local valid-k-mer index of the run's first k-mer
    uint32_t pos0;      // contig-local base position of the run's first base
};

// a run as k_bs_select (sketch_bs.hip) reads it: one aligned 32-byte entry where Run + the strip prefix + the contig's k-mer
// count are three dependent table reads (strip0 belongs to the assembly's sparse strip length)
struct alignas(32) RunX {
    uint64_t base_off;
    uint32_t n_kmers, contig, kidx0;
    uint32_t strip0S;   // (strips of the sparse strip table in front of the run) x (k-mers per strip), mod 2^32
    uint32_t nk;        // valid k-mers of the run's contig
    uint32_t pad;
};

struct HashTab {  // ntHash step table, entry (out*4+in), out==4: warm-up step with no outgoing base
    // x,y = low/high word of  srol^k(SEED[out]) ^ SEED[in]            (forward update term)
    // z,w = low/high word of  SEED[comp(out)] ^ srol^k(SEED[comp(in)]) (reverse update term, before sror)
    uint4 e[20];
};

// ---- host-side helpers ---------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // grow-only; contents are NOT preserved
    hipError_t ensure(size_t need)
    {
        if (need <= bytes) return hipSuccess;
        static const bool dbg = getenv("MXG_DEBUG_ALLOC") != nullptr;  // (diagnostics: what a handle's first step allocates)
        const auto t0 = std::chrono::steady_clock::now();
        const size_t had = bytes;
        release();
        size_t want = need + need / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        bytes = want;
        if (dbg)
            fprintf(stderr, "[mxg] alloc %.1f MB (had %.1f MB): %.3f ms\n", want / 1048576.0, had / 1048576.0,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        return hipSuccess;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct Record {
    std::string id;
    uint64_t len = 0;       // bases in the record
    uint64_t base_off = 0;  // global base offset in the packed array (multiple of 16)
    uint64_t text_off = 0;  // offset of the record's text in Assembly::text (if kept)
};

struct Assembly {
    std::string name;
    double weight = 0.0;
    std::vector<Record> recs;
    uint64_t total_bases = 0;
    uint64_t shard_lo = 0, shard_hi = ~0ull;  // records this handle holds bases for (fasta_shard); others: id + length only
    // bases
    bool has_bases = false;
    std::string text;                // concatenated record text as read (kept unless MXG_FLAG_DROP_SEQ)
    bool has_text = false;
    std::vector<uint32_t> h_packed;  // host 2-bit packing (dropped after upload)
    // the invalid (non-ACGTU) bases as maximal intervals [first, second) of global base indices, in base order.  Unlike the run
    // table below (runs of >= k bases of eligible records, for the handle's k and w) this holds for any k and w: what
    // mxg_overlap_cuts (overlap.hip) decides validity by.  Empty for packed-device input (no invalid bases by contract).
    std::vector<std::pair<uint64_t, uint64_t>> inv;
    DevBuf d_inv;              // ... uploaded by the first mxg_overlap_cuts
    bool inv_on_device = false;
    bool holds_pieces = false;  // split load: the handle holds pieces of records, not whole records
    // device ingest (ingest.hip): the raw FASTA text in HBM + the tile index that maps a base to its byte
    bool text_on_device = false;
    uint64_t text_bytes = 0;
    bool flat_text_on_device = false;  // host ingest: Assembly::text copied to d_text by the first mxg_write_scaffolds (no line ends, no index)
    DevBuf d_text, d_ing_items, d_ing_cnt, d_ing_sub, d_ing_pbase, d_ing_item0;
    std::vector<uint64_t> ing_item0;  // [n_records + 1] first tile of every record
    // the members of a BGZF input that hold text: where each starts in the file and in the text (what its .gzi is made of, fai.hip)
    bool from_bgzf = false;
    std::vector<uint64_t> bgzf_comp_off, bgzf_text_off;
    DevBuf d_packed_own;
    const uint32_t *d_packed = nullptr;  // owned (above) or borrowed
    uint64_t packed_words = 0;
    // eligibility tables (host), uploaded by the sketch driver
    std::vector<Run> runs;
    std::vector<uint32_t> ctg_rec;   // eligible contig -> record index
    std::vector<uint32_t> ctg_nk;    // eligible contig -> valid k-mer count
    std::vector<uint32_t> ctg_run0;  // eligible contig -> first run (size n+1)
    std::vector<uint8_t> ctg_drop;   // split load only: the contig is a piece whose first minimizer belongs to the shard before
    bool any_drop = false;
    bool split_first_cont = false;   // split load: this handle's first record continues a record begun on the shard before
    uint64_t total_kmers = 0;        // over eligible contigs
    // device copies of the tables above + strip / k-mer prefix tables (built once, by the first sketch)
    bool tables_ready = false;
    uint32_t S_sparse = 256;  // strip length chosen for the sparse hash kernel
    uint32_t cand_hint = 0;   // candidates of the last sparse run (k_resolve: which blocks may load before the count arrives)
    bool full_grid_once = false;       // the next enqueue sizes every grid for the candidate capacity, not the estimate
    double gap_rate_hint = 0;          // candidate-free stretches per k-mer met by earlier sketches (sizes the batches)
    std::vector<uint32_t> cand_hints;  // ... per batch of the pipelined multi-batch driver
    std::vector<uint32_t> strip0_dense, strip0_sparse;  // [n_runs+1] exclusive prefix of strips per run
    std::vector<uint64_t> g0;                           // [n_runs+1] exclusive prefix of k-mers per run
    DevBuf d_runs, d_strip0_dense, d_strip0_sparse, d_g0, d_ctg_nk, d_ctg_rec, d_ctg_run0, d_ctg_drop;
    DevBuf d_ctg_info;  // uint4 per contig {first run, runs, first run's pos0, record}: what k_emit needs of a contig in one read
    DevBuf d_strip_run;  // strip of the sparse strip table -> its run (k_strip_runs)
    DevBuf d_runx;       // RunX per run
    // k = 32 route (sketch_bs.hip): the bases transposed for the bit-sliced ring filter, its result, chunk -> first run
    bool bs_ready = false, bs_impossible = false;
    uint32_t bs_chunks = 0;
    DevBuf d_bs_tail, d_bs_out;  // k = 32 route: padded copies of the first / last chunk's words, the filter's bitmap
    bool sel_again = false;  // the second attempt of an assembly's batches may take k_bs_select again (only the stretch budget failed)
    uint32_t sel_H = 0, sel_H_S = 0, sel_H_w = 0;  // k_bs_select: halo strips (0: the route does not take this run table) for (S, w)
    // sketch (device, ordered by (record,pos)) + lazily filled host mirror
    bool has_sketch = false;
    uint64_t n_mx = 0;
    uint64_t n_mx_seen = 0;  // the largest sketch an earlier mxg_sketch* of this assembly ended with (sizes the fused graph stage)
    DevBuf d_hash, d_pos, d_rec, d_fwd, d_rec_base;
    bool fwd_valid = false;  // d_fwd filled (lazily: k_strand)
    bool foreign_sketch = false;  // sketch holds minimizers of records this handle has no bases for (gathered / imported)
    bool host_valid = false;
    std::vector<uint64_t> h_hash;
    std::vector<uint32_t> h_pos, h_rec;
    std::vector<uint8_t> h_fwd;
    std::vector<uint64_t> rec_first;
    // graph stage
    DevBuf d_flags, d_slot, d_ivid;
    DevBuf d_perm, d_fg, d_frec, d_dgtmp;  // distributed graph stage (dgraph.hip), sender side
    std::vector<uint8_t> h_flags;
    bool flags_valid = false;   // device flags computed
    bool flags_on_host = false; // h_flags mirrors d_flags
};

struct Graph {
    bool valid = false;       // device results computed
    bool own_order = false;   // ... by the whole stage on this handle's own sketches: row a of g_fv / g_frec is assembly a's sketch order
    bool host_valid = false;  // host mirrors below filled (lazily, by graph_to_host)
    uint32_t n_asm = 0;
    uint64_t nv = 0, ne = 0, nv_stride = 0;
    std::vector<uint64_t> vhash;
    std::vector<uint32_t> vpos, vrec;  // [a*nv+v]
    std::vector<uint32_t> eu, ev, esup;
    std::vector<double> ew;
};

struct Paths {  // result of mxg_find_paths (host copies)
    bool valid = false;
    uint64_t n_components = 0;        // components of the globally filtered graph (singletons included)
    std::vector<uint32_t> vertex;     // concatenated paths, vertex indices of the graph, source -> target
    std::vector<uint64_t> first;      // [n_paths+1]
    std::vector<uint32_t> component;  // [n_paths] component (root vertex index) of the globally filtered graph
};

struct Segments {  // results of mxg_path_segments / mxg_mx_extremes / mxg_path_segments_mk (host copies)
    int assembly = -1;                          // the segments' assembly (-1: none since the last mxg_find_paths)
    std::vector<uint32_t> path, record, first;  // per segment
    std::vector<uint32_t> stat;                 // per segment: n, min pos, max pos, increasing pairs, decreasing pairs
    std::vector<int64_t> mk_s;                  // per segment: Mann-Kendall S
    std::vector<uint64_t> mk_tie;               // ... and tie term
    std::vector<uint32_t> ext_min, ext_max;     // per record of the assembly last asked for
};

struct PathNodes {  // result of mxg_format_paths (host copies)
    std::vector<uint64_t> node_first;  // [n_paths + 1]
    std::vector<uint64_t> block;       // the node arrays as the device holds them (one copy); the pointers below look into it
    size_t n_nodes = 0;
    const uint32_t *record = nullptr, *start = nullptr, *end = nullptr, *contig_size = nullptr, *first_vertex = nullptr,
                   *terminal_vertex = nullptr, *segment = nullptr;
    const uint8_t *reverse = nullptr;
    const int64_t *gap = nullptr, *raw = nullptr;
};

struct Timers {
    double ms_hash = 0, ms_resolve = 0, ms_graph = 0;
    // MXG_FLAG_TIMING_FINE: one span per kernel (ms_resolve stays the sum of the three behind the hash kernel)
    double ms_reorder = 0, ms_resolve_k = 0, ms_emit = 0, ms_join = 0, ms_vertices = 0, ms_edges = 0;
    uint64_t launches_hash = 0, hash_bases = 0;
};

// MXG_FLAG_TIMING: event pairs recorded around the hash kernel / the rest of a batch.  Events come from a pool and are
// read back lazily (flush_timers: mxg_get_stats, mxg_reset_timers), so timing adds two hipEventRecord per pair to the
// hot path and nothing else.
struct TimedSpan {
    hipEvent_t a, b;
    uint64_t bases;
    bool is_hash;
    int kind;  // 0 hash, 1 everything behind it (coarse timing), 2 reorder, 3 resolve, 4 emit (fine timing)
};

// what sketch_assemblies (sketch.hip) knows of an assembly's sketch while the step runs, and what mxg_sketch_pack leaves
// for sketch_finish
enum class AsmState : int {
    Sync = 0,      // not (or no longer) in the streams: the synchronous path sketches it
    Enqueued = 1,  // its batches are in the streams, their reports not read yet
    Done = 2,      // its sketch is complete (an assembly without k-mers is, from the start)
    Retry = 3,     // its batches did not all end the common way: enqueue it once more
};

struct JoinPlan;  // graph.hip: the layout of the graph stage's join (plan_join)

// report.hip: one file's report as the handle keeps it (mxg_seq_report points into the vectors)
struct SeqReportHost {
    bool valid = false;
    uint64_t min_gap = 0, min_len = 0;
    uint64_t n_records = 0, bases = 0;
    uint64_t cnt[7] = {0, 0, 0, 0, 0, 0, 0};  // A C G T N other lower (seqstat.h)
    std::vector<uint64_t> rec_len, gap_len, ctg_len;
};

}  // namespace mxg

struct mxg_handle {
    mxg_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // second stream of the pipelined multi-assembly sketch (always library-owned)
    uint64_t timing_batches = 0;    // batches enqueued with MXG_FLAG_TIMING (MXG_TIMING_SAMPLE picks one in n)
    hipStream_t stream_x[2] = {nullptr, nullptr};  // third / fourth stream: batches of multi-batch assemblies (created on first use)
    bool own_stream = false;
    std::string err;
    std::vector<mxg::Assembly *> asms;
    mxg::Graph graph;
    std::vector<hipEvent_t> ev_pool;       // every event ever created for timing; [0, ev_used) are in flight
    size_t ev_used = 0;
    std::vector<mxg::TimedSpan> ev_spans;  // not yet folded into tm
    mxg::DevBuf d_nmx;              // fused sketch+graph call: sketch sizes on the device
    mxg::DevBuf d_chain;            // pipelined batches: where the next batch of an assembly starts in its sketch (u64 per batch)
    std::vector<hipEvent_t> ev_sync;  // ... and the events by which a batch waits for its predecessor on the other stream
    hipEvent_t ev_join = nullptr;   // ... and the event that joins the second stream into the first
    hipEvent_t ev_part[MXG_MAX_ASSEMBLIES] = {};  // mxg_sketch_pack_parts: assembly a's part is packed
    mxg::DevBuf dbg_buf;            // (profiling: MXG_BSR_DBG)
    uint32_t dbg_blocks = 0;
    std::vector<hipEvent_t> ev_bs;  // k = 32 route: "the assembly's filter has run" (batches on other streams wait for it)
    mxg::DevBuf dg_cnt, dg_cursor;  // dgraph.hip: per-destination counts / cursors
    mxg::DevBuf dg_ghost;           // ... {record, global vertex id} of the shared minimizer before this rank's first, per assembly
    bool dg_ghost_on = false;
    mxg::Paths paths;
    mxg::DevBuf pbuf[56];  // scratch of paths.hip
    mxg::DevBuf mkbuf[8];  // scratch of mk.hip
    mxg::DevBuf ovbuf[16];  // scratch of overlap.hip
    mxg::DevBuf scbuf[8];   // scratch of scaffold.hip
    mxg::DevBuf adjbuf[32];  // scratch of adjust.hip
    std::vector<mxg_adjust_node> adj_nodes;      // the last mxg_adjust_paths' result (what its view points into)
    std::vector<uint64_t> adj_first, adj_source;
    // MXG_SCAF_KEEP: the text of both scaffold files of the last mxg_write_scaffolds, resident (mxg_scaffold_text), what its records
    // are made of (mxg_scaffold_pieces) and their names (mxg_scaffold_record_id); valid until the next mxg_write_scaffolds
    mxg::DevBuf scaf_keep;
    bool scaf_keep_valid = false;
    uint64_t scaf_keep_bytes = 0;
    int scaf_keep_asm = -1;
    std::vector<mxg_seq_piece> scaf_keep_pieces;
    std::vector<uint64_t> scaf_keep_first;
    std::vector<std::string> scaf_keep_id;
    mxg::DevBuf cmpbuf[16];  // scratch of compose.hip
    std::vector<mxg_seq_piece> cmp_pieces;       // the last mxg_compose_pieces' result (what its pointers point into)
    std::vector<uint64_t> cmp_first;
    mxg::DevBuf synbuf[32];  // scratch of synteny.hip
    struct Synteny {         // the last mxg_synteny_blocks (what its view points into, and what mxg_write_synteny_paf writes)
        bool valid = false, q_table = false;  // q_table: the query's records are those of a piece table, not the handle's
        int q = -1, s = -1;
        uint64_t n_anchors = 0, n_links = 0;
        std::vector<uint32_t> block;     // eight arrays of n_blocks words: n_anchors, q_record, q_start, q_end, s_record, s_start, s_end, reverse
        std::vector<uint8_t> reverse;    // [n_blocks]
        std::vector<uint32_t> q_len, s_len;  // the lengths of the query's records (a piece table's: the sums of their pieces) and the subject's
        std::vector<uint32_t> q_pre, q_first;  // q_table: every piece's offset in its record, and the records' first pieces (n_records + 1)
        // what the call left in synbuf, for mxg_synteny_identity: the anchor list, and per block (kept or not) its first and last
        // anchor, the keep flag and the kept blocks before it.  Nothing but the next mxg_synteny_blocks writes these arrays
        const void *d_anchor = nullptr;
        const uint32_t *d_first = nullptr, *d_last = nullptr, *d_keep = nullptr, *d_kscan = nullptr;
        uint32_t n_dev_blocks = 0;
    } syn;
    struct Identity {        // the last mxg_synteny_identity (what its view points into); void after the next mxg_synteny_blocks
        bool valid = false;
        uint64_t n_segments = 0;
        std::vector<uint64_t> blk;  // eight arrays of n_blocks words: n_aligned, n_skip_len, n_skip_shift, n_skip_n, n_saturated, aligned_q, aligned_s, edits
    } idy;
    mxg::DevBuf asbuf[32];   // scratch of assess.hip
    struct Assess {          // the last mxg_synteny_assess (what its view points into)
        uint64_t n_chains = 0, n_bp = 0, query_bases = 0, subject_bases = 0;
        uint64_t sum[32] = {};          // assess.hip's summary words
        std::vector<uint32_t> chain;    // ten arrays of n_chains words, in the order of AsChain's fields
        std::vector<uint32_t> bp;       // five arrays of n_bp words: chain, kind, at_join, q_lo, q_hi
        std::vector<uint32_t> bp_all;   // scratch: the same as they come home, five arrays of n_chains words
    } assess;
    mxg::DevBuf idybuf[24];   // scratch of identity.hip
    mxg::DevBuf lftbuf[48];   // scratch of lift.hip, and the index of the last mxg_lift_prepare
    struct Lift {             // the last mxg_lift_prepare, and the last lift call's result (what mxg_lift_view points into)
        bool valid = false;
        uint32_t m = 0;                 // sequence pieces in the index
        int sorted_in = 0;              // which of the sort's two buffers holds the sorted keys
        uint64_t n_records = 0;         // records of the table
        std::vector<uint32_t> src_len;  // [n_source]
        std::vector<uint64_t> part_first;
        std::vector<uint8_t> status, reverse;
        std::vector<uint32_t> parts;    // five arrays of n_parts words: s_record, s_start, s_end, src_start, reverse
        uint64_t n_parts = 0;
    } lift;
    std::vector<uint32_t> scaf_lead, scaf_tail;  // N/n stripped from either end of every unassigned interval by the last mxg_write_scaffolds
    struct ScafInterval {
        uint32_t rec, lo, hi, lead, tail;
    };
    // the unassigned intervals, in BED order, with their strips, of the last mxg_write_scaffolds that computed the unassigned side,
    // and their assembly (-1: no such call yet): what mxg_write_paths makes the AGP's unassigned lines of
    std::vector<ScafInterval> scaf_iv;
    int scaf_iv_asm = -1;
    mxg::DevBuf ptbuf[16];  // scratch of pathtext.hip
    mxg::DevBuf faibuf[16];  // scratch of fai.hip
    mxg::DevBuf repbuf[16];  // scratch of report.hip
    uint64_t rep_min_gap = 10, rep_min_len = 500;  // mxg_set_report_params
    mxg::SeqReportHost rep_asm;                    // the last mxg_assembly_report
    mxg::SeqReportHost rep_scaf[3];                // the last mxg_write_scaffolds with MXG_SCAF_REPORT: assigned, unassigned; [2]: their union, made on demand
    std::vector<uint64_t> rep_sorted;              // scratch of the contiguity blocks
    struct RepRun {  // a report that is being made on the device (report.hip)
        uint64_t starts_seen = 0, gap_cap = 0, ctg_cap = 0, n_records = 0;
        const void *d_segs = nullptr;
        uint32_t n_segs = 0;
    } rep_run;
    mxg::Segments segs;
    mxg::PathNodes nodes;
    mxg::Timers tm;
    mxg::HashTab tab{};
    mxg::DevBuf d_init_tab;  // byte table of the direct hash formula (256 x 16 B), built by the first sketch
    uint64_t stat_candidates = 0, stat_dense_kmers = 0, stat_unique = 0;
    uint64_t stat_bs_bases = 0;  // bases the bit-sliced filter (k = 32 route) has covered
    uint64_t stat_sel_slices = 0;  // slices enqueued through k_bs_select
    uint64_t stat_slice_stretches = 0;  // candidate-free stretches handed to k_sel_stretch
    hipEvent_t ev_sel_done[4] = {nullptr, nullptr, nullptr, nullptr};  // recorded behind every slice kernel, per stream slot
    uint64_t stat_graph_join = 0; // mxg_stats::graph_join
    mxg::JoinLearnt pj_learnt;   // graph stage: what the LDS joins' overflows have taught this handle (join_plan.h)
    // fused call: the join as it was planned before the sketches (graph_plan_early), how many assemblies have been partitioned behind
    // their own k_emit since (graph_partition_early), the event behind the plan's clears
    mxg::JoinPlan *pj_plan = nullptr;
    uint32_t pj_early_done = 0;
    hipEvent_t ev_plan = nullptr;
    uint64_t stat_retries = 0;   // assemblies enqueued a second time (their batches did not all end the common way)
    uint64_t stat_deferred = 0;  // candidate-free stretches the device route handed to the host
    uint64_t stat_batches_redone = 0, stat_sync_assemblies = 0;  // batches that did not end the common way / assemblies redone whole
    // scratch reused across calls
    mxg::DevBuf scratch[4][40];  // indexed by mxg::Scratch (sketch.hip): one set per in-flight sketch driver (= stream)
    std::vector<mxg::Assembly *> pend_list;  // mxg_sketch_pack in flight: assemblies and how each was enqueued
    std::vector<mxg::AsmState> pend_state;
    std::vector<unsigned char> pend_dev;     // ... and whether its stretches went the device route (sketch_finish accepts those)
    mxg::DevBuf g_part;     // partitioned join (graph.hip): partition offsets of every bucketing block
    mxg::DevBuf g_recs1;    // two-level join: the coarse partitions' records
    mxg::DevBuf g_keys, g_cnt, g_vid, g_ctl, g_vhash, g_vpos, g_vrec, g_fv, g_frec, g_nxt, g_prv, g_eflag,
        g_ebs, g_eu, g_ev, g_esup, g_ew;  // indexed by mxg::Scratch (sketch.hip) / graph.hip's own enum
    uint64_t arena_cap_hint = 0;
    // environment knobs (README: tuning / test / profiling switches), each parsed ONCE per handle, at its first use: what a
    // handle ran with is what mxg_knobs reports, whatever the environment says later
    struct Knob {
        bool set = false;
        uint64_t value = 0;
        std::string raw;
    };
    std::map<std::string, Knob> knobs;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_g[2] = {nullptr, nullptr};  // MXG_FLAG_TIMING_FINE: after the join, after vertices + adjacency
    uint64_t *pinned_dg = nullptr;    // dgraph.hip: pinned copy of the per-destination counters
    uint64_t *pinned_gctl = nullptr;  // pinned host copy of the graph stage's control block
    uint32_t *pinned_ctrl = nullptr;  // pinned host copies of per-assembly control blocks (pipelined sketch)
    std::vector<char> dot_part[2];    // a formatted part of the .mx.dot (mxg_dot_part_format -> mxg_dot_part_write)
    void *pinned_defer = nullptr;     // per control block: the stretches its batch left to the host (sketch.hip defer_stretch)
    // 128 MB of pinned host memory shared by the file routes (FASTA text on its way in: 4 x 32 MB, TSV text on its way out: 2 x 64 MB)
    // and the TSV writer's device windows: allocated on first use, kept until mxg_destroy -- a pinned allocation of this size
    // costs 25-55 ms, and the one-process route (mxgraph) would pay it four times
    void *pin_pool = nullptr;
    // ... and pinning is what costs: the pool is ordinary memory that a (detached) thread of the handle registers with HIP in four pieces of
    // 32 MB (pin_pool_start), so the first file's upload starts when the first staging buffer is pinned (~7 ms), not the last (~29 ms)
    std::atomic<uint32_t> pin_ready{0};   // pieces registered so far
    std::atomic<int> pin_state{0};        // 0 no pool, 1 the thread is at work, 2 done, 3 failed (pin_err)
    hipError_t pin_err = hipSuccess;
    bool pin_registered = false;          // the pool is mmap'ed memory registered piece by piece (else: hipHostMalloc)
    std::vector<std::pair<void *, size_t>> kept_maps;  // MXG_FLAG_ONE_SHOT: file mappings left for mxg_destroy / the process's end
    mxg::DevBuf tsv_win[2];
    mxg::DevBuf zbuf[4];  // scratch of bgzf_deflate.hip: the members' slots, their sizes and places, the packed window
};

namespace mxg {

int set_err(mxg_handle *h, int code, const char *fmt, ...);
// environment knob `name` as the handle first saw it (host_io.cpp): its value, or dflt when it is unset / empty
uint64_t knob_u64(const mxg_handle *h, const char *name, uint64_t dflt);
bool knob_set(const mxg_handle *h, const char *name);
const char *knob_raw(const mxg_handle *h, const char *name);  // the text it was set to, or nullptr
// a helper thread of the library points this at a string of its own: set_err then leaves the handle's message alone (host_io.cpp)
extern thread_local std::string *tl_err_sink;
constexpr size_t PIN_POOL_BYTES = 128ull << 20;
constexpr size_t PIN_PIECE_BYTES = 32ull << 20;
constexpr uint32_t PIN_PIECES = (uint32_t)(PIN_POOL_BYTES / PIN_PIECE_BYTES);
// host_io.cpp: starts the pool (no-op when there is one); waits until `pieces` pieces from the pool's start are pinned
hipError_t pin_pool_start(mxg_handle *h);
hipError_t pin_pool_wait(mxg_handle *h, uint32_t pieces);
void pin_pool_release(mxg_handle *h);
inline hipError_t pin_pool_get(mxg_handle *h, unsigned char **p)  // the whole pool
{
    hipError_t e = pin_pool_start(h);
    if (e == hipSuccess) e = pin_pool_wait(h, PIN_PIECES);
    if (e != hipSuccess && (e = pin_pool_start(h)) == hipSuccess) e = pin_pool_wait(h, PIN_PIECES);  // (once more, in one allocation)
    if (e != hipSuccess) return e;
    *p = static_cast<unsigned char *>(h->pin_pool);
    return hipSuccess;
}
// Wait for a stream by polling: hipStreamSynchronize parks the thread and its wake-up costs tens of microseconds, which
// is a tenth of a whole sketch+graph step at 2 x 100 Mbp.  The two syncs on the hot path (end of the sketch stage, end
// of the graph stage) poll for a bounded time, then fall back to the blocking wait.
inline hipError_t stream_wait(hipStream_t s)
{
    for (int spin = 0; spin < 200000; ++spin) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
    }
    return hipStreamSynchronize(s);
}

#define MXG_HIP(h, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return mxg::set_err((h), e_ == hipErrorOutOfMemory ? MXG_ENOMEM : MXG_EDEVICE,      \
                                "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                                __LINE__);                                                       \
    } while (0)

// host_io.cpp
int load_fasta(mxg_handle *h, Assembly *a, const char *path, uint32_t shard = 0, uint32_t n_shards = 1, bool split = false);
void shard_range(const uint64_t *lengths, uint64_t n, uint32_t shard, uint32_t n_shards, uint64_t *lo, uint64_t *hi);
int load_buffers(mxg_handle *h, Assembly *a, const uint8_t *ascii, const uint64_t *offsets,
                 const char *const *ids, uint64_t n_records);
int load_tsv(mxg_handle *h, Assembly *a, const char *path, std::vector<uint64_t> &hash,
             std::vector<uint32_t> &pos, std::vector<uint32_t> &rec);
void build_runs_from_lengths(mxg_handle *h, Assembly *a);  // N-free packed-device input
int write_tsv(mxg_handle *h, Assembly *a, const char *path, int with_pos, int with_strand, int with_seq);
// ingest.hip: FASTA -> packed bases + run table on the device (1: not for this route, use load_fasta); TSV text on the device
int load_fasta_device(mxg_handle *h, Assembly *a, const char *path, uint32_t n_threads);
// ... and of FASTA text that lies in HBM already (mxg_add_assembly_text_device): MXG_OK or a negative error
int load_text_device(mxg_handle *h, Assembly *a, const void *d_src, uint64_t n_bytes);
int write_tsv_device(mxg_handle *h, Assembly *a, const char *path, int with_pos, int with_strand, int with_seq);
int fetch_device_text(mxg_handle *h, Assembly *a, std::string &seq, std::vector<uint64_t> &rec_off);  // (for the host TSV writer)
uint32_t host_threads(const mxg_handle *h);
// bgzf.hip: the members of a BGZF file (bgzf_inflate.h) inflated by one launch on `st`; d_status: n_members + 1 words, word 0 ends as
// 0 or the largest BgzfStatus of any member, word 1 + m as member m's
struct BgzfMember;
int bgzf_inflate_device(mxg_handle *h, const unsigned char *d_comp, uint64_t comp_bytes, const BgzfMember *d_members, uint32_t n_members,
                        unsigned char *d_text, uint64_t text_bytes, uint32_t *d_status, hipStream_t st);
// win_out.hip: how text formed on the device reaches a file.  The file is cut into windows of WIN bytes; window c is formed in
// h->tsv_win[c & 1], copied into half c & 1 of the pinned pool and put into the file while the device forms window c + 1.
// fill(c, d_win, lo, hi) enqueues on the handle's stream what puts bytes [lo, hi) of the text at d_win.
using WinFill = std::function<int(uint64_t c, unsigned char *d_win, uint64_t lo, uint64_t hi)>;
constexpr size_t PIN_HALF = PIN_POOL_BYTES / 2;
static_assert(PIN_HALF % PIN_PIECE_BYTES == 0, "a half is whole pieces");
// the two halves of the pinned pool, the two device windows and the events of one writer; all the handle's but the events
struct WinBufs {
    mxg_handle *h;
    char *pin[2] = {nullptr, nullptr};
    hipEvent_t ev[8] = {};
    explicit WinBufs(mxg_handle *h_) : h(h_) {}
    WinBufs(const WinBufs &) = delete;
    WinBufs &operator=(const WinBufs &) = delete;
    // the pool, win_bytes <= PIN_HALF a device window, ev[0, n_plain) without timing and ev[n_plain, n_plain + n_timed) with
    int init(size_t win_bytes, uint32_t n_plain, uint32_t n_timed = 0);
    ~WinBufs();  // waits for the stream: nothing is in flight into the pool or out of the windows when the caller goes on
};
// n bytes of device memory to the START of a half of the pool (n <= PIN_HALF), enqueued on the handle's stream
int copy_pieces(mxg_handle *h, char *dst_pinned, const void *src_dev, uint64_t n);
struct WinTimes {  // seconds: taking the buffers, waiting for the device, putting
    double buffers = 0, dev_wait = 0, put = 0;
};
// `total` bytes into `of` behind its first `base` bytes, window by window (nothing at all for total = 0)
int write_windows(mxg_handle *h, OutFile &of, uint64_t total, uint64_t WIN, uint64_t base, const WinFill &fill, const char *who,
                  WinTimes *times = nullptr);
// what a fill starts from: bounds[c] = the item (node, row, block, line) whose text holds byte c * WIN of the file, for the n_win
// windows; off: the [n + 1] offsets of the n items' texts, off[0] = 0, off[n] = the file's size > (n_win - 1) * WIN
void launch_win_bounds(hipStream_t st, const uint64_t *off, uint32_t n, uint64_t WIN, uint32_t n_win, uint32_t *bounds);
// bgzf_deflate.hip: text on the device -> a BGZF file (bgzf_deflate.h).  bgzf_payload: text bytes a member (MXG_BGZF_PAYLOAD);
// bgzf_window_bytes: text bytes a window, whole units of lcm(tile, P); bgzf_write_windows: the file, window by window, deflated
// between fill and copy; bgzf_write: host bytes (mxg_bgzf_write)
uint32_t bgzf_payload(const mxg_handle *h);
uint64_t bgzf_window_bytes(uint64_t want, uint32_t tile, uint32_t P);
// (member_off, if given: where every member that holds text starts in the file)
int bgzf_write_windows(mxg_handle *h, OutFile &of, uint64_t total, uint64_t WIN, uint32_t P, const WinFill &fill, const char *who,
                       std::vector<uint64_t> *member_off = nullptr);
int bgzf_write(mxg_handle *h, const void *data, uint64_t n, const char *path);
int write_dot(mxg_handle *h, const char *path);
int dot_part_format(mxg_handle *h, uint32_t part, uint32_t n_parts, uint64_t bytes[2]);
int dot_part_write(mxg_handle *h, const char *path, uint64_t v_off, uint64_t e_off, int first, int last);
void build_rec_first(Assembly *a);
std::string py_repr_str(const std::string &s);
std::string py_repr_float(double v);
void make_hash_tab(uint32_t k, HashTab *t);
void make_init_tab(uint32_t k, std::vector<uint4> &out);

// sketch.hip
int sketch_assembly(mxg_handle *h, Assembly *a);
struct XchgPackReq {  // mxg_sketch_pack: where the sketches go once they exist (see xchg_pack for the slot layout)
    void *d_slot;
    uint64_t head_bytes;
    const uint64_t *caps;
    // mxg_sketch_pack_parts: one buffer per assembly instead, [64 bytes: int64 count, int64 records | caps[a] hashes | caps[a]
    // positions | rcaps[a] first entries of the records], packed right behind that
    // assembly's own k_emit on the stream it ran on, with an event the caller's communication stream can wait for (ev_part)
    void *const *d_parts = nullptr;
    const uint64_t *rcaps = nullptr;  // ... and room for this many records' first entries behind the 12 bytes per entry
    // mxg_sketch_dg_pack_slots: instead, every assembly's minimizers into the item slots of the partitioned graph stage (dgraph.hip),
    // right behind that assembly's k_emit, with the same per-assembly event
    const struct DgPackReq *dg = nullptr;
};
struct DgPackReq {
    uint32_t world, n_asm;
    const uint32_t *cap;      // items per (destination, assembly) slot
    const uint32_t *rec_off;  // record index shift per assembly
    void *d_send;
};
constexpr uint64_t XCHG_PART_HEAD = 64;
int sketch_assemblies(mxg_handle *h, Assembly *const *list, size_t n, bool fuse_graph = false, const XchgPackReq *xp = nullptr);
int sketch_finish(mxg_handle *h);
int upload_packed(mxg_handle *h, Assembly *a);
int prewarm_assembly(mxg_handle *h, Assembly *a);  // tables, output arrays, the filter's bitmap: when the assembly is added
int sync_sketch_to_host(mxg_handle *h, Assembly *a);
int write_sketch_bin(mxg_handle *h, Assembly *a, const char *path);  // host_io.cpp
int load_sketch_bin(mxg_handle *h, Assembly *a, const char *path, std::vector<uint64_t> &hash, std::vector<uint32_t> &pos,
                    std::vector<uint32_t> &rec);
int ensure_strand(mxg_handle *h, Assembly *a);
int pack_sketch(mxg_handle *h, Assembly *a, void *d_buf, uint64_t nmax);
int unpack_gathered(mxg_handle *h, Assembly *a, const void *d_allbuf, uint32_t world, uint64_t nmax,
                    const uint64_t *counts, const uint64_t *rec_offsets, uint64_t stride_bytes = 0);
// graph.hip
struct GraphBounds {  // fused sketch+graph call: per assembly an upper bound of its sketch and where the count will be
    uint64_t n_bound[MXG_MAX_ASSEMBLIES];
    const uint32_t *n_ptr[MXG_MAX_ASSEMBLIES];
};
// One call of the graph stage (modes: join_plan.h).  GRAPH_FULL is the whole stage.  The distributed graph (dgraph.hip) runs it in
// two halves on the OWNER's handle: GRAPH_DG_VERTICES stops after the vertices (and records the vertex id of every item),
// GRAPH_DG_EDGES resumes with the adjacency taken from messages, GRAPH_DG_EDGES_APPLIED with the adjacency already in place.
struct GraphCall {
    int mode = GRAPH_FULL;
    // the sketches are still being computed on the stream: sizes are the bounds gb->n_bound[a], the kernels read the counts from
    // gb->n_ptr[a] on the device (GRAPH_FULL: the fused sketch+graph call; GRAPH_DG_VERTICES: items in fixed slots)
    const GraphBounds *gb = nullptr;
    const void *d_msgs = nullptr;  // GRAPH_DG_EDGES: the adjacency messages (uint4 each) ...
    uint64_t n_msgs = 0;           // ... and their number
    void *d_n_vertices = nullptr;  // GRAPH_DG_VERTICES: where the vertex count goes (8 bytes on the device), if anywhere
    static GraphCall full(const GraphBounds *gb = nullptr) { return GraphCall{GRAPH_FULL, gb}; }
    static GraphCall dg_vertices(void *d_n_vertices, const GraphBounds *gb = nullptr) { return GraphCall{GRAPH_DG_VERTICES, gb, nullptr, 0, d_n_vertices}; }
    static GraphCall dg_edges(const void *d_msgs, uint64_t n_msgs) { return GraphCall{GRAPH_DG_EDGES, nullptr, d_msgs, n_msgs}; }
    static GraphCall dg_edges_applied() { return GraphCall{GRAPH_DG_EDGES_APPLIED}; }
};
int build_graph(mxg_handle *h, const GraphCall &call = GraphCall());
// The fused call's two-level join, partitioned under the sketches (MXG_PJ_EARLY=0: never).  graph_plan_early lays the join out from
// the bounds before the first filter is launched (allocations; cursors and super-counts cleared on the main stream) and says
// whether the join is one to partition early; graph_partition_early puts levels 1 and 2 of assembly a on stream st, behind that
// assembly's k_emit.  The next build_graph uses the partitions if every assembly has been through it, and partitions from
// scratch otherwise; either way it leaves nothing of the plan in force.
int graph_plan_early(mxg_handle *h, const GraphBounds &gb, bool *early);
int graph_partition_early(mxg_handle *h, uint32_t a, hipStream_t st);
void graph_drop_plan(mxg_handle *h);  // (mxg_destroy)
int xchg_pack(mxg_handle *h, void *d_slot, uint64_t head_bytes, const uint64_t *caps);
int xchg_unpack_graph(mxg_handle *h, const void *d_all, uint32_t world, uint64_t slot_bytes, uint64_t head_bytes,
                      const uint64_t *caps, const uint64_t *rec_offsets, const void *const *d_all_parts = nullptr,
                      const uint64_t *rcaps = nullptr);
int graph_to_host(mxg_handle *h);
int find_paths(mxg_handle *h, int64_t n_min);  // paths.hip
// dgraph.hip
int dg_owner_counts(mxg_handle *h, uint32_t world, uint64_t *counts);
int dg_pack_items(mxg_handle *h, Assembly *a, uint32_t world, uint32_t rec_offset, const uint64_t *starts, void *d_send);
int dg_set_items(mxg_handle *h, Assembly *a, const void *d_items, uint32_t world, const uint64_t *sec_start,
                 const uint64_t *sec_count);
int dg_item_results(mxg_handle *h, Assembly *a, const void *d_gbase, uint32_t world, const uint64_t *sec_start,
                    const uint64_t *sec_count, void *d_out);
int dg_msg_counts(mxg_handle *h, uint32_t world, const void *d_ret, const void *d_bases, uint64_t *counts);
int dg_last_shared(mxg_handle *h, const void *d_ret, void *d_out);
int dg_set_ghosts(mxg_handle *h, const void *d_all, uint32_t world, uint32_t rank);
int dg_pack_msgs(mxg_handle *h, Assembly *a, uint32_t assembly, uint32_t world, const void *d_bases, const uint64_t *starts,
                 void *d_send);
int dg_pack_slots(mxg_handle *h, Assembly *a, uint32_t ai, uint32_t rec_offset, uint32_t world, uint32_t n_asm, const uint32_t *cap,
                  void *d_send);
int dg_pack_slots_dev(mxg_handle *h, Assembly *a, uint32_t ai, const DgPackReq &rq, hipStream_t st, uint32_t mode, const uint32_t *n_ptr,
                      const uint32_t *ctrl, uint64_t out_cap, uint32_t dev_gaps, uint32_t place4);
int dg_owner_slots(mxg_handle *h, uint32_t world, uint32_t n_asm, const uint32_t *cap, const void *d_recv, void *d_nv);
// the words behind the per-assembly counts of d_nmx: [MXG_MAX_ASSEMBLIES] = a slot overflowed, then (8-byte aligned) "the owner's LDS join failed"
inline uint64_t *dg_pj_fail_word(mxg_handle *h) { return reinterpret_cast<uint64_t *>(h->d_nmx.as<unsigned char>() + 4 * MXG_MAX_ASSEMBLIES + 8); }
int dg_slot_results(mxg_handle *h, uint32_t world, uint32_t n_asm, const uint32_t *cap, const void *d_recv, const void *d_gbase,
                    void *d_out);
int dg_pack_msg_slots(mxg_handle *h, uint32_t world, uint32_t M, const void *d_ret, const void *d_bases, void *d_send);
int dg_edges_slots(mxg_handle *h, const void *d_recv, uint32_t world, uint32_t M, uint64_t *n_vertices, uint64_t *n_edges,
                   uint32_t *overflow);
int path_segments(mxg_handle *h, uint32_t assembly);
int mx_extremes(mxg_handle *h, uint32_t assembly);
int path_segments_mk(mxg_handle *h, uint32_t assembly);
// the path stage in one call (mxg_format_paths): fills h->nodes; record_length = one entry per record of the assembly;
// *overhang = the error returned is the negative overhang (h->nodes is complete all the same)
int format_paths(mxg_handle *h, uint32_t assembly, const mxg_format_params &p, const uint32_t *record_length, bool *overhang);
// the minimizer hashes of the given graph vertices, gathered on the device (mxg_vertex_hashes)
int vertex_hashes(mxg_handle *h, const uint32_t *vertices, uint64_t n, uint64_t *out);
// mk.hip: Mann-Kendall S and tie term of the runs [d_first[r], d_first[r + 1]) of d_x (device arrays, d_first with n_runs + 1
// entries; d_x is sorted in place run by run), len[r] = the runs' lengths on the host
int mk_runs(mxg_handle *h, uint32_t *d_x, const uint32_t *d_first, uint32_t n_runs, uint32_t n_total,
            const std::vector<uint32_t> &len, int64_t *s, uint64_t *tie_term);
int mk_stats(mxg_handle *h, const uint32_t *values, const uint64_t *run_first, uint64_t n_runs, int64_t *s, uint64_t *tie_term);
// overlap.hip: the cut points of every overlapping junction of the given paths (mxg_overlap_cuts)
int overlap_cuts(mxg_handle *h, Assembly *a, int assembly, uint32_t k, uint32_t w, const mxg_overlap_node *nodes,
                 const uint64_t *path_first, uint64_t n_paths, uint32_t *start_adjust, uint32_t *end_adjust, uint8_t *cut_found);
// scaffold.hip: the scaffold FASTA of the given paths and the unassigned rest (mxg_write_scaffolds)
int write_scaffolds(mxg_handle *h, Assembly *a, int assembly, const mxg_scaffold_node *nodes, const uint64_t *path_first, uint64_t n_paths,
                    int32_t overlap_gap, uint32_t flags, const char *assigned_fa, const char *unassigned_fa, const char *unassigned_bed,
                    uint32_t *lead_strip, uint32_t *tail_strip, uint64_t *n_unassigned);
// pathtext.hip: the .path and AGP text of the given paths (mxg_write_paths)
int write_paths(mxg_handle *h, Assembly *a, int assembly, const mxg_scaffold_node *nodes, const uint64_t *path_first, uint64_t n_paths,
                const uint32_t *lead_strip, const uint32_t *tail_strip, const char *first_line, const char *path_file, const char *agp_file,
                uint32_t flags);
// fai.hip: the .fai of a loaded assembly and, for a BGZF input, its .gzi (mxg_write_fai)
int write_fai(mxg_handle *h, Assembly *a, int assembly, const char *fai_path, const char *gzi_path);
// ... the .fai of a file mxg_write_scaffolds writes, every record one line: ntJoin<i>, or id:lo-hi of the assembly's record
struct FaiOutRec {
    uint64_t len;           // bases written
    uint32_t header_bytes;  // its header line with the line end
    uint32_t rec, lo, hi;   // the unassigned interval
};
int write_fai_records(mxg_handle *h, const Assembly *a, OutFile &of, const std::vector<FaiOutRec> &recs, bool ntjoin_names);
// ... and a .gzi: the members that hold text, in file order, each with its place in the file and in the text
int write_gzi(mxg_handle *h, OutFile &of, const std::vector<uint64_t> &comp_off, const std::vector<uint64_t> &text_off);
// report.hip: contiguity, composition and gaps (mxg_assembly_report; MXG_SCAF_REPORT)
int assembly_report(mxg_handle *h, Assembly *a, int assembly);  // fills h->rep_asm
struct RepSeg {  // a stretch of a scaffold file: it ends where the next one begins
    uint64_t out;   // offset of its first byte in the file
    uint32_t kind;  // 0 sequence, 1 passed over (a line end), 2 passed over and a record begins at its first byte (a header line)
    uint32_t pad;
};
// a file written window by window: begin (segs ends with {the file's size, 1}), every window once it is formed at d_win (enqueued on
// the handle's stream, waits for the first pass), end (cross-checks the bases; fills h->rep_scaf[which])
int report_file_begin(mxg_handle *h, const std::vector<RepSeg> &segs, uint64_t n_records);
int report_file_window(mxg_handle *h, const unsigned char *d_win, uint64_t lo, uint64_t hi);
int report_file_end(mxg_handle *h, int which, std::vector<uint64_t> &&rec_len, const char *path);
void report_fill(const SeqReportHost &r, std::vector<uint64_t> &scratch, mxg_seq_report *out);
// adjust.hip: relocations, --no_cut and overlapping regions of the given paths (mxg_adjust_paths); fills h->adj_*
int adjust_paths(mxg_handle *h, const mxg_adjust_node *nodes, const uint64_t *path_first, uint64_t n_paths, const mxg_adjust_params &p);
// compose.hip: two piece tables composed (mxg_compose_pieces); fills h->cmp_*
int compose_pieces(mxg_handle *h, const mxg_seq_piece *outer, const uint64_t *outer_first, uint64_t n_outer, const mxg_seq_piece *inner,
                   const uint64_t *inner_first, uint64_t n_inner);
// synteny.hip: the synteny blocks of two assemblies (mxg_synteny_blocks; fills h->syn) and their PAF text (mxg_write_synteny_paf)
int synteny_blocks(mxg_handle *h, int q, int s, const mxg_synteny_params &p, const mxg_seq_piece *pieces, const uint64_t *first, uint64_t n_records,
                   const uint32_t *query_length, const uint32_t *subject_length);
int write_synteny_paf(mxg_handle *h, const char *const *query_names, const char *path, int append, uint32_t flags = 0);
// assess.hip: chains, breakpoints and the summary of h->syn's kept blocks (mxg_synteny_assess; fills h->assess)
int synteny_assess(mxg_handle *h, const mxg_assess_params &p);
enum { AS_BP0, AS_ALIGNED = 6, AS_CHAINED, AS_COVERED, AS_NA, AS_NGA = AS_NA + 6, AS_NG = AS_NGA + 6, AS_HEADS = AS_NG + 6, AS_NBP, AS_SCRATCH, AS_WORDS };
static_assert(AS_WORDS <= 32, "mxg_handle::Assess::sum too small");
// identity.hip: the banded edit distance of explicit segments over texts the handle holds on the device (mxg_identity_segments)
int identity_segments(mxg_handle *h, int q_text, int s_text, const mxg_identity_seg *segs, uint64_t n, uint32_t max_seg, uint32_t *out_edits,
                      uint32_t *out_status);
// ... and of the segments between the anchors of h->syn's kept blocks (mxg_synteny_identity; fills h->idy)
int synteny_identity(mxg_handle *h, const mxg_identity_params &p);
// lift.hip: the index of a piece table (mxg_lift_prepare; fills h->lift), features through it (mxg_lift_intervals) and a BED file's
// (mxg_lift_bed).  BedBatch (host_io.cpp: bed_next_batch) is a batch of whole lines as the device takes it.
int lift_prepare(mxg_handle *h, const mxg_seq_piece *pieces, const uint64_t *first, uint64_t n_records, const uint32_t *source_length,
                 uint64_t n_source);
int lift_intervals(mxg_handle *h, const uint32_t *record, const uint32_t *start, const uint32_t *end, uint64_t n, uint32_t flags, bool host_parts);
int lift_bed(mxg_handle *h, const char *bed_path, const char *const *source_names, const char *const *scaffold_names, const char *lifted_path,
             const char *unlifted_path, uint32_t flags, mxg_lift_stats *stats);
struct BedFile {  // a BED file mapped for reading (host_io.cpp)
    const char *text = nullptr;
    uint64_t size = 0;
    void *map = nullptr;
    BedFile() = default;
    BedFile(const BedFile &) = delete;
    BedFile &operator=(const BedFile &) = delete;
    bool open(const char *path);
    ~BedFile();
};
struct BedBatch {
    uint64_t lo = 0, hi = 0;  // the batch is text[lo, hi)
    uint64_t lines = 0, skipped = 0;
    std::vector<uint64_t> line_off, line_len;          // per feature: its line in the file, without the line end
    std::vector<uint32_t> record, a, b;                // per feature: LFT_NONE for a name that is no record; a = b = 0 when not parsed
    std::vector<uint32_t> rest_off, rest_len, strand;  // per feature, relative to lo: column 4 on (LFT_NONE: none), column 6 if a strand
    std::vector<uint8_t> unknown;
};
// the names -> the first record of each; the batch that begins at `from` (false: the file is through)
struct BedNames;
BedNames *bed_names_make(const char *const *names, uint64_t n);
void bed_names_free(BedNames *);
bool bed_next_batch(const BedFile &f, uint64_t from, uint64_t max_bytes, const BedNames *names, BedBatch &out);
int flush_timers(mxg_handle *h);                // sketch.hip: fold the recorded event pairs into h->tm
int flags_to_host(mxg_handle *h, Assembly *a);

}  // namespace mxg
