/*
 * ntjoin_mx.h -- C-ABI of libntjoin_mx.so: the MI355X-native minimizer-sketch + minimizer-graph engine
 * that drops in for ntJoin's hot path (sketch -> uniqueness -> intersection -> adjacency edges).
 *
 * Plain C linkage, plain pointers and sizes; no C++/torch types cross this boundary.  Every function
 * returns 0 on success or a negative MXG_E* code; mxg_last_error(h) then holds a message.  The library
 * owns every buffer it returns (valid until the next call that recomputes it, or mxg_destroy);
 * a handle is not thread-safe, distinct handles are.  All device work runs on the handle's HIP stream
 * and each call blocks until its results are usable.  There is NO CPU fallback: without a usable HIP
 * device every compute entry point fails with MXG_EDEVICE.
 *
 * Reference interfaces replaced (file:line under the reference tree):
 *   mxg_add_assembly_fasta + mxg_sketch + mxg_write_tsv
 *        = `indexlr --seq --long --pos -k K -w W -t T X.fa > X.fa.kK.wW.tsv`          ntJoin:204-205
 *          (and its twin run_indexlr()                                                  bin/ntjoin_utils.py:195-202)
 *   mxg_add_assembly_tsv            = the parse half of read_minimizers()               bin/ntjoin_utils.py:167-185
 *   mxg_build_graph (uniqueness)    = the dup_mxs logic of read_minimizers()            bin/ntjoin_utils.py:182-193
 *   mxg_build_graph (intersection)  = filter_minimizers()                               bin/ntjoin_utils.py:152-165
 *   mxg_build_graph (edges/weights) = build_graph(), calc_total_weight()                bin/ntjoin_utils.py:83-141,54-56
 *   assembly order = refs (CLI order) then target, weights as double                    bin/ntjoin.py:178-186,
 *                                                                                       bin/ntjoin_assemble.py:788-807
 *   mxg_write_dot                   = Ntjoin.print_graph()                              bin/ntjoin.py:25-62
 */
#ifndef NTJOIN_MX_H
#define NTJOIN_MX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MXG_ABI_VERSION 3

/* error codes */
#define MXG_OK 0
#define MXG_EINVAL (-1)   /* bad argument / bad state                                   */
#define MXG_EIO (-2)      /* file could not be read / written / parsed                  */
#define MXG_ENOMEM (-3)   /* host or device allocation failed                           */
#define MXG_EDEVICE (-4)  /* no usable HIP device, or a HIP call / kernel failed        */
#define MXG_ELIMIT (-5)   /* an engine limit was exceeded (see mxg_last_error)          */

/* canonical-hash variant */
#define MXG_VARIANT_V2_SUM 0 /* min_hash = fwd+rev: current btllib; default                */
#define MXG_VARIANT_V1_MIN 1 /* min_hash = min(fwd,rev): what the reference's stale golden TSVs hold */

/* mxg_config.flags */
#define MXG_FLAG_DENSE_ONLY 0x1u  /* disable the sparse-candidate fast path (every k-mer is a candidate) */
#define MXG_FLAG_DROP_SEQ 0x2u    /* do not keep FASTA text on the host (mxg_write_tsv then decodes k-mers from the packed bases: upper-case) */
#define MXG_FLAG_TIMING 0x4u      /* bracket each kernel family with HIP events (read back through mxg_stats) */
#define MXG_FLAG_TIMING_FINE 0x8u /* ... one event pair per kernel (profiling; fills the per-kernel fields of mxg_stats) */
#define MXG_FLAG_ONE_SHOT 0x10u   /* the handle sketches once and writes its outputs once (the CLIs): mxg_write_outputs returns the bases, the
                                     text and the scratch buffers to the driver as soon as the TSVs are written, beside the .mx.dot writer;
                                     mxg_add_assembly_fasta leaves the file's mapping in place until mxg_destroy (or the process's end:
                                     taking 3 GB of page table apart costs ~25 ms per file) */

#define MXG_MAX_ASSEMBLIES 32

typedef struct mxg_handle mxg_handle;

typedef struct mxg_config {
    uint32_t struct_size;  /* = sizeof(mxg_config); lets the struct grow compatibly          */
    uint32_t k;            /* k-mer size, 1..1024  (ntJoin: k=32, ntJoin:36)                 */
    uint32_t w;            /* window size in k-mers, >= 1 (ntJoin: w=1000, ntJoin:33)        */
    uint32_t variant;      /* MXG_VARIANT_*                                                   */
    int32_t device;        /* HIP device ordinal, -1 = current device                         */
    uint32_t flags;        /* MXG_FLAG_*                                                      */
    void *stream;          /* hipStream_t to launch on; NULL = the library creates its own    */
    uint32_t cand_per_window; /* sparse path: expected candidates per window (0 = chosen by assembly size: 18 / 10) */
    uint32_t host_threads;    /* worker threads for file ingest and output (`indexlr -t`); 0 = min(16, cores) */
    uint32_t reserved[4];
} mxg_config;

/* host view of one assembly's ordered sketch: minimizer i is (out_hash[i], pos[i], record[i], strand[i]);
   entries are sorted by (record, pos); record indexes the assembly's FASTA records in input order. */
typedef struct mxg_sketch_view {
    uint64_t n;
    const uint64_t *out_hash;
    const uint32_t *pos;
    const uint32_t *record;
    const uint8_t *forward;      /* 1 = forward hash <= reverse hash ('+' under --strand) */
    uint64_t n_records;
    const uint64_t *record_first; /* n_records+1 offsets into the arrays above (CSR by record) */
} mxg_sketch_view;

/* device view (HBM pointers) of the same arrays, for collectives run by the caller (RCCL all-gather) */
typedef struct mxg_sketch_dview {
    uint64_t n;
    const void *out_hash; /* uint64[n] */
    const void *pos;      /* uint32[n] */
    const void *record;   /* uint32[n] */
    const void *forward;  /* uint8[n]  */
} mxg_sketch_dview;

/* per-minimizer classification after mxg_build_graph (parallel to mxg_sketch_view arrays) */
#define MXG_MX_UNIQUE 0x1u /* hash occurs exactly once in its assembly  -> key of mx_info (ntjoin_utils.py:187)  */
#define MXG_MX_SHARED 0x2u /* ... and exactly once in EVERY assembly    -> vertex of the minimizer graph          */
#define MXG_MX_INALL 0x4u  /* hash occurs (any number of times) in EVERY assembly: filter_minimizers' set rule (:152-165) */

typedef struct mxg_graph_view {
    uint32_t n_assemblies;
    uint64_t n_vertices;          /* |intersection|                                                     */
    const uint64_t *vertex_hash;  /* [n_vertices] out_hash = igraph vertex `name` (decimal string there) */
    /* [a * n_vertices + v]: where vertex v lies in assembly a  (= list_mx_info[a][name], ntjoin.py:183)  */
    const uint32_t *vertex_pos;
    const uint32_t *vertex_record;
    uint64_t n_edges;
    const uint32_t *edge_u;       /* [n_edges] vertex index, first-seen orientation (ntjoin_utils.py:101-108) */
    const uint32_t *edge_v;
    const uint32_t *edge_support; /* bit a set = assembly a (order of mxg_add_*) supports the edge      */
    const double *edge_weight;    /* sum of weights over support, in assembly order (ntjoin_utils.py:54-56) */
} mxg_graph_view;

/* mxg_stats::graph_join: which join the last mxg_build_graph ended with (low byte), and what happened on the way (bits)  */
enum mxg_graph_join {
    MXG_JOIN_LDS = 1,           /* LDS tables per hash partition                                                            */
    MXG_JOIN_LDS_TWO_LEVEL = 2, /* the same behind coarse partitions (two levels)                                           */
    MXG_JOIN_GLOBAL = 3,        /* one global table                                                                         */
    MXG_JOIN_RESIZED = 0x100,   /* coarse partitions re-sized and the join redone                                           */
    MXG_JOIN_GAVE_UP = 0x200,   /* the LDS join gave up and the global table ran (a slot that was reserved)                 */
    MXG_JOIN_EARLY = 0x400      /* mxg_sketch_graph partitioned every assembly behind its own sketch (MXG_PJ_EARLY)         */
};

typedef struct mxg_stats {
    uint32_t struct_size;
    uint32_t n_assemblies;
    uint64_t bases;            /* sum of record lengths over all assemblies                     */
    uint64_t kmers;            /* valid k-mers hashed (records with >= w valid k-mers)          */
    uint64_t minimizers;       /* sum of sketch sizes                                           */
    uint64_t candidates;       /* sparse path: candidates that reached the resolve kernel       */
    uint64_t dense_kmers;      /* k-mers re-processed by the dense (gap / fallback) path        */
    uint64_t unique;           /* minimizers flagged MXG_MX_UNIQUE                              */
    uint64_t vertices, edges;
    /* HIP-event times in ms, accumulated since mxg_create / mxg_reset_timers (MXG_FLAG_TIMING)  */
    double ms_hash;            /* hash + candidate kernels (the dominant kernel family)         */
    double ms_resolve;         /* window arg-min resolve + compaction + emit                    */
    double ms_graph;           /* uniqueness, intersection, vertex ids, edges                   */
    uint64_t launches_hash;    /* number of hash-kernel launches in ms_hash                     */
    uint64_t hash_kernel_bases;/* bases covered by those launches                               */
    /* MXG_FLAG_TIMING_FINE: ms_resolve split by kernel, ms_graph split into its three parts     */
    double ms_reorder;         /* arena entry -> exact hash -> ordered candidate slot            */
    double ms_resolve_kernel;  /* window arg-min decision per candidate                          */
    double ms_emit;            /* ordered compaction into the sketch arrays                      */
    double ms_join;            /* uniqueness + intersection (hash join, flags)                   */
    double ms_vertices;        /* vertex ids + adjacency arrays                                  */
    double ms_edges;           /* edge flags + edge compaction                                   */
    uint64_t bs_filter_bases;  /* bases covered by the bit-sliced filter (k = 32 route; 0: the rolling-hash kernel ran) */
    uint64_t graph_join;       /* the last mxg_build_graph's join: one of the three joins | what happened on the way (mxg_graph_join) */
    /* what the common route (every batch enqueued once, one host sync) could not finish: candidate floods beyond the estimate,
       stretches the device route cannot hold, output beyond its bound.  Such batches are redone one by one behind the good ones */
    uint64_t batches_redone;   /* batches redone through the synchronous route                               */
    uint64_t sync_assemblies;  /* assemblies none of whose batches could be kept                             */
    uint64_t retried_assemblies; /* assemblies whose batches went through the streams a second time, re-sized    */
    uint64_t deferred_stretches; /* candidate-free stretches sketched apart and merged in (satellites, low complexity) */
    uint64_t select_slices;    /* slices of 64 strips that went through k_bs_select (k = 32 route: bitmap -> selected minimizers
                                  in one kernel; 0: count -> reorder -> resolve ran)                                           */
    uint64_t slice_stretches;  /* candidate-free stretches (>= w k-mers without a candidate) that k_sel_stretch was handed: sketched
                                  one wave per slice right behind k_bs_select, their minimizers put into the slice's row.  Counted
                                  as entries of the batches' request arrays: a batch that fills its array (262 136 requests) counts
                                  the array's capacity, of which up to 7 entries are tombstones of a slice that did not fit       */
} mxg_stats;

/* ---- lifecycle ------------------------------------------------------------------------------- */
int mxg_abi_version(void);
int mxg_create(const mxg_config *cfg, mxg_handle **out);
void mxg_destroy(mxg_handle *h);
const char *mxg_last_error(const mxg_handle *h); /* h may be NULL: error of the last failed mxg_create */

/* ---- assemblies: call in the reference's order, references first (CLI order), target last -----
   every mxg_add_assembly_* returns the new assembly's index (>= 0) on success, a negative code on failure */
/* FASTA file (plain text; `>id comment`, multi-line, any case; non-ACGTU bytes invalidate k-mers). */
int mxg_add_assembly_fasta(mxg_handle *h, const char *name, double weight, const char *fasta_path);
/* Contig sharding for one-process-per-GPU runs: the same FASTA is opened by every rank; ALL records are registered
   (ids, lengths: record indices are global) but only the records of shard `shard` of `n_shards` are packed and
   sketched.  Shards are contiguous record ranges balanced by base count (mxg_shard_range), so concatenating the ranks'
   sketches in rank order yields the globally (record,pos)-sorted sketch. */
int mxg_add_assembly_fasta_shard(mxg_handle *h, const char *name, double weight, const char *fasta_path,
                                 uint32_t shard, uint32_t n_shards);
/* Sub-record sharding (chunks with a halo): as ..._fasta_shard, but shard s owns the BASE range
   [total*s/n, total*(s+1)/n) of the concatenated records, whatever the record boundaries: a record cut by the range is
   sketched in pieces.  Every window belongs to the shard its last k-mer starts in; a piece that does not start its
   record also loads the w valid k-mers before its first own one and withholds its first minimizer (the last minimizer
   of the piece before it), so the rank-ordered concatenation of the shards' sketches is exactly the sketch of the
   whole file: positions and record indices are those of the whole records.  mxg_assembly_shard gives the records the
   handle holds pieces of; mxg_assembly_continues says whether the first of them began on the shard before (its TSV
   line is then the continuation of that shard's last line).  Replaces a single `indexlr` process per assembly,
   reference ntJoin:204-205, for inputs with few very long records. */
int mxg_add_assembly_fasta_split(mxg_handle *h, const char *name, double weight, const char *fasta_path,
                                 uint32_t shard, uint32_t n_shards);
int mxg_assembly_continues(const mxg_handle *h, int assembly);  /* 1 / 0, negative: error */
/* records [*lo,*hi) of shard `shard`: cut points at multiples of total/n_shards of the cumulative base count
   (a record belongs to the shard its midpoint falls in).  Host only; usable without a device. */
int mxg_shard_range(const uint64_t *lengths, uint64_t n_records, uint32_t shard, uint32_t n_shards, uint64_t *lo,
                    uint64_t *hi);
/* the record range this handle sketches for an assembly ([0,n_records) unless added with ..._fasta_shard) */
int mxg_assembly_shard(const mxg_handle *h, int assembly, uint64_t *lo, uint64_t *hi);
/* Records already in host memory: record r is ascii[offsets[r] .. offsets[r+1]) with id ids[r]. */
int mxg_add_assembly_buffers(mxg_handle *h, const char *name, double weight, const uint8_t *ascii,
                             const uint64_t *offsets, const char *const *ids, uint64_t n_records);
/* Bases already resident in HBM, 2-bit packed (A=0,C=1,G=2,T=3; base i in bits 2*(i%16).. of 32-bit word
   i/16), no invalid bases.  record r starts at base rec_start[r] (a multiple of 16) and has rec_len[r]
   bases; the buffer must be readable 1 KiB past the last base.  d_packed is borrowed, not copied.
   ids may be NULL (records are then named "0","1",...). */
int mxg_add_assembly_packed_device(mxg_handle *h, const char *name, double weight, const void *d_packed,
                                   const uint64_t *rec_start, const uint64_t *rec_len,
                                   const char *const *ids, uint64_t n_records);
/* Sub-record sharding of bases already in HBM (the packed counterpart of mxg_add_assembly_fasta_split, for inputs that never
   were text: generated or produced on the device).  Every record is registered (ids, full lengths: record indices are global);
   the handle holds the bases [piece_lo[r], piece_hi[r]) of record r where piece_hi > piece_lo: base b of the record sits at
   packed index rec_start[r] + (b - (piece_lo[r] & ~15)) (rec_start a multiple of 16); piece_drop[r] bit 0 = the piece begins
   with the halo of the shard before it and withholds its first minimizer, bit 1 = the record began on an earlier shard (what
   mxg_assembly_continues reports for the handle's first record; set even when the halo reaches back to the record's base 0).  mxg_plan_split computes the pieces of shard `shard` of
   `n_shards` for N-free records (equal base ranges, a halo of w k-mers: the rule of mxg_add_assembly_fasta_split), so that the
   rank-ordered concatenation of the shards' sketches is the sketch of the whole assembly.  No counterpart in the reference
   (one process per assembly, ntJoin:204-205). */
int mxg_plan_split(const uint64_t *lengths, uint64_t n_records, uint32_t shard, uint32_t n_shards, uint32_t k, uint32_t w,
                   uint64_t *piece_lo, uint64_t *piece_hi, uint8_t *piece_drop);
int mxg_add_assembly_packed_device_pieces(mxg_handle *h, const char *name, double weight, const void *d_packed,
                                          const uint64_t *rec_start, const uint64_t *rec_len, const uint64_t *piece_lo,
                                          const uint64_t *piece_hi, const uint8_t *piece_drop, const char *const *ids,
                                          uint64_t n_records);
/* FASTA text that lies in HBM already: the n_bytes at d_text, on the handle's device, with no work pending on them.
   ntJoin is run in rounds, the scaffolds of one run being the target of the next, usually with a smaller w; a handle has one w, so
   a round is a new handle, and the texts of the old one need not go through a file to reach it.  Any FASTA is accepted:
   multi-line, CRLF, comments behind the id, no final line end.  The call copies the text device to device into the assembly's own
   padded text buffer (for a moment two copies exist: one byte per base more); the source may be freed, or its handle destroyed, as
   soon as the call returns.  From there on the assembly is in every respect what mxg_add_assembly_fasta of a file with those bytes
   gives by the device route: record ids and lengths, packed bases, run table and tile index, and so the sketch, the TSV, .fai,
   report, overlap cuts and scaffolds.  n_bytes == 0 gives an assembly without records.
   Where the file route hands a file to the host parser there is none to go to: more changes between valid and invalid bases than
   the route records (MXG_INGEST_EV_CAP) is MXG_ELIMIT, a device allocation that finds no room MXG_ENOMEM, each with a message; the
   handle is left as it was.  MXG_EINVAL: d_text == NULL with n_bytes > 0, a name in use. */
int mxg_add_assembly_text_device(mxg_handle *h, const char *name, double weight, const void *d_text, uint64_t n_bytes);
/* The FASTA text of an assembly that the device ingest route loaded (a regular plain or BGZF file, or the entry above): the
   file's own bytes (of a BGZF file: inflated), line ends included, in device memory of the handle; *n_bytes of them.  The pointer
   holds until mxg_destroy.  MXG_EINVAL for every assembly without such text, the message naming the reason: a minimizer table from
   a TSV, side-car or arrays, packed bases, MXG_HOST_INGEST=1, plain gzip, a pipe, text dropped by MXG_FLAG_DROP_SEQ or released by
   a one-shot handle, a shard or pieces of a file. */
int mxg_assembly_text(mxg_handle *h, int assembly, const void **d_text, uint64_t *n_bytes);
/* A sketch computed elsewhere: an indexlr TSV (`id \t hash:pos[:seq] ...`), parsed as read_minimizers does. */
int mxg_add_assembly_tsv(mxg_handle *h, const char *name, double weight, const char *tsv_path);
/* ... or the binary side-car mxg_write_sketch_bin left next to the TSV (the reference re-parses ~65
   bytes of text per minimizer in read_minimizers, bin/ntjoin_utils.py:167-193; the side-car is 12 bytes of raw arrays
   per minimizer).  Fails with MXG_EINVAL when the file was written with another k or hash variant. */
int mxg_add_assembly_bin(mxg_handle *h, const char *name, double weight, const char *bin_path);
/* ... or arrays (sorted by record, then pos); record_ids has n_records entries. */
int mxg_add_assembly_minimizers(mxg_handle *h, const char *name, double weight, const uint64_t *out_hash,
                                const uint32_t *pos, const uint32_t *record, uint64_t n,
                                const char *const *record_ids, uint64_t n_records);
int mxg_num_assemblies(const mxg_handle *h);
const char *mxg_assembly_name(const mxg_handle *h, int assembly);
/* id of record r of an assembly (first whitespace-delimited token of the FASTA header) */
const char *mxg_record_id(const mxg_handle *h, int assembly, uint64_t record);
uint64_t mxg_record_length(const mxg_handle *h, int assembly, uint64_t record);
uint64_t mxg_num_records(const mxg_handle *h, int assembly);
double mxg_assembly_weight(const mxg_handle *h, int assembly);

/* ---- sketch stage (replaces indexlr) --------------------------------------------------------- */
#define MXG_SKETCH_PENDING (-1) /* every assembly that has bases and no sketch yet                         */
#define MXG_SKETCH_ALL (-2)     /* every assembly that has bases (re-sketch); pipelined: one host sync for all */
int mxg_sketch(mxg_handle *h, int assembly /* index, MXG_SKETCH_PENDING or MXG_SKETCH_ALL */);
/* mxg_sketch(h, MXG_SKETCH_ALL) followed by mxg_build_graph(h) in ONE call and, in the common case, with ONE host sync: the
   graph kernels are enqueued behind the sketch kernels with upper bounds for the sizes and read the sketch sizes on the
   device.  Same results as the two calls (what ntJoin's `%.tsv` rule plus make_minimizer_graph produce, ntJoin:204-205,
   bin/ntjoin.py:189-204). */
int mxg_sketch_graph(mxg_handle *h);
int mxg_get_sketch(mxg_handle *h, int assembly, mxg_sketch_view *out);
/* (forward is NULL until the strands have been computed: mxg_get_sketch, mxg_write_tsv or mxg_compute_strands) */
int mxg_get_sketch_device(mxg_handle *h, int assembly, mxg_sketch_dview *out);
int mxg_compute_strands(mxg_handle *h, int assembly);
/* Replace an assembly's sketch by device arrays (e.g. the concatenation an all-gather produced);
   entries must be sorted by (record, pos).  The arrays are copied. */
int mxg_set_sketch_device(mxg_handle *h, int assembly, const void *d_out_hash, const void *d_pos,
                          const void *d_record, const void *d_forward, uint64_t n);
/* Exchange step of the multi-GPU path (one all-gather per assembly).  Every rank packs its sketch into
   one byte buffer of 16*nmax bytes laid out [out_hash u64 x nmax | pos u32 x nmax | record u32 x nmax] (nmax >= n,
   a multiple of 8), the caller all-gathers the buffers (RCCL), and mxg_set_sketch_gathered unpacks the `world`
   buffers in rank order -- counts[r] minimizers from rank r, record indices shifted by rec_offsets[r] -- straight into
   the assembly's sketch.  Strands do not travel (they are recomputed from bases on demand, or reported as '+'). */
int mxg_pack_sketch_device(mxg_handle *h, int assembly, void *d_buf, uint64_t nmax);
int mxg_set_sketch_gathered(mxg_handle *h, int assembly, const void *d_allbuf, uint32_t world, uint64_t nmax,
                            const uint64_t *counts, const uint64_t *rec_offsets);
/* the same when rank r's packed buffer starts at d_allbuf + r * stride_bytes (several assemblies in ONE all-gather) */
int mxg_set_sketch_gathered_strided(mxg_handle *h, int assembly, const void *d_allbuf, uint32_t world,
                                    uint64_t stride_bytes, uint64_t nmax, const uint64_t *counts,
                                    const uint64_t *rec_offsets);
/* Steady-state exchange with the counts on the device (the union path of ntjoin_amd/dist.py after its first step): a
   rank's slot = [int64 count per assembly (-1: does not fit) padded to head_bytes | caps[0] entries of assembly 0 as
   mxg_pack_sketch_device lays them out | caps[1] entries of assembly 1 | ...].  mxg_xchg_pack fills this handle's slot
   (every assembly, the counts written by the packing kernels); after ONE all-gather of the slots,
   mxg_xchg_unpack_graph on the union's handle unpacks all `world` slots with the counts read from the headers on the
   device (rec_offsets[a * world + r] = record index shift of rank r) and runs the graph stage behind it: one host sync
   for exchange + graph.  Returns 1 when some rank's header says "does not fit" (nothing usable: exchange sizes first,
   mxg_set_sketch_gathered), else as mxg_build_graph.  No counterpart in the reference (single process). */
int mxg_xchg_pack(mxg_handle *h, void *d_slot, uint64_t head_bytes, const uint64_t *caps);
/* mxg_sketch(h, MXG_SKETCH_ALL) + mxg_xchg_pack without the host sync in between: the sketches are enqueued, the packing
   kernels follow them on the stream and read the counts on the device (a sketch that did not end the common way -- arena
   overflow, candidate-free stretch, several batches -- or does not fit its slot travels as -1, so every rank falls back
   together).  The handle must have been created on the caller's stream (mxg_config.stream).  After the caller's next
   sync on that stream (mxg_xchg_unpack_graph on the union's handle does it), mxg_sketch_finish completes this handle's
   sketches (those that travelled as -1 are redone the ordinary way); until then the handle has no sketches. */
int mxg_sketch_pack(mxg_handle *h, void *d_slot, uint64_t head_bytes, const uint64_t *caps);
int mxg_sketch_finish(mxg_handle *h);
int mxg_xchg_unpack_graph(mxg_handle *h, const void *d_all, uint32_t world, uint64_t slot_bytes, uint64_t head_bytes,
                          const uint64_t *caps, const uint64_t *rec_offsets);
/* The same exchange with ONE BUFFER PER ASSEMBLY, so that an assembly's sketch can travel while the next assembly is still
   being sketched -- and with 12 bytes per minimizer instead of 16: part a = [64 bytes: int64 count (-1: does not fit), int64
   records | caps[a] hashes (u64) | caps[a] positions (u32) | rcaps[a] x u32: the first entry of every record of the sender
   (entries are in (record, position) order: the record column is a step function of the entry index, the receiver finds an
   entry's record by bisection)]; caps[a] a multiple of 8, rcaps[a] even and at least the sender's number of records;
   64 + 12 caps[a] + 4 rcaps[a] bytes.  mxg_sketch_pack_parts enqueues every assembly's sketch and packs each part right behind that assembly's own last
   kernel; mxg_part_packed_wait(h, a, stream) makes `stream` (a hipStream_t: the caller's communication stream) wait for part
   a -- the caller then issues the all-gather of part a on it, one collective per assembly.  mxg_xchg_unpack_graph_parts on
   the union's handle takes the gathered parts (d_all_parts[a] = world parts of assembly a, rank after rank) once the
   handle's stream has been made to wait for the collectives; returns as mxg_xchg_unpack_graph.  mxg_sketch_finish as
   above.  No counterpart in the reference (single process). */
int mxg_sketch_pack_parts(mxg_handle *h, void *const *d_parts, const uint64_t *caps, const uint64_t *rcaps);
int mxg_part_packed_wait(mxg_handle *h, int assembly, void *stream);
int mxg_xchg_unpack_graph_parts(mxg_handle *h, const void *const *d_all_parts, uint32_t world, const uint64_t *caps,
                                const uint64_t *rcaps, const uint64_t *rec_offsets);
/* indexlr TSV: `id \t out_hash[:pos][:+|-][:kmer] ( out_hash...)* \n`, one line per record, input order.
   path "-" = stdout. */
int mxg_write_tsv(mxg_handle *h, int assembly, const char *path, int with_pos, int with_strand,
                  int with_seq);
/* the same sketch as raw arrays (record ids, lengths, out_hash, pos): read back by mxg_add_assembly_bin */
int mxg_write_sketch_bin(mxg_handle *h, int assembly, const char *path);

/* ---- graph stage (replaces read_minimizers' uniqueness, filter_minimizers, build_graph) -------- */
int mxg_build_graph(mxg_handle *h);
/* flags[i] (MXG_MX_*) for minimizer i of the assembly's sketch */
int mxg_get_mx_flags(mxg_handle *h, int assembly, const uint8_t **flags, uint64_t *n);
int mxg_get_graph(mxg_handle *h, mxg_graph_view *out);
/* `.mx.dot` as Ntjoin.print_graph writes it (HEAD syntax); vertex/edge line order: vertices in first-assembly
   order, edges in first-seen order (the reference's own order is unspecified: python set order). */
int mxg_write_dot(mxg_handle *h, const char *path);
/* The .mx.dot written by several processes that each hold the WHOLE graph (one process per GPU, union route): part `part` of
   `n_parts` = the vertex lines [nv part / n, nv (part + 1) / n) and the edge lines likewise.  mxg_dot_part_format formats the
   part's two segments into memory and reports their sizes (bytes[0] vertices, bytes[1] edges); the caller exchanges the sizes
   (one small all-gather) and every process writes its segments at
       v_off = 10 + sum of bytes[0] of the parts before it,   e_off = 10 + sum of ALL bytes[0] + sum of bytes[1] of the parts before it
   (10 = strlen("graph G {\n"), written by the part with first != 0; the part with last != 0 appends "}\n").  The file must not
   be truncated by anybody after the first write.  Together the parts are byte for byte what mxg_write_dot writes.
   No counterpart in the reference (bin/ntjoin.py:25-67 is one process). */
int mxg_dot_part_format(mxg_handle *h, uint32_t part, uint32_t n_parts, uint64_t bytes[2]);
int mxg_dot_part_write(mxg_handle *h, const char *path, uint64_t v_off, uint64_t e_off, int first, int last);
/* The text outputs of a whole run in one call: <prefix>.mx.dot (mxg_write_dot) formatted by the host workers WHILE the TSVs of
   the assemblies (mxg_write_tsv with these flags; tsv_paths[a] == NULL: none for assembly a) are formatted on the device and
   written out -- the two use different resources (host threads / GPU + one writer), so a run's text output takes the longer
   of the two instead of their sum.  Same bytes as the separate calls.  Replaces the tail of reference ntJoin:204-205 (the
   `> $@` of every indexlr recipe) and bin/ntjoin.py:25-67 (print_graph) when one process does both. */
int mxg_write_outputs(mxg_handle *h, const char *dot_path, const char *const *tsv_paths, int with_pos, int with_strand,
                      int with_seq);

/* ---- next row: linear paths through the minimizer graph -------------------------------------------
   What the reference computes with igraph right after the graph (bin/ntjoin_assemble.py:759,779): filter_graph_global
   with minimum edge weight n (bin/ntjoin.py:80-89), then per component the branch filtering with rising thresholds
   (filter_graph :69-77, find_paths_process :137-161), circular components opened (check_circularity :113-135), source
   and target chosen by position in the highest-weight assembly (determine_source_vertex :91-103); a sub-component yields
   a path iff it is a simple chain.  Vertices are indices into mxg_graph_view; paths are ordered by source vertex. */
typedef struct mxg_paths_view {
    uint64_t n_components;           /* components of the globally filtered graph (bin/ntjoin.py:166-167)         */
    uint64_t n_paths;
    const uint64_t *path_first;      /* [n_paths+1] offsets into path_vertex                                     */
    const uint32_t *path_vertex;     /* vertex indices, source -> target                                          */
    const uint32_t *path_component;  /* [n_paths] id of the component of the globally filtered graph it came from */
} mxg_paths_view;
int mxg_find_paths(mxg_handle *h, int64_t min_edge_weight /* ntJoin's n */, mxg_paths_view *out);

/* ---- next row: what the scaffolder derives from the paths for one assembly (the target) ------------
   mxg_mx_extremes   = find_mx_min_max (bin/ntjoin_assemble.py:688-702): per record of the assembly, the smallest and
                       largest position among its minimizers that are graph vertices (no vertex: min = 2^32-1, max = 0).
   mxg_path_segments = the grouping loop of format_path (bin/ntjoin_assemble.py:175-218): every path of the last
                       mxg_find_paths is cut into runs of consecutive vertices lying on the same record of `assembly`;
                       per run what determine_orientation (:30-50) and calc_start/end_coord (:52-65) need. */
typedef struct mxg_segments_view {
    uint64_t n_segments;             /* in path order, then position in the path                                  */
    const uint32_t *seg_path;        /* index into mxg_paths_view                                                 */
    const uint32_t *seg_record;      /* record (contig) of the assembly                                           */
    const uint32_t *seg_first;       /* offset of the run's first vertex in mxg_paths_view.path_vertex            */
    const uint32_t *seg_stat;        /* 5 per run: vertices, min pos, max pos, increasing pairs, decreasing pairs */
} mxg_segments_view;
int mxg_path_segments(mxg_handle *h, int assembly, mxg_segments_view *out);
/* --mkt: determine_orientation (bin/ntjoin_assemble.py:30-50) decides every run that is not strictly monotone by
   pymannkendall.original_test(positions) (:37-40), whose decision reads two exact integers of the run x_0..x_{n-1}:
       s = sum over i < j of sign(x_j - x_i),   tie_term = sum over groups of t equal values of t(t-1)(2t+5)
   (the test's variance is (n(n-1)(2n+5) - tie_term) / 18).  O(n log^2 n) per run, on the device.
   mxg_path_segments_mk: s and tie_term of every run of the last mxg_path_segments, in its order, over the same positions
                         (MXG_EINVAL if there was none since the last mxg_find_paths, or it was for another assembly); host
                         copies owned by the handle, like mxg_segments_view.
   mxg_mk_stats:         the same for runs the caller gives: run r = values[run_first[r] .. run_first[r+1]) (run_first has
                         n_runs + 1 entries; runs of 0 or 1 values give 0, 0), results written to s[n_runs], tie_term[n_runs].
   A tie term beyond 2^64 - 1 (a group of more than about 2*10^6 equal values) fails with MXG_ELIMIT. */
int mxg_path_segments_mk(mxg_handle *h, int assembly, const int64_t **s, const uint64_t **tie_term, uint64_t *n_segments);
int mxg_mk_stats(mxg_handle *h, const uint32_t *values, const uint64_t *run_first /* n_runs + 1 */, uint64_t n_runs,
                 int64_t *s, uint64_t *tie_term);
int mxg_mx_extremes(mxg_handle *h, int assembly, const uint32_t **min_pos, const uint32_t **max_pos, uint64_t *n_records);

/* ---- the path stage in one call: nodes, orientations and gap sizes of all paths -------------------------------------
   What format_path (bin/ntjoin_assemble.py:175-218) builds per path with determine_orientation (:30-50), calc_start_coord /
   calc_end_coord (:52-65) and calculate_gap_size (:67-113), for every path of the last mxg_find_paths, in its order, from
   what the graph and path stages left on the device.  The runs are those of mxg_path_segments (whose host copies, and those
   of mxg_mx_extremes, this call refreshes for `assembly` as well); a run of one vertex has no orientation; longer runs are
   '+' / '-' when strictly increasing / decreasing, otherwise by the m rule in fp64 as the reference forms it
   (inc / double(n - 1) * 100 >= m: '+', else 100 - that >= m: '-') or, with mkt, by the Mann-Kendall decision below on the
   statistics of mxg_path_segments_mk (decided on the host with libm, one byte per run goes back to the device).
   Nodes are the runs with an orientation, in path order:
       start = min pos == the record's smallest vertex position ? 0 : min pos
       end   = max pos == the record's largest vertex position ? record length : max pos + k        (k: the handle's)
   Gap between node i and node i + 1 of one path, u = last vertex of node i's run, v = first vertex of node i + 1's run (the
   runs without orientation between them make the stretch u..v longer than one edge): common = AND of the support masks of
   the path's edges from u to v; common == 0: gap = raw = g; otherwise
       mean = (sum over the assemblies of common of |pos_b[v] - pos_b[u]|) / count - k         (integer division)
       a = node i '+' ? end_i - pos[u] - k : pos[u] - start_i,   b = node i+1 '+' ? pos[v] - start_i+1 : end_i+1 - pos[v] - k
       raw = mean - a - b,   gap = max(raw, g), then min(gap, G) when G > 0.
   record_length[r] replaces the lengths the handle holds (NULL: the handle's own).  The arrays of the view are host copies
   owned by the handle, valid until the next call of this function or mxg_destroy.
   MXG_EINVAL: no graph or no paths, assembly out of range, struct_size too small, record_length == NULL for an assembly
   that holds no lengths (TSV, side-car or minimizer input), or some a < 0 or b < 0 (the reference's "Gap distance estimation
   less than 0": lengths shorter than the minimizers imply).  In that last case the kernels have finished: the message names
   the first such path and node as "path <p> node <i>", the view is filled (gap_size = raw_gap_size = 0 at every such
   junction) and the handle stays usable.  No other error writes to the view: a caller that zeroes it first tells the two apart by
   node_first != NULL.
   mxg_mk_orientation: '+', '-' or '?' for a run of n values with Mann-Kendall score s and the given tie term:
   pymannkendall.original_test's z and p as determine_orientation reads them (:37-40), evaluated on the host. */
typedef struct mxg_format_params {
    uint32_t struct_size;
    int64_t  g;        /* minimum gap size (ntJoin -g) */
    int64_t  G;        /* maximum gap size, 0 = none (-G) */
    double   m;        /* percentage rule (-m) */
    uint32_t mkt;      /* != 0: --mkt */
} mxg_format_params;

typedef struct mxg_path_nodes_view {
    uint64_t n_paths, n_nodes;
    const uint64_t *node_first;      /* [n_paths + 1]; a path whose runs are all '?' has an empty range */
    const uint32_t *record, *start, *end, *contig_size;
    const uint8_t  *reverse;         /* 0 = '+', 1 = '-' */
    const uint32_t *first_vertex, *terminal_vertex;  /* vertex indices: first_mx / terminal_mx */
    const int64_t  *gap_size, *raw_gap_size;         /* to the NEXT node; 0, 0 on a path's last node */
    const uint32_t *segment;         /* index of the run in mxg_segments_view order */
} mxg_path_nodes_view;

int mxg_format_paths(mxg_handle *h, int assembly, const mxg_format_params *p,
                     const uint32_t *record_length /* NULL: the handle's own */, mxg_path_nodes_view *out);
char mxg_mk_orientation(uint64_t n, int64_t s, uint64_t tie_term);   /* '+', '-' or '?' */
/* The minimizer hashes of n graph vertices (mxg_graph_view.vertex_hash[vertices[i]] -> out[i]): what names first_mx / terminal_mx
   of the nodes above (the reference's vertex names, bin/ntjoin_assemble.py:205-206), gathered on the device, so that the graph's
   host mirror (mxg_get_graph: every array of the graph) is not made for them.  MXG_EINVAL: no graph, a vertex out of range. */
int mxg_vertex_hashes(mxg_handle *h, const uint32_t *vertices, uint64_t n, uint64_t *out);

/* ---- next row (f5): the overlap stage's cut points -------------------------------------------------------------------
   What the reference's default run (overlap=True, ntJoin:39) computes between the paths and the scaffold sequence: the
   joined segments are written to <prefix>.segments.fa with their middles hard-masked (print_scaffolds,
   bin/ntjoin_assemble.py:556-578; get_valid_regions, bin/ntjoin_overlap.py:98-114), that file is sketched with
   btllib.Indexlr at (overlap_k, overlap_w) (adjust_for_trimming :468-499), every node keeps the minimizers of its
   overlapping ends that occur once (tally_minimizers_overlap :501-516), and for every junction with a negative raw gap
   merge_overlapping (bin/ntjoin_overlap.py:20-88) builds an igraph graph of the two filtered lists and picks the cut.
   Here: no file, no graph; the segments' ends are sketched from the assembly's packed bases.
   Node i of path p is nodes[path_first[p] + i]: the bases [start, end) of `record`, reverse-complemented when `reverse`;
   raw_gap is the raw gap size to the NEXT node of the path (read for every node, the last one included, as the reference's
   position filter reads it).  Paths hold the nodes with an orientation only and have at least two of them (:562-568).
   Results per node: start_adjust / end_adjust as PathNode holds them (0 = none, bin/path_node.py:41-45), and
   cut_found[node] = 1 when the junction between the node and the next one got a cut (end_adjust of the node and
   start_adjust of the next; either may be 0 and still be a cut).  k and w are the call's own (ntJoin: --overlap_k 15
   --overlap_w 10), the hash variant is the handle's.  The assembly must hold bases; sketches, graph and paths of the
   handle are left as they are.  MXG_EINVAL: an assembly without bases, start >= end, end beyond the record, a path of
   fewer than two nodes, a segment whose first or last base is invalid (the reference asserts there).  MXG_ELIMIT: k > 256
   or w > 4096. */
typedef struct mxg_overlap_node {
    uint32_t record, start, end;
    int32_t raw_gap;
    uint8_t reverse, pad[3];
} mxg_overlap_node;
int mxg_overlap_cuts(mxg_handle *h, int assembly, uint32_t k, uint32_t w, const mxg_overlap_node *nodes,
                     const uint64_t *path_first /* n_paths + 1 */, uint64_t n_paths, uint32_t *start_adjust,
                     uint32_t *end_adjust, uint8_t *cut_found /* per node: junction to the next */);

/* ---- next row (f6): the scaffold FASTA of all paths, and what no path took ------------------------------------------------
   What the reference's print_scaffolds loop (bin/ntjoin_assemble.py:580-613; get_fasta_segment :327-332, get_adjusted_sequence
   :519-527, join_sequences :407-439) and print_unassigned (:628-658: bedtools complement + bedtools getfasta) produce by reading
   the target FASTA a second time and slicing Python strings.  Here: from the text the handle already holds, on the device.
   Node i of path p is nodes[path_first[p] + i], as print_scaffolds holds it at :580 (orientation '+' / '-' only, the last node's
   gap already zeroed by the caller as check_terminal_node_gap_zero does).  With T = the record's bases [start, end)
   (reversed and mapped through the table of bin/ntjoin_utils.py:145-150 when `reverse`: ACGTUNMRWSYKVHDB -> TGCAANKYWSRMBDHV,
   the same in lower case, any other byte unchanged), L = end - start and g = gap_size, the node's piece is
     overlap_gap < 0 (overlap stage off):  T + "N" * g
     overlap_gap >= 0:  T[start_adjust : e] with e = end_adjust ? end_adjust : L (empty when start_adjust >= e), followed,
                        if g > 0, by "N" * g when e == L and by "N" * overlap_gap otherwise.
   The scaffold of path p is the concatenation of its pieces with N/n stripped from the left of the first piece and from the
   right of the last one; the two counts come back in lead_strip[p] / tail_strip[p] (the reference moves the .path coordinates
   by them).  assigned_fa gets ">ntJoin<p>\n<sequence>\n" per path, paths numbered in input order (:600-603).
   Unassigned: per record, in record order, the complement of the union of the nodes' [start, end) (unadjusted, unstripped: the
   Bed entries of :589) within [0, record length), zero-length intervals left out; unassigned_bed gets "id\tstart\tend\n" per
   interval, unassigned_fa ">id:start-end\n<text>\n" with N/n stripped from both ends of the text (the header keeps the
   interval's coordinates; an interval left empty is dropped from the FASTA, not from the BED); *n_unassigned = records written
   to unassigned_fa.  Either file name may be NULL, as may lead_strip, tail_strip and n_unassigned.
   Bytes are the record's own spelling with line ends removed; MXG_SCAF_FOLD_CASE folds a-z to A-Z in assigned_fa only.
   MXG_EINVAL (nothing is written): an assembly whose text the handle does not hold (TSV / side-car / minimizer / packed-device
   input, a shard or pieces of a file, text dropped by MXG_FLAG_DROP_SEQ or released by a one-shot handle), start >= end, end
   beyond the record, a path of fewer than two nodes, end_adjust > L, a first or last piece whose text part is empty or N/n
   throughout (the reference asserts there).  MXG_ELIMIT: 2^31 nodes or more.  Sketches, graph and paths are left as they are. */
#define MXG_SCAF_FOLD_CASE 0x1u
/* MXG_SCAF_BGZF: assigned_fa and unassigned_fa are BGZF files (what `bgzip` writes: a chain of gzip members of at most 65 280 bytes
   of text each, the 28-byte end marker behind the last) of exactly the bytes the call writes without the flag, deflated on the
   device (literals only: about 2.25 bits a base); the BED, the strips and every return value are as without it. */
#define MXG_SCAF_BGZF 0x2u
/* MXG_SCAF_FAI: beside assigned_fa write <assigned_fa>.fai and beside unassigned_fa, when given, <unassigned_fa>.fai: the index
   `samtools faidx` makes of the file (the reference's `%.fai: %` rule, ntJoin:152-153, 207-208; format under mxg_write_fai).  Every
   record of these files is one line: "name\tlen\toffset\tlen\tlen+1\n", name = ntJoin<p> or id:start-end, len = the bases written,
   offset = where they start in the (uncompressed) file; an interval dropped from the FASTA has no line.  With MXG_SCAF_BGZF also
   <...>.gzi for each (format under mxg_write_fai).  FASTA, BED, strips and return values are as without the flag. */
#define MXG_SCAF_FAI 0x4u
/* MXG_SCAF_REPORT: every window of assigned_fa and unassigned_fa goes through the report's two passes once it is formed in device
   memory and before it leaves (plain and BGZF alike); mxg_scaffold_report hands the reports out.  The record lengths the piece
   table knows are checked against the bases the device counts (MXG_EDEVICE on a mismatch).  Every file is byte for byte what the
   call writes without the flag; without it nothing more is launched. */
#define MXG_SCAF_REPORT 0x8u
/* MXG_SCAF_KEEP: the bytes of assigned_fa followed by the bytes of unassigned_fa -- the all.scaffolds.fa that `cat`
   makes of them, the target of the next round -- are also left in a device buffer of the handle: the uncompressed text, also under
   MXG_SCAF_BGZF; the assigned part folded under MXG_SCAF_FOLD_CASE as its file is.  The unassigned side is always computed with this
   flag.  The buffer holds until the handle's next mxg_write_scaffolds or mxg_destroy.  With the flag, assigned_fa, unassigned_fa and
   unassigned_bed may all be NULL; what is not named is not written.  MXG_SCAF_BGZF, MXG_SCAF_FAI or MXG_SCAF_REPORT without
   assigned_fa is MXG_EINVAL.  Files that are named are byte for byte what they are without the flag; without it nothing more is
   launched. */
#define MXG_SCAF_KEEP 0x10u
typedef struct mxg_scaffold_node {
    uint32_t record, start, end;       /* [start, end) of the record */
    uint32_t gap_size;                 /* Ns behind the node (PathNode.gap_size) */
    uint32_t start_adjust, end_adjust; /* as mxg_overlap_cuts returns them; 0 = none */
    uint8_t  reverse, pad[3];
} mxg_scaffold_node;
int mxg_write_scaffolds(mxg_handle *h, int assembly, const mxg_scaffold_node *nodes,
                        const uint64_t *path_first /* n_paths + 1 */, uint64_t n_paths,
                        int32_t overlap_gap /* < 0: overlap stage off */, uint32_t flags, const char *assigned_fa,
                        const char *unassigned_fa /* may be NULL */, const char *unassigned_bed /* may be NULL */,
                        uint32_t *lead_strip, uint32_t *tail_strip /* [n_paths] */, uint64_t *n_unassigned);
/* The N/n stripped from the left and the right of every unassigned interval by the last successful mxg_write_scaffolds of the
   handle that computed the unassigned side (any of unassigned_fa, unassigned_bed, n_unassigned given), one entry per line of the
   BED, in its order; an interval that is N throughout has lead = its length and tail = 0.  What write_agp_unassigned
   (bin/ntjoin_assemble.py:379-404) recomputes from the text of every record (len_diff_start, len_diff_end).  The arrays are the
   handle's and hold until its next mxg_write_scaffolds. */
int mxg_scaffold_strips(mxg_handle *h, const uint32_t **lead_strip, const uint32_t **tail_strip, uint64_t *n_intervals);
/* What the last mxg_write_scaffolds kept under MXG_SCAF_KEEP: the text in device memory, its bytes and (n_records may be NULL) its
   records.  MXG_EINVAL when that call kept none (no flag, or it failed).  What the records are made of: mxg_scaffold_pieces. */
int mxg_scaffold_text(mxg_handle *h, const void **d_text, uint64_t *n_bytes, uint64_t *n_records);

/* ---- next row (f9): FASTA indexes -----------------------------------------------------------------------------------------------
   <fasta>.fai as `samtools faidx` writes it (the reference's `%.fai: %` rule, ntJoin:152-153, 207-208: `$(target).fai` and one per
   reference), from the text the handle holds.  One line per record, in file order: "NAME\tLENGTH\tOFFSET\tLINEBASES\tLINEWIDTH\n".
   With T = the record's sequence text (from behind its header line to the next header's '>' or the end of the text) split at '\n':
   NAME = the record's id; OFFSET = where T starts (for BGZF input: in the inflated text); LINEWIDTH = bytes of the first line with its
   line end ("\n" or "\r\n"; the last line of the file may have none); LINEBASES = its bytes in 0x21 .. 0x7E; LENGTH = the bytes of T
   in 0x21 .. 0x7E; empty T: "NAME\t0\tOFFSET\t0\t0".  A later record of a name already seen is left out (one line on stderr).
   Accepted: every line but the last non-empty one has exactly the first line's bytes; the last non-empty line has 1 .. LINEBASES
   bases and the same kind of line end, or none at the end of the text; empty lines follow only behind the last record of the file;
   every byte of a line is in 0x21 .. 0x7E but a '\r' directly in front of the '\n'.  Anything else is MXG_EINVAL (samtools'
   "different line length in sequence", taken conservatively): nothing is left at fai_path, and the message names the record and the
   byte offset of the first offending line.
   gzi_path (may be NULL): the .gzi of a BGZF input -- little-endian, a uint64 count N, then N pairs {compressed offset, uncompressed
   offset}, one for every member that holds text except the first, in file order.
   MXG_EINVAL also: an assembly whose text the handle does not hold on the device (TSV / side-car / minimizer / packed input,
   MXG_HOST_INGEST=1, plain gzip, a pipe, MXG_FLAG_DROP_SEQ, text released by a one-shot handle, a shard or pieces of a file);
   gzi_path for an assembly that did not come from BGZF.  MXG_FAI_WIN: bytes of the index formed per window (default and at most
   64 Mi). */
int mxg_write_fai(mxg_handle *h, int assembly, const char *fai_path, const char *gzi_path);

/* The n bytes at data (host memory) written to `path` as a BGZF file, deflated on the device as the scaffold files of
   MXG_SCAF_BGZF are: member j holds bytes [j P, j P + P) with P = 65 280 (the environment's MXG_BGZF_PAYLOAD, 1 .. 65 280, if set),
   the end marker follows; n = 0 gives the end marker alone.  MXG_EINVAL: a null argument; MXG_EIO: the file. */
int mxg_bgzf_write(mxg_handle *h, const void *data, uint64_t n, const char *path);

/* ---- next row (f10): the assembly report -- contiguity, base composition and N gaps -------------------------------------------
   What the reference's `analysis` target asks QUAST for with --split-scaffolds (ntJoin:158-161, 244-252), as far as it needs no
   alignment, from the text the handle holds and from the scaffold files on their way out.
   A FASTA file is a list of records.  A record's BASES are the bytes of its sequence text other than '\n' and '\r'; header lines are
   no part of it.  Classes of a base: A, C, G in either case; T in either case, U/u counted as T; N for N/n; OTHER for anything
   else.  lower = the bases in 'a' .. 'z'.
   An N RUN is a maximal stretch of N/n bases inside one record: line ends do not interrupt it, a record border ends it.  A GAP is
   an N run of at least min_gap bases (default 10, QUAST's rule for --split-scaffolds).  A record's CONTIGS are what is left of it
   when its gaps are cut out; shorter N runs stay inside contigs, a contig of 0 bases is none.
   The CONTIGUITY BLOCK of a multiset of lengths: n = how many; over those of at least min_len (default 500): n_min, sum, min, max
   and, for x in {50, 75, 90}, with the lengths sorted descending and S_j the sum of the first j: Lx = the smallest j with
   100 S_j >= x sum, Nx = the j-th length.  Nothing selected: zeros.  Exact 64-bit integers throughout.
   A REPORT holds n_records and bases, the six class counts and lower, n_gaps / gap_bases / max_gap, the contiguity block of the
   record lengths (scaffold) and of the contig lengths (contig), and the two lists behind them: every gap's and every contig's
   length, in no particular order.  The lists are the handle's and hold until its next mxg_assembly_report / mxg_scaffold_report /
   mxg_write_scaffolds with MXG_SCAF_REPORT. */
typedef struct mxg_contiguity {
    uint64_t n, n_min, sum, min, max;
    uint64_t n50, l50, n75, l75, n90, l90;
} mxg_contiguity;
typedef struct mxg_seq_report {
    uint32_t struct_size; /* sizeof(mxg_seq_report), set by the caller */
    uint32_t reserved;
    uint64_t min_gap, min_len; /* the parameters the report was made with */
    uint64_t n_records, bases;
    uint64_t a, c, g, t, n, other, lower;
    uint64_t n_gaps, gap_bases, max_gap;
    mxg_contiguity scaffold, contig;
    const uint64_t *gap_len;    /* [n_gaps] */
    const uint64_t *contig_len; /* [contig.n] */
} mxg_seq_report;
/* min_gap (0: MXG_EINVAL) and min_len (0 is allowed) of every later report of the handle. */
int mxg_set_report_params(mxg_handle *h, uint64_t min_gap, uint64_t min_len);
/* The report of a loaded assembly, computed on the device from its text: of a file the device ingest read (with its line ends) or
   of host-ingested text (MXG_HOST_INGEST=1, plain gzip).  MXG_EINVAL: an assembly whose text the handle does not hold (a minimizer
   table from a TSV, side-car or arrays, packed bases, text dropped by MXG_FLAG_DROP_SEQ or released by a one-shot handle, a shard
   or pieces of a file); out->struct_size too small.  MXG_REPORT_SCAN_W (tests): work items per block of the scan, 2 .. 256. */
int mxg_assembly_report(mxg_handle *h, int assembly, mxg_seq_report *out);
/* The reports of the files the last mxg_write_scaffolds with MXG_SCAF_REPORT wrote.  which: */
#define MXG_REPORT_ASSIGNED 0
#define MXG_REPORT_UNASSIGNED 1
#define MXG_REPORT_ALL 2 /* the file that holds both: counts added, contiguity over the merged lists */
/* MXG_EINVAL: no such write came before (or it failed, or it wrote no unassigned file and that one is asked for). */
int mxg_scaffold_report(mxg_handle *h, int which, mxg_seq_report *out);

/* ---- next row (f7): the paths adjusted for relocations, --no_cut and overlapping regions ------------------------------------
   What the reference's main_scaffolder (bin/ntjoin_assemble.py:751-786) does to the PathNodes between format_path and the
   trimming / printing of the scaffolds, for all paths in one call, in its order:
     1  tally_incorporated_segments (:220-230): per contig the set of (start, end) of the nodes of every path with two nodes or more;
     2  merge_relocations (:126-172) over all paths in path order: adjacent nodes of one contig, both '+' and ascending or both '-'
        and descending, become one (the chain's head takes the end / start, terminal_mx / first_mx and gap of the node merged into
        it) unless a segment of the contig's set that shares neither end with either node touches the joined region (:115-123);
     3  with no_cut, adjust_paths (:266-305): subsumed nodes leave (:253-264), another merge_relocations, then per node: the
        contig's best region (:233-244) or only node becomes the whole contig, any other node of a contig in several nodes leaves
        and, strictly inside its path, adds its length to the gap of the last kept node (clamped to G when G > 0);
     4  tally_intersecting_segments (:661-686): per contig the segments of its set that intersect another one (half-open:
        max(starts) < min(ends)), ascending by (start, end), resolved by OverlapRegion.find_non_overlapping (bin/overlap_region.py);
        equal start: the smaller end first -- bedtools' sort leaves that order open, the rule is this library's;
     5  merge_relocations again (print_scaffolds :550);
     6  remove_overlapping_regions (:451-466): a node whose exact (start, end) phase 4 resolved is dropped or takes the replacement;
     7  check_terminal_node_gap_zero (:441-448): gap 0 on every path's last node whose ori is not '?'.
   Node i of path p is nodes[path_first[p] + i] as format_path made it; `record` is any index below 2^28 that names the target
   contig (nodes of one contig carry one index), first_mx / terminal_mx are opaque tags.  The result is what print_scaffolds holds
   at :555: the nodes of every path (a path may come back with one node or none), and per node the index of the input node it is
   (the head of its merged chain).  The arrays of `out` are host copies owned by the handle, valid until its next
   mxg_adjust_paths.  Sketches, graph and paths of the handle are left as they are.
   MXG_EINVAL: ori above 2, start >= end, path_first not increasing from 0; and, naming "path <p> node <i>" of the input, the merge
   step at which the reference raises KeyError: a segment that an earlier merge already took out of its contig's set (two nodes with
   the same contig, start and end, one of which merges).  MXG_ELIMIT: a record index of 2^28 or more, 2^31 nodes or paths or more. */
typedef struct mxg_adjust_node {           /* one PathNode as format_path made it */
    uint32_t record, start, end, contig_size;
    uint64_t first_mx, terminal_mx;        /* opaque tags (the minimizer hashes); copied on merges, compared by is_best_region */
    int64_t  gap_size, raw_gap_size;
    uint8_t  ori, pad[7];                  /* 0 '+', 1 '-', 2 '?' */
} mxg_adjust_node;
typedef struct mxg_adjust_params { uint32_t struct_size; uint32_t no_cut; int64_t G; } mxg_adjust_params;
typedef struct mxg_adjusted_view {         /* host copies owned by the handle, valid until the next call */
    uint64_t n_paths, n_nodes;
    const uint64_t *node_first;            /* [n_paths + 1]; a path may come back empty */
    const mxg_adjust_node *nodes;          /* the paths as print_scaffolds holds them at :555 */
    const uint64_t *source;                /* per output node: index of the input node it is (the head of its merged chain) */
} mxg_adjusted_view;
int mxg_adjust_paths(mxg_handle *h, const mxg_adjust_node *nodes, const uint64_t *path_first /* n_paths + 1 */, uint64_t n_paths,
                     const mxg_adjust_params *p, mxg_adjusted_view *out);

/* ---- next row (f8): the .path file and the AGP of all paths --------------------------------------------------------------
   What the reference's print_scaffolds writes per path with Python strings (bin/ntjoin_assemble.py:605-610), what write_agp
   (:346-376) parses back out of that string with two regular expressions per component, and write_agp_unassigned (:379-404).
   Here: formatted on the device from the node array, in the state mxg_write_scaffolds takes it (orientation '+' / '-' only, at
   least two nodes per path, the last node's gap already zero), and the strips that call returned; no sequence text is read and
   `end` is not compared with the record's length (mxg_write_scaffolds has done that).
   Per node, after the strips (the first node of a path loses lead_strip[p] at its start if '+', at its end if '-'; the last node
   loses tail_strip[p] at its end if '+', at its start if '-'; join_sequences :413-436), with L = end - start and
   e = end_adjust ? end_adjust : L, the adjusted interval [s, t) is (bin/path_node.py:41-61)
     '+':  (start + start_adjust, end - (L - e))        '-':  (start + (L - e), end - start_adjust).
   path_file: "first_line\n", then per path "ntJoin<p>\t<id><ori>:<s>-<t> <gap>N <id><ori>:<s>-<t> ... <id><ori>:<s>-<t>\n"; the
   last node's gap is left out whatever its value (:607).  id = the record's id as the handle holds it, gap = gap_size.
   agp_file (may be NULL): nine tab-separated columns per component in path order; a node gives
   "ntJoin<p> at at+n-1 part W id s+1 t ori" with n = t - s, the gap behind every node but the last
   "ntJoin<p> at at+n-1 part N n scaffold yes align_genus" with n = gap (a gap of 0 still has its line, ending at at - 1, as the
   reference writes it); `at` starts at 1 per path and advances by n (a 64-bit sum), `part` counts the components from 1.
   MXG_PATHS_AGP_UNASSIGNED: behind the last path, for every interval [lo, hi) of the handle's last mxg_write_scaffolds that
   computed the unassigned side (of this assembly), in BED order, with n = hi - lo - lead - tail > 0:
   "id:lo-hi 1 n 1 W id lo+1+lead lo+lead+n +".
   MXG_EINVAL (nothing is written): a path of fewer than two nodes, start >= end, end_adjust > L, a record index outside the
   assembly, path_first not increasing from 0, path_file == NULL, MXG_PATHS_AGP_UNASSIGNED without such an mxg_write_scaffolds
   before it, and, naming "path <p> node <i>", an adjusted interval that is empty or inverted after the strips.  MXG_ELIMIT: 2^31
   nodes or more.  n_paths == 0 is valid (path_file holds its first line, agp_file the unassigned lines or nothing).  Sketches,
   graph and paths of the handle are left as they are.  MXG_PATH_WIN (test knob): bytes of text per device window. */
#define MXG_PATHS_AGP_UNASSIGNED 0x1u
int mxg_write_paths(mxg_handle *h, int assembly, const mxg_scaffold_node *nodes,
                    const uint64_t *path_first /* n_paths + 1 */, uint64_t n_paths,
                    const uint32_t *lead_strip, const uint32_t *tail_strip /* [n_paths]; NULL = all 0 */,
                    const char *first_line /* the FASTA's name, written as line 1 of path_file */,
                    const char *path_file, const char *agp_file /* may be NULL */, uint32_t flags);

/* ---- next row (f11): piece tables of scaffolding rounds, composed ----------------------------------------------
   ntJoin is run in rounds: the scaffold file of one run is the target of the next.  After round 2 the .path and the AGP name
   records of round 1 (`ntJoin7`, `ctgA:0-5000`), not the contigs the user began with; the reference leaves composing the AGPs of
   all rounds to the user.  A PIECE TABLE says what every record of a scaffold file is made of, in terms of the records of the file
   it was cut from: record r is the concatenation of pieces[first[r] .. first[r + 1]), a piece being
     MXG_PIECE_FWD  bases [start, end) of `record`
     MXG_PIECE_REV  the same, reversed and mapped through the table of bin/ntjoin_utils.py:145-150
     MXG_PIECE_GAP  end - start Ns; record and start are 0.
   A table is VALID when first starts at 0, every record has at least one piece, every piece has start < end and a known kind, and
   no record is longer than 2^32 - 1 bases.
   The composition of two tables: outer's `record` fields index inner's records; the result spells outer's records in terms of
   whatever inner refers to, so that a record spells the same sequence before and after.  Per outer piece, in order:
     FWD / REV over [a, b) of inner record r: the inner pieces of r that meet [a, b), the first and the last clipped to it; under
         REV in reverse order, FWD and REV swapped, gaps kept;
     GAP: itself.
   Then neighbouring GAP pieces of one record become one piece whose length is their sum (a round may cut inside a gap of the round
   before, and an AGP has no two gap lines in a row); sequence pieces are never joined.  The result is a valid table again.
   Computed on the device (count per outer piece, scan, emit, flag what survives the join, scan, compact).  *pieces and *first
   (n_outer + 1 entries) are host copies owned by the handle, valid until its next call of this entry.
   MXG_EINVAL: a null argument, a table that is not valid, an outer piece that names no inner record or is not inside it (end beyond
   the record's length); the message names the table, the record and the piece.  MXG_ELIMIT: 2^31 pieces or records or more in
   either table or in the result, a record longer than 2^32 - 1 bases.  n_outer == 0 is valid.  Sketches, graph and paths of the
   handle are left as they are. */
#define MXG_PIECE_FWD 0u
#define MXG_PIECE_REV 1u
#define MXG_PIECE_GAP 2u
typedef struct mxg_seq_piece {
    uint32_t record, start, end, kind;
} mxg_seq_piece;
int mxg_compose_pieces(mxg_handle *h, const mxg_seq_piece *outer, const uint64_t *outer_first /* n_outer + 1 */, uint64_t n_outer,
                       const mxg_seq_piece *inner, const uint64_t *inner_first /* n_inner + 1 */, uint64_t n_inner,
                       const mxg_seq_piece **pieces, const uint64_t **first /* n_outer + 1 */);
/* The records of the text mxg_write_scaffolds kept under MXG_SCAF_KEEP, in its order, in terms of the records of the assembly they were cut from, as a piece table
   (above): pieces rec_first[r] .. rec_first[r + 1] spell record r.  This is the table the text was written from,
   without its header literals and after the N strips were applied; a gap of 0 Ns has no piece.  A path gives FWD / REV pieces with
   GAP pieces between them, an unassigned interval one FWD piece.  The arrays are the handle's and hold as long as the text.
   mxg_scaffold_record_id: a kept record's name, ntJoin<p> or id:lo-hi (NULL: no such record, or nothing kept). */
int mxg_scaffold_pieces(mxg_handle *h, const mxg_seq_piece **pieces, const uint64_t **rec_first, uint64_t *n_records);
const char *mxg_scaffold_record_id(const mxg_handle *h, uint64_t record);

/* ---- next row (f12): synteny blocks of one assembly against another, and their PAF ------------------------------
   What the alignment half of the reference's `analysis` target is asked for (`minimap2 -x asm5 ... | samtools sort` on the target,
   the references and the scaffolds, ntJoin:158-161, 238-242): where a record lies on another assembly, in which orientation, and
   whether it is collinear with it -- alignment-free, from the graph: every vertex is a minimizer that occurs exactly once in every
   assembly, which is what a chaining aligner starts from.
   Inputs: a handle with a graph built on its own sketches; a query assembly q and a subject assembly s, q != s; the parameters;
   optionally a piece table over the records of q (mxg_seq_piece rows and first[n_records + 1], valid by the rule of
   mxg_compose_pieces: the table of mxg_scaffold_pieces makes the scaffolds the query); optionally query_length / subject_length,
   one entry per record of q / s, which replace the lengths the handle holds as record_length does in mxg_format_paths.
   ANCHORS.  Every graph vertex v is an anchor (qrec, qpos, srec, spos): its place in q and in s, from the graph.  Without a piece
   table the anchor list is the vertices ordered by (qrec, qpos): the order of q's sketch.  With one, the list is rebuilt record by
   record and piece by piece, in table order; off = the sum of the lengths of the earlier pieces of the piece's record, k = the
   handle's k:
     MXG_PIECE_FWD over [a, b) of record r takes the anchors with qrec == r, a <= qpos and qpos + k <= b, by rising qpos; the new
                   record is the table's record, the new qpos' = off + (qpos - a);
     MXG_PIECE_REV takes the same anchors by falling qpos, qpos' = off + (b - (qpos + k));
     MXG_PIECE_GAP takes none.
   An anchor in no piece vanishes, an anchor in two pieces appears twice; the length of a query record is the sum of its pieces.
   LINKS.  Anchors i and i + 1 of the list, d = sign(spos[i + 1] - spos[i]), are linked with direction d iff they lie on the same
   query record and the same subject record, d != 0 and, when max_gap > 0, qpos'[i + 1] - qpos'[i] <= max_gap and
   |spos[i + 1] - spos[i]| <= max_gap.
   BLOCKS.  A block is a maximal run of consecutive links of equal direction: links j .. j + r - 1 over anchors j .. j + r.  An
   anchor at which the direction turns belongs to both neighbouring blocks; an anchor without a link makes no block.  Per block:
     n_anchors = r + 1;  q_record;  q_start = qpos'[j], q_end = qpos'[j + r] + k;  s_record;
     s_start = min(spos[j], spos[j + r]), s_end = max(...) + k;  reverse = (d < 0).
   Kept are the blocks with n_anchors >= min_anchors and q_end - q_start >= min_span, in the order of their first anchor.
   The arrays of the view are host copies owned by the handle, valid until its next mxg_synteny_blocks; n_anchors_total = the length
   of the anchor list, n_links = its links (of either direction, before the filter).
   MXG_EINVAL: a null argument, no graph (or the graph of a distributed stage, whose vertex order is not the sketches'), q == s, an
   assembly out of range, struct_size too small, min_anchors < 2, a length array missing where the handle holds no lengths (an
   assembly loaded from a TSV, a side-car or minimizers), a table that is not valid or a piece outside its record (the message as
   mxg_compose_pieces words it, the table named "query").  MXG_ELIMIT: a query record longer than 2^32 - 1 bases, 2^31 anchors or
   blocks or more.  Zero vertices is valid and gives zero blocks.  Sketches, graph, paths and kept text stay as they are.
   mxg_write_synteny_paf: the blocks of the last mxg_synteny_blocks as PAF, formatted on the device, one line per block:
       qname qlen qstart qend strand tname tlen tstart tend matches blocklen 255 cm:i:<n_anchors>       (tab-separated)
   strand = '-' for a reverse block; matches = min(n_anchors * k, qend - qstart, tend - tstart), blocklen = max(qend - qstart,
   tend - tstart); cm:i is the tag minimap2 gives the number of minimizers on a chain.  tname = the handle's record ids of s;
   query_names = one name per query record (NULL: the handle's record ids of q; MXG_EINVAL when the query went through a piece
   table, whose records the handle has no names for -- those of mxg_scaffold_pieces' table are mxg_scaffold_record_id).  append != 0:
   the lines are added behind what `path` holds already (a file that a failed call was adding to is left as it is found).
   MXG_EINVAL: no such blocks.  MXG_SYN_WIN (test knob): bytes of PAF text per device window (at least 1, default and at most 64 Mi). */
typedef struct mxg_synteny_params {
    uint32_t struct_size; /* = sizeof(mxg_synteny_params) */
    uint32_t max_gap;     /* largest distance between linked anchors on either assembly; 0 = none */
    uint32_t min_anchors; /* >= 2 */
    uint32_t min_span;    /* smallest q_end - q_start */
} mxg_synteny_params;
typedef struct mxg_synteny_view {
    uint64_t n_blocks, n_anchors_total, n_links;
    const uint32_t *n_anchors, *q_record, *q_start, *q_end, *s_record, *s_start, *s_end; /* [n_blocks] */
    const uint8_t *reverse;                                                              /* [n_blocks] 0 = '+', 1 = '-' */
} mxg_synteny_view;
int mxg_synteny_blocks(mxg_handle *h, int q, int s, const mxg_synteny_params *params, const mxg_seq_piece *pieces /* may be NULL */,
                       const uint64_t *first /* n_records + 1 */, uint64_t n_records, const uint32_t *query_length /* NULL: the handle's own */,
                       const uint32_t *subject_length /* NULL: the handle's own */, mxg_synteny_view *out);
int mxg_write_synteny_paf(mxg_handle *h, const char *const *query_names, const char *path, int append);

/* ---- next row (f13): reference-based assessment of the kept blocks: chains, breakpoints, NGA50 --------------------
   What the reference's `analysis` target runs QUAST for (`quast -r ref --split-scaffolds --scaffold-gap-max-size 100000`,
   ntJoin:243-252): how much of the reference the query covers in how long collinear stretches, and where it breaks collinearity --
   from the kept blocks of the handle's last successful mxg_synteny_blocks: the blocks in their order, with the piece table, the
   query lengths and the subject lengths that call used (the handle keeps what it needs of these).  k = the handle's k.
   PIECE OF A BASE.  piece_of(r, x) = the index of the piece of query record r that holds base x: the piece with
   off <= x < off + len (off = the sum of the lengths of the record's earlier pieces).  GAP pieces count.  Without a piece table
   every record is one piece.
   JOINED.  Consecutive kept blocks i and i + 1 are joined iff all of these hold:
     they have the same q_record, the same s_record and the same reverse;
     gq = q_start[i+1] - q_end[i];  gs = s_start[i+1] - s_end[i] when forward, s_start[i] - s_end[i+1] when reverse (signed 64-bit):
         gq >= 1 - k and gs >= 1 - k (the next block's first anchor lies beyond this block's last anchor on both assemblies, in
         the block's direction);
     when merge_gap > 0: max(gq, gs) <= merge_gap;
     with at_join(i) = (piece_of(q_record, q_end[i] - 1) != piece_of(q_record, q_start[i+1])) and
         bound = at_join(i) ? join_indel : max_indel: when bound > 0, |gq - gs| <= bound.
   CHAINS.  A chain is a maximal run of joined consecutive kept blocks; chains are kept in order.  Per chain: n_blocks; first_block;
   n_anchors = the sum of its blocks' counts (joined blocks share no anchor); q_record; q_start of its first block, q_end of its
   last; s_record; s_start = min and s_end = max over its first and last block; reverse.  There is no chain filter (min_anchors /
   min_span of the blocks call filter what should not count).
   BREAKPOINTS.  Every pair of consecutive chains c, c + 1 with equal q_record is a breakpoint, of the first kind that applies:
   MXG_BP_TRANSLOCATION the subject records differ; MXG_BP_INVERSION reverse differs; MXG_BP_RELOCATION anything else.  Per
   breakpoint: chain = c; kind; at_join, taken from the last block of c and the first block of c + 1; q_lo = q_end[c];
   q_hi = q_start[c+1] (q_lo > q_hi where the two chains share a turning anchor).
   SUMMARY (exact 64-bit integers).  n_blocks, n_chains, n_breakpoints; breakpoints[kind][at_join]; query_bases and subject_bases =
   the sums of the record lengths; aligned_query = the sum of q_end - q_start over chains; chained_subject = the sum of
   s_end - s_start over chains; covered_subject = the sum over subject records of the size of the union of that record's chains'
   [s_start, s_end); three Nx blocks {n50, l50, n75, l75, n90, l90}:
       na   the chains' query spans,     D = query_bases
       nga  the chains' query spans,     D = subject_bases
       ng   the query record lengths,    D = subject_bases
   With the multiset sorted descending and S_j the sum of its first j: Lx = the smallest j with 100 S_j >= x D, Nx = the j-th
   length; both 0 when no j reaches it or D == 0.
   Computed on the device (assess.hip): the blocks are uploaded from the host copy the blocks view holds, so the result spells that
   view.  The view's arrays are host copies owned by the handle until its next mxg_synteny_assess.
   MXG_EINVAL: a null argument, struct_size too small, no successful mxg_synteny_blocks before.  MXG_ELIMIT: as in the blocks call
   (2^31 blocks or more; the blocks call refuses them first).  Zero blocks is valid: zero chains, zero breakpoints, zero sums, and
   ng still computed.  Sketches, graph, paths, kept text and the blocks stay as they are: mxg_write_synteny_paf still works. */
#define MXG_BP_TRANSLOCATION 0u
#define MXG_BP_INVERSION 1u
#define MXG_BP_RELOCATION 2u
typedef struct mxg_assess_params {
    uint32_t struct_size; /* = sizeof(mxg_assess_params) */
    uint32_t merge_gap;   /* largest gap between joined blocks, on either assembly; 0 = no bound.  Default 100000 */
    uint32_t max_indel;   /* largest |gq - gs| between joined blocks inside one piece; 0 = no bound.  Default 1000 */
    uint32_t join_indel;  /* the same where the two blocks lie in different pieces; 0 = no bound.  Default 100000 */
} mxg_assess_params;
typedef struct mxg_nx {
    uint64_t n50, l50, n75, l75, n90, l90;
} mxg_nx;
typedef struct mxg_assess_view {
    uint64_t n_blocks, n_chains, n_breakpoints;
    uint64_t breakpoints[3][2]; /* [kind][at_join] */
    uint64_t query_bases, subject_bases, aligned_query, chained_subject, covered_subject;
    mxg_nx na, nga, ng;
    const uint32_t *chain_n_blocks, *chain_first_block, *chain_n_anchors, *chain_q_record, *chain_q_start, *chain_q_end, *chain_s_record,
        *chain_s_start, *chain_s_end, *chain_reverse;                      /* [n_chains] */
    const uint32_t *bp_chain, *bp_kind, *bp_at_join, *bp_q_lo, *bp_q_hi; /* [n_breakpoints] */
} mxg_assess_view;
int mxg_synteny_assess(mxg_handle *h, const mxg_assess_params *params, mxg_assess_view *out);

/* ---- next row (f14): base-level identity of stretches whose ends are pinned -------------------------------------
   How far apart two stretches of bases are, where the caller -- the graph's anchors, say -- already knows where both begin and end:
   a narrow-band edit distance per SEGMENT, nothing is searched for, no alignment is kept.
   BASES.  The bases of a record are the bytes of its sequence text that are no line breaks ('\n', '\r').  A base's class is 0..3 for
   A C G T/U in either case and 4 for anything else; the complement of class c < 4 is 3 - c.
   A SEGMENT is lq >= 1 bases of record q_record of the query text from base q_start, and ls >= 1 bases of record s_record of the
   subject text from base s_start.  Q = the classes of the query interval; S = the classes of the subject interval, read backwards
   and complemented when reverse != 0.  d = ls - lq.
   STATUS, the first rule that applies:
     MXG_IDY_SKIP_LEN    lq > max_seg or ls > max_seg
     MXG_IDY_SKIP_SHIFT  |d| > MXG_IDY_MAX_SHIFT
     MXG_IDY_SKIP_N      a base of Q or S has class 4 (a base outside the interval does not count)
     MXG_IDY_ALIGNED     edits = D[lq][ls] of the unit-cost DP over the cells (i, j), 0 <= i <= lq, 0 <= j <= ls, whose diagonal
                         j - i lies in [min(0, d) - MXG_IDY_E, max(0, d) + MXG_IDY_E] (at most 64 diagonals):  D[0][0] = 0,
                         D[i][j] = min(D[i-1][j-1] + (Q[i] != S[j]), D[i-1][j] + 1, D[i][j-1] + 1) over the neighbours inside the
                         band.  The status word also carries MXG_IDY_SATURATED iff edits > |d| + 2 MXG_IDY_E; without that flag
                         edits is the unbanded edit distance (a path that cheap cannot leave the band), with it an upper bound.
   out_status[i] = the status, with the flag; out_edits[i] = edits, 0 for a skipped segment.
   TEXTS.  q_text and s_text name texts the handle holds on the device: an assembly index, whose records are the file's (folded
   lines, "\r\n" and records across many tiles are all walked), or MXG_TEXT_SCAFFOLDS, the text the last mxg_write_scaffolds kept
   under MXG_SCAF_KEEP, whose records are those of mxg_scaffold_pieces.  q_text == s_text is allowed.
   Computed on the device (identity.hip): one lane per segment, the band in one 64-bit word per lane (identity.h), the bases read
   from the resident text in aligned words.  segs, out_edits and out_status are host arrays of n entries.
   MXG_EINVAL: a null argument with n > 0, max_seg == 0, no such assembly, an assembly whose text the handle does not hold on the
   device (the conditions of mxg_write_fai), MXG_TEXT_SCAFFOLDS with nothing kept, a record out of range, lq == 0 or ls == 0, an
   interval that ends beyond its record; the message names the segment.  MXG_ELIMIT: 2^31 segments or more.  n == 0 is valid.
   Nothing of the handle changes; it stays usable after every refusal. */
#define MXG_IDY_E 16u
#define MXG_IDY_MAX_SHIFT 31u
#define MXG_IDY_ALIGNED 0u
#define MXG_IDY_SKIP_LEN 1u
#define MXG_IDY_SKIP_SHIFT 2u
#define MXG_IDY_SKIP_N 3u
#define MXG_IDY_STATUS_MASK 0xFFu
#define MXG_IDY_SATURATED 0x100u
#define MXG_IDY_DEFAULT_MAX_SEG 10000u
#define MXG_TEXT_SCAFFOLDS (-1)
typedef struct mxg_identity_seg {
    uint32_t q_record, q_start, lq;
    uint32_t s_record, s_start, ls;
    uint32_t reverse, pad; /* pad: 0 */
} mxg_identity_seg;
int mxg_identity_segments(mxg_handle *h, int q_text, int s_text, const mxg_identity_seg *segs, uint64_t n, uint32_t max_seg,
                          uint32_t *out_edits, uint32_t *out_status);
/* mxg_synteny_identity: the segments between the anchors of the kept blocks of the handle's last successful mxg_synteny_blocks.
   SEGMENTS OF A BLOCK over anchors j .. j + r of the anchor list (qpos' = the query positions of that list, through the piece table
   when there was one; k = the handle's k):
     link i -> i + 1:  query bases [qpos'[i], qpos'[i+1]); subject bases [spos[i], spos[i+1]) in a forward block,
                       [spos[i+1] + k, spos[i] + k) with reverse = 1 in a reverse block;
     the last anchor:  query bases [qpos'[j+r], + k), subject bases [spos[j+r], + k), reverse as the block's.
   A block has n_anchors segments, and its aligned segments cover q_end - q_start query bases when none is skipped.
   PER BLOCK (the view's arrays, in the order of the kept blocks): n_aligned, n_skip_len, n_skip_shift, n_skip_n = its segments by
   status; n_saturated = its aligned segments that carry the flag; aligned_q, aligned_s = the sums of lq and of ls over its aligned
   segments; edits = the sum over its aligned segments, the flagged ones included (they are upper bounds).
   SUMMARY: the same fields summed over all kept blocks, n_segments, and block_q = the sum of q_end - q_start.
   The query text is assembly q of the blocks call, or, when that call went through a piece table, the text mxg_write_scaffolds
   kept under MXG_SCAF_KEEP: the table must then be the one of mxg_scaffold_pieces of that text (same assembly, same number of
   records, same lengths).  The subject text is assembly s.  Either assembly's record lengths must be the ones the blocks call used.
   Computed on the device (identity.hip): the anchors and the blocks' first anchors are read where the blocks call left them; one
   thread per anchor of a kept block, placed by a scan over n_anchors, writes its segment; the segment kernel of
   mxg_identity_segments; six 64-bit prefix scans over the segments, the blocks' sums as differences at their borders.  A run that
   never calls this allocates and launches nothing for it.  The view's arrays are host copies owned by the handle until its next
   mxg_synteny_identity or mxg_synteny_blocks.
   MXG_EINVAL: a null argument, struct_size too small, max_seg == 0, flags != 0, no successful mxg_synteny_blocks before, a text
   that is not held on the device (as mxg_identity_segments), a piece table that is not the kept text's, record lengths that differ
   from the text's.  MXG_ELIMIT: 2^31 segments or more.  Zero blocks is valid.  Sketches, graph, paths, kept text, blocks and the
   assessment stay as they are: mxg_synteny_blocks' view, mxg_write_synteny_paf and mxg_synteny_assess work as before. */
typedef struct mxg_identity_params {
    uint32_t struct_size; /* = sizeof(mxg_identity_params) */
    uint32_t max_seg;     /* segments longer than this on either side are counted, not aligned; default MXG_IDY_DEFAULT_MAX_SEG */
    uint32_t flags;       /* 0 */
    uint32_t reserved;    /* 0 */
} mxg_identity_params;
typedef struct mxg_identity_view {
    uint64_t n_blocks, n_segments, n_aligned, n_skip_len, n_skip_shift, n_skip_n, n_saturated, block_q, aligned_q, aligned_s, edits;
    const uint64_t *blk_n_aligned, *blk_n_skip_len, *blk_n_skip_shift, *blk_n_skip_n, *blk_n_saturated, *blk_aligned_q, *blk_aligned_s,
        *blk_edits; /* [n_blocks] */
} mxg_identity_view;
int mxg_synteny_identity(mxg_handle *h, const mxg_identity_params *params, mxg_identity_view *out);
/* mxg_write_synteny_paf_ex: mxg_write_synteny_paf with flags.  flags == 0: byte for byte that call.  MXG_PAF_IDENTITY: every line
   gets "\tal:i:<aligned_q>" appended and, when aligned_q > 0, "\tNM:i:<edits>\tdv:f:0.dddd" with
   dddd = floor(10000 edits / max(aligned_q, aligned_s)) in four digits ("1.0000" when the ratio reaches 1), the block's values of
   the last mxg_synteny_identity, computed in integers on the device; columns 1 to 13 do not change.  MXG_EINVAL also: an unknown
   flag; MXG_PAF_IDENTITY without a successful mxg_synteny_identity since the last mxg_synteny_blocks. */
#define MXG_PAF_IDENTITY 0x1u
int mxg_write_synteny_paf_ex(mxg_handle *h, const char *const *query_names, const char *path, int append, uint32_t flags);

/* ---- next row (f15): features of the source records lifted onto the records a piece table spells ---------------
   A user's gene models, repeat tracks and variant sites lie on the contigs they began with; the scaffold file's records are
   `ntJoin7` and `ctgA:0-5000`, cut, reverse-complemented, trimmed and, over several rounds, renamed twice.  The reference leaves an
   AGP and the liftover to the user.  The piece table (row f11; mxg_scaffold_pieces, mxg_compose_pieces) is the answer read the
   other way round: from the SOURCE records -- those the table's FWD / REV pieces name -- to the records it spells.
   A FEATURE is (record r, start a, end b), 0-based and half-open, over the source records.  Its PARTS come from the sequence
   pieces p of the table with p.record == r, p.start < b and p.end > a, ordered by (p.start, index of p in the table).  A GAP piece
   never matches; a base in two pieces is lifted twice; a base in no piece (a trimmed overlap, stripped Ns, a dropped interval) is
   lost.  For each such piece, with lo = max(a, p.start), hi = min(b, p.end), R the table record of p and off the bases of R in
   front of p, the part is (R, s_start, s_end, src_start = lo, reverse):
     FWD  [off + lo - p.start, off + hi - p.start), reverse = 0        REV  [off + p.end - hi, off + p.end - lo), reverse = 1
   With lifted = the sum of hi - lo over the parts, the feature's STATUS is the first that holds of
     MXG_LIFT_INVALID  r >= n_source, a >= b or b > source_length[r]     MXG_LIFT_UNKNOWN  (BED only) the name is no source record
     MXG_LIFT_LOST     no part                                           MXG_LIFT_WHOLE    one part and lifted == b - a
     MXG_LIFT_PARTIAL  lifted < b - a                                    MXG_LIFT_SPLIT    anything else
   INVALID and UNKNOWN give no parts.  Parts are never joined (composition never joins sequence pieces either).

   mxg_lift_prepare checks the table as mxg_compose_pieces does (valid; every sequence piece inside the source record it names,
   source_length[n_source] giving their lengths; the same messages, the table named "table") and builds the table's index on the
   device: the sequence pieces compacted, sorted by (record << 32) | start with a stable radix sort over exactly the key bits
   n_source needs, and the running maximum of (record << 32) | end over that order.  The handle keeps the index until the next
   mxg_lift_prepare (a failed one leaves none) or mxg_destroy; sketches, graph, paths and kept text stay as they are.
   n_records == 0 is valid.  MXG_ELIMIT: as mxg_compose_pieces, and 2^31 source records or more.

   mxg_lift_intervals lifts n features, one thread each: two bisections bound the candidate pieces, those that end behind a are
   counted, the counts' 64-bit sum is taken before anything is scanned in 32 bits (2^31 parts or more: MXG_ELIMIT, nothing is
   emitted), then the parts are emitted.  The view's arrays are host copies owned by the handle, valid until its next lift call:
   feature i's parts are part_first[i] .. part_first[i + 1].  MXG_LIFT_WHOLE_ONLY: a feature that is not WHOLE keeps its status
   and gives no parts.  MXG_EINVAL: no prepared index, a null argument, an unknown flag.  n == 0 is valid.

   mxg_lift_bed lifts the features of a BED file.  Lines end in '\n' (a '\r' in front of it is dropped; the last line may lack
   its '\n'); empty lines and lines that begin with '#', "track" or "browser" are skipped.  Fields are separated by tabs; fewer
   than three, or a column 2 or 3 that is not 1 to 10 decimal digits of a value <= 2^32 - 1, make the feature INVALID.  Column 1
   is matched exactly against source_names[n_source] (the first record of a name wins; no match: UNKNOWN).  lifted_path gets one
   line per part, in input order, then part order:
       scaffold_names[R] \t s_start \t s_end [\t the input line from column 4 on, byte for byte] \n
   but that a column 6 that is exactly "+" or "-" is flipped on a reverse part.  The text is formatted on the device and leaves
   window by window.  unlifted_path (may be NULL) gets, for every feature that is not WHOLE, in input order, a line "#<reason>" and
   the original line: "Split in new", "Partially deleted in new", "Deleted in new" (UCSC liftOver's wording), "Invalid", "Unknown
   record".  The file is worked through in batches of whole lines of at most MXG_LIFT_BATCH bytes (a longer line is a batch of
   its own); neither file depends on the batch size or on the window size MXG_LIFT_WIN.  A failing call removes the files it
   created.  MXG_EIO: a file that cannot be read or written. */
#define MXG_LIFT_WHOLE 0u
#define MXG_LIFT_SPLIT 1u
#define MXG_LIFT_PARTIAL 2u
#define MXG_LIFT_LOST 3u
#define MXG_LIFT_INVALID 4u
#define MXG_LIFT_UNKNOWN 5u
#define MXG_LIFT_WHOLE_ONLY 0x1u
typedef struct mxg_lift_view {
    uint64_t n_features, n_parts;
    const uint64_t *part_first; /* n_features + 1 */
    const uint8_t *status;      /* n_features */
    const uint32_t *s_record, *s_start, *s_end, *src_start; /* n_parts */
    const uint8_t *reverse;                                 /* n_parts */
} mxg_lift_view;
typedef struct mxg_lift_stats {
    uint64_t lines, skipped, features;
    uint64_t status[6]; /* features per MXG_LIFT_* */
    uint64_t parts, lifted_bytes, unlifted_bytes;
} mxg_lift_stats;
int mxg_lift_prepare(mxg_handle *h, const mxg_seq_piece *pieces, const uint64_t *first /* n_records + 1 */, uint64_t n_records,
                     const uint32_t *source_length /* n_source */, uint64_t n_source);
int mxg_lift_intervals(mxg_handle *h, const uint32_t *record, const uint32_t *start, const uint32_t *end, uint64_t n, uint32_t flags,
                       mxg_lift_view *out);
int mxg_lift_bed(mxg_handle *h, const char *bed_path, const char *const *source_names /* n_source */,
                 const char *const *scaffold_names /* n_records */, const char *lifted_path, const char *unlifted_path /* may be NULL */,
                 uint32_t flags, mxg_lift_stats *stats /* may be NULL */);

/* ---- graph stage distributed over ranks by hash range (one process per GPU) --------------------------
   No counterpart in the reference (it is one process).  Uniqueness and intersection need every occurrence of a hash in
   one place: every minimizer travels to the rank that owns its hash, the owner runs the ordinary graph kernels on what it
   received and numbers its vertices, the verdict travels back, and adjacency (which stays with the records) reaches the
   owners of both end points as messages.  These entry points pack, unpack and count on the device; the all-to-all
   exchanges between them are the caller's (ntjoin_amd/dist.py: torch.distributed, backend "nccl" = RCCL).
   Sender side (the handle that holds the sketches):
     mxg_dg_owner_counts  counts[a * world + r] = minimizers of assembly a owned by rank r
     mxg_dg_pack_items    assembly a's minimizers as 16-byte items {hash, pos, record + rec_offset}, bucket r starting at
                          item starts[r] of d_send
     mxg_dg_msg_counts    after the verdicts came back (d_ret: 8 bytes per item, same layout as d_send): flags of every
                          assembly, and counts[a * world + r] = adjacency messages of assembly a for rank r; d_bases =
                          device array u32[world + 1], first global vertex id of every rank
     mxg_dg_pack_msgs     those messages (16 bytes each), bucket r starting at message starts[r] of d_send
   Owner side (a second handle with the same assemblies registered, no sketches):
     mxg_dg_set_items     assembly a's received items: source s's section starts at item sec_start[s] of d_items and holds
                          sec_count[s] items
     mxg_dg_vertices      uniqueness, intersection, local vertex ids; the owner's vertex count is written to the DEVICE
                          word d_n_vertices (u64) -- no host sync
     mxg_dg_item_results  the verdict of every item (flags | global vertex id << 8, or 2^32-1 << 8) written to d_out at the
                          item's place in the receive layout; d_gbase = device u32 holding this owner's first global id
     mxg_dg_edges         adjacency from the received messages, then the edges whose first supporter's source vertex is
                          local (the stage's sync); afterwards mxg_get_graph gives this owner's vertices and edges
                          (edge_u: local vertex index, edge_v: global vertex id) */
int mxg_dg_owner_counts(mxg_handle *h, uint32_t world, uint64_t *counts);
int mxg_dg_pack_items(mxg_handle *h, int assembly, uint32_t world, uint32_t rec_offset, const uint64_t *starts, void *d_send);
int mxg_dg_set_items(mxg_handle *h, int assembly, const void *d_items, uint32_t world, const uint64_t *sec_start,
                     const uint64_t *sec_count);
int mxg_dg_vertices(mxg_handle *h, void *d_n_vertices);
int mxg_dg_item_results(mxg_handle *h, int assembly, const void *d_gbase, uint32_t world, const uint64_t *sec_start,
                        const uint64_t *sec_count, void *d_out);
int mxg_dg_msg_counts(mxg_handle *h, uint32_t world, const void *d_ret, const void *d_bases, uint64_t *counts);
int mxg_dg_pack_msgs(mxg_handle *h, int assembly, uint32_t world, const void *d_bases, const uint64_t *starts, void *d_send);
/* Records cut between ranks (mxg_add_assembly_fasta_split / ..._packed_device_pieces): the adjacency between the last shared
   minimizer of one rank's piece and the first shared minimizer of the next rank's piece lies with neither rank.  After the
   verdicts came back, mxg_dg_last_shared writes {record, global vertex id} of this rank's LAST shared minimizer of every
   assembly (2^32-1: none) to d_out (device u32[A][2]); the caller all-gathers these (u32[world][A][2]) and hands them to
   mxg_dg_set_ghosts, after which mxg_dg_msg_counts / mxg_dg_pack_msgs / mxg_dg_pack_msg_slots also emit the pair (nearest
   shared minimizer of that record on an earlier rank, this rank's first).  d_all = NULL switches it off.  No host sync. */
int mxg_dg_last_shared(mxg_handle *h, const void *d_ret, void *d_out);
int mxg_dg_set_ghosts(mxg_handle *h, const void *d_all, uint32_t world, uint32_t rank);
int mxg_dg_edges(mxg_handle *h, const void *d_msgs, uint64_t n_msgs, uint64_t *n_vertices, uint64_t *n_edges);
/* Steady state of the same exchange with FIXED-CAPACITY SLOTS: once one exact step has shown the sizes, every (source,
   destination, assembly) triple gets a slot = 64-byte header (word 0 = the count) + cap[a] 16-byte items (<= 8 assemblies);
   the all-to-alls then have equal splits and the receivers read the counts on the device: no size exchange, no host sync
   before mxg_dg_edges_slots.  A count above its capacity sets *overflow there: repeat the step the exact way.  The item
   buffer is ASSEMBLY-MAJOR: assembly a's `world` slots lie side by side at byte offset sum over a' < a of
   world * (64 + 16 cap[a']), so that one all-to-all per assembly carries them (the verdict buffers stay [world][sum cap]).
   Message slots: 64-byte header (word 0 = count) + max_msgs 16-byte messages.  mxg_dg_pack_slots clears its assembly's
   headers, mxg_dg_pack_msg_slots all of them at its start.
   mxg_sketch_dg_pack_slots = mxg_sketch(h, MXG_SKETCH_ALL) + mxg_dg_pack_slots for every assembly WITHOUT the host sync in
   between: the sketches are enqueued, every assembly's items are packed right behind its own last kernel with the count
   read on the device (rec_offsets[a] = that assembly's record index shift), and mxg_part_packed_wait(h, a, stream) lets the
   caller's communication stream send assembly a's slots while the next assembly is still being sketched.  A sketch that did
   not end the common way reaches every destination as a count far above any capacity (overflow: all ranks repeat the step the
   exact way).  After the caller's sync on the handle's stream: mxg_sketch_finish.  No counterpart in the reference. */
int mxg_sketch_dg_pack_slots(mxg_handle *h, uint32_t world, uint32_t n_asm, const uint32_t *cap, const uint32_t *rec_offsets,
                             void *d_send);
int mxg_dg_pack_slots(mxg_handle *h, int assembly, uint32_t rec_offset, uint32_t world, uint32_t n_asm, const uint32_t *cap,
                      void *d_send);
int mxg_dg_owner_slots(mxg_handle *h, uint32_t world, uint32_t n_asm, const uint32_t *cap, const void *d_recv, void *d_n_vertices);
int mxg_dg_slot_results(mxg_handle *h, uint32_t world, uint32_t n_asm, const uint32_t *cap, const void *d_recv,
                        const void *d_gbase, void *d_out /* [world][sum cap] u64 */);
int mxg_dg_pack_msg_slots(mxg_handle *h, uint32_t world, uint32_t max_msgs, const void *d_ret, const void *d_bases, void *d_send);
int mxg_dg_edges_slots(mxg_handle *h, const void *d_recv, uint32_t world, uint32_t max_msgs, uint64_t *n_vertices,
                       uint64_t *n_edges, uint32_t *overflow);

/* ---- text helpers used by the writers (host only; usable without a device) --------------------- */
/* python repr() of a float / of a str, as Ntjoin.print_graph's f-strings produce them.  Returns the length
   written (excluding the NUL), or the length needed if it exceeds cap. */
size_t mxg_py_repr_double(double v, char *buf, size_t cap);
size_t mxg_py_repr_str(const char *s, char *buf, size_t cap);


/* ---- synthetic inputs (bench / test support; no counterpart in the reference, whose tests hold four small FASTA files)
   SURVEY.md 8(d) configs 2-5: assemblies of 0.1-20 Gbp "generated on device from a counter-based RNG mirrored on the
   CPU".  The genome is a pure function of (seed, coordinate): 32 bases per splitmix64 output; an assembly is a list of
   segments, output bases [dst_base, dst_base+len) = genome coordinates src..src+len-1, reverse-complemented when rc,
   each base substituted with probability sub_per_65536/65536 (decided by a second splitmix64 stream indexed by the
   coordinate).  Segments must be sorted by dst_base (multiples of 16, non-overlapping); words outside are zero.
   Formulas: ntjoin_amd/csrc/synth.hip, mirrored in numpy by ntjoin_amd/synth.py. */
typedef struct mxg_synth_seg {
    uint64_t dst_base; /* first output base (multiple of 16)          */
    uint64_t src;      /* genome coordinate of the segment's first base (its LAST output base when rc) */
    uint64_t len;      /* bases                                       */
    uint32_t rc;       /* 1: output is the reverse complement         */
    uint32_t reserved;
} mxg_synth_seg;
/* fills d_out[0..n_words) (HBM, 2-bit packed as mxg_add_assembly_packed_device expects); device < 0 = current device */
int mxg_synth_fill_packed_device(void *d_out, uint64_t n_words, const mxg_synth_seg *segs, uint64_t n_segs, uint64_t seed,
                                 uint64_t sub_seed, uint32_t sub_per_65536, int device);
/* the same words computed on the host (n_threads workers); usable without a device */
int mxg_synth_fill_packed_host(uint32_t *out, uint64_t n_words, const mxg_synth_seg *segs, uint64_t n_segs, uint64_t seed,
                               uint64_t sub_seed, uint32_t sub_per_65536, uint32_t n_threads);
/* FASTA text of packed host records (ids "<id_prefix><r>", `line` bases per line): materialises a synthetic assembly
   as a file for the end-to-end (FASTA -> .tsv + .mx.dot) measurement.  Host only. */
int mxg_synth_write_fasta(const char *path, const uint32_t *packed, const uint64_t *rec_start, const uint64_t *rec_len,
                          uint64_t n_records, const char *id_prefix, uint32_t line, uint32_t n_threads);

/* ---- introspection ----------------------------------------------------------------------------- */
int mxg_get_stats(mxg_handle *h, mxg_stats *out);
int mxg_reset_timers(mxg_handle *h);
/* The environment knobs (README: MXG_* tuning / test / profiling switches) this handle has read and found SET, as
   "NAME=value NAME=value ..." sorted by name.  A knob is parsed once per handle, at its first use, so this is what the
   handle really ran with.  Returns the text's length; writes at most cap - 1 bytes + NUL (buf may be NULL).  No reference
   counterpart (bench.py records it next to every number). */
size_t mxg_knobs(mxg_handle *h, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* NTJOIN_MX_H */
