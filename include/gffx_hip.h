/*
 * gffx_hip.h -- C ABI of the MI355X (gfx950) engine for the `gffx intersect` hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  It is what a
 * Rust `gffx-hip` FFI crate would bind with `extern "C"` (binding shown in INTEGRATION.md).
 * Reference anchors are Baohua-Chen/GFFx v0.4.0, paths relative to its src/.
 *
 *   reference item (file:line)                          entry point here
 *   --------------------------------------------------  ---------------------------------------
 *   TreeIndexData / IntervalTree<u32> per seqid         gffx_hip_index_create / _destroy
 *     (utils/tree_index.rs:12-16, utils/tree.rs:5-23)     (device-resident sorted SoA + AoS)
 *   IntervalTree::query_interval (utils/tree.rs:98-121) \
 *   query_features + OverlapMode predicates + invert     > gffx_hip_batch_run / _wait and the
 *     (commands/intersect.rs:105-169, :73-78, :145-161) /   one-shot gffx_hip_query_features
 *   unique-root collection (commands/intersect.rs:598-615)  GFFX_OUT_ROOT_BITMAP
 *   gff_line_overlaps_queries, numeric part             gffx_hip_lines_* (Join B)
 *     (commands/intersect.rs:500-521)
 *   compute_hit_depth / compute_root_depth              gffx_hip_depth_* (`gffx depth`, BED source)
 *     (commands/depth.rs:121-293)
 *   merge_intervals + the two-pointer walk              gffx_hip_segments_covered, gffx_hip_union_* (`gffx coverage`)
 *     (commands/coverage.rs:92-124, :339-364)
 *   (no reference item: the reference reports no per-base depth)  gffx_hip_pileup_* (`gffx coverage --mean-depth`)
 *   (no reference item)                                           gffx_hip_pileup_meta_* (`gffx meta`)
 *   (no reference item)                                           gffx_hip_profile_* (`gffx coverage --thresholds / --bedgraph`)
 *   (no reference item)                                           gffx_hip_closest_* (`gffx closest`)
 *   bam::Reader records -> (chr, start, end) rows        gffx_hip_bgzf_inflate, gffx_hip_bam_* (BAM sources)
 *     (commands/depth.rs:297-372, coverage.rs:125-168)
 *   the same reader on a .sam file                       gffx_hip_sam_* (SAM sources, plain or BGZF-compressed)
 *   BED text, plain or BGZF-compressed, to rows          gffx_hip_bed_* (BED sources, the two dialects of the commands)
 *     (commands/depth.rs:588-591, coverage.rs:520-541)
 *   FtsMap::map_fnames_to_fids, PrtMap::map_fids_to_roots, gffx_hip_ids_* (`gffx extract`)
 *   the ID test of write_gff_output_filtered
 *     (index_loader/fts.rs:16-93, prt.rs:54-102, utils/common.rs:389-431)
 *   the line loop, feature_map and the numbering loop of   gffx_hip_gff_* (`gffx index --gpu`)
 *     build_index (index_builder/core.rs:71-203)
 *   (no reference item: the reference writes no sequences)   gffx_hip_genome_*, gffx_hip_seq_* (`gffx seq`)
 *   (no reference item: the reference reads no variants)     gffx_hip_effect_* (`gffx effect`)
 *
 * Semantics (bit-exact with the reference):
 *   a root interval iv of the query's seqid is a HIT iff  iv.start < q.end && iv.end > q.start
 *   (strict, half-open; u32 compares; q.start >= q.end rows are legal and evaluated as-is);
 *   keep = mode predicate(iv, q);  a (query, root) pair is emitted iff  invert ^ keep.
 * Output order: the pairs of one query are contiguous (its segment); WHERE the segments lie and the order inside a segment
 * depend on the strategy, and only the multiset of pairs per query is the contract (the reference's own order is that of an
 * FxHashMap walk plus a tree DFS and is unspecified as well):
 *   DIRECT                 segments in INPUT order (CSR: offsets = exclusive prefix of the counts); inside a segment
 *                          descending position in the seqid's start-sorted list (ties in start: later builder order first)
 *   WINDOWS / FUSED        segments in the order in which rounds (2048 or 4096 regions) reserve them (differs from run to run);
 *                          inside a round the runs of its groups of 256 regions in the order the waves arrive, the regions
 *                          of a group in input order; every query's segment start is given explicitly (GFFX_OUT_OFFSETS /
 *                          GFFX_OUT_OFFSETS32) or per group (GFFX_OUT_SEGBASE) and the segments tile [0, pairs) exactly.  Inside a segment:
 *                          WINDOWS ascending list order (start, ties in builder order) for regions answered from the
 *                          window's candidate list (the wide form: the inline entries of the line of the region's first
 *                          base, then the run of roots that start inside the region, then the entries of that line's
 *                          list that continue in the spill records -- these start at or before the region, so a wide-form
 *                          segment is NOT ascending by start), descending for regions that took the exact sweep; FUSED descending
 *   SORTED (partitioned)   segments in the order genome tiles were served, offsets explicit, inside a segment descending
 *
 * Threading: an index is immutable after creation and may be shared by threads; a batch owns
 * one HIP stream plus its buffers and must not be used from two threads at once.
 * Errors: every function returns GFFX_OK (0) or a negative gffx_status; the message of the
 * last failure on the calling thread is in gffx_hip_last_error().  Nothing throws or aborts
 * across this boundary.  There is NO CPU fallback: without a HIP device every compute entry
 * point fails with GFFX_E_NO_DEVICE.
 *
 * Tuning knobs (results never depend on any of them).  Each is an environment variable that is read ONCE per object -- the
 * index builders' when gffx_hip_index_create runs (a clone inherits them), the passes' when gffx_hip_batch_create runs -- and a
 * batch's can be changed afterwards with gffx_hip_batch_set_option(batch, "WIN_THREADS", 512).  No launch reads the environment.
 * gffx_hip_index_options / gffx_hip_batch_options report the values that differ from the defaults as a JSON object
 * (`gffx ... --stats-json` and bench.py's `config.knobs` carry it).
 *   passes (batch):
 *   GFFX_HIP_WIN_THREADS=0|512|1024 block width of the window kernels (0 = the engine's choice: 1024 for a pass of >= 500 000 regions
 *                                   that runs alone, 512 otherwise).  Batches sorted by position handed over in groups on ONE stream
 *                                   (GFFX_HIP_GROUP=1) are 25 % faster at 1024: their gene-dense wave rounds overflow the 512-thread
 *                                   kernel's smaller strips (on two streams: 1.5 %; profiles/r06_block_width_on_sorted_batches.txt)
 *   GFFX_HIP_WIN_WIDE=0|1|2         the mixed form of the window kernels: never / AUTO's choice for batches with wide rows (default) /
 *                                   every eligible pass of the windows strategy
 *   GFFX_HIP_WIDTH_SAMPLE=0         no width sample of the rows the host hands over (AUTO then learns from a first waited pass)
 *   GFFX_HIP_GROUP=0|1|2|3          gffx_hip_batches_run_n with four batches or more: one launch per GROUP of batches, the groups on 1 / 2
 *                                   (default) / 3 streams of the index; 0: always pass by pass; 1 also groups two or three batches
 *   GFFX_HIP_TICKETS=0..4           how a launch's blocks get their rounds: 0 a fixed stride, 1 the launch's tail by ticket, 2 every round by
 *                                   ticket, 3 only the rounds beyond the last full stride, 4 (default) the engine's choice (1 for a launch that
 *                                   serves one batch with eight or more rounds per block, else 0)
 *   GFFX_HIP_WIN_FILTER=0|1|2       coverage filter of the window kernels: the engine's choice (default: the fine level of the index where it
 *                                   fits the launch's LDS and the blocks run four rounds or more, else the coarse one) / the coarse level
 *                                   only / the fine level wherever it fits
 *   GFFX_HIP_AUTO_STRATEGY=n        what GFFX_STRATEGY_AUTO resolves to (0: the engine's choice)
 *   launch sizes (0 = the engine's choice): GFFX_HIP_FUSED_BLOCKS, GFFX_HIP_BITMAP_BLOCKS; GFFX_HIP_JOIN_BLOCKS, GFFX_HIP_MAX_BLOCKS;
 *   GFFX_HIP_PARTITION_BUDGET_MB (record buffers of the partitioned strategy)
 *   index build: GFFX_HIP_SLOT_WMAX (widest region a window line answers, 16384), GFFX_HIP_WIN_PER_ENTRY, GFFX_HIP_WIN_SPLIT,
 *   GFFX_HIP_WIN_FILTER_KB (coarse coverage filter, 24), GFFX_HIP_WIN_FILTER_FINE_KB (the fine one: at most this, and at most the LDS a
 *   1024-thread pair pass has left; 0 = none), GFFX_HIP_WIN_MAX_LINES, GFFX_HIP_BINS_PER_ENTRY
 */
#ifndef GFFX_HIP_H
#define GFFX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFFX_HIP_ABI_VERSION 1

/* commands/intersect.rs:73-78 OverlapMode */
enum gffx_mode { GFFX_MODE_CONTAINED = 0, GFFX_MODE_CONTAINS_REGION = 1, GFFX_MODE_OVERLAP = 2 };

enum gffx_status {
    GFFX_OK = 0,
    GFFX_E_INVALID = -1,   /* bad argument */
    GFFX_E_NO_DEVICE = -2, /* no HIP device / device index out of range */
    GFFX_E_HIP = -3,       /* a HIP runtime call failed */
    GFFX_E_OOM = -4,       /* host or device allocation failed */
    GFFX_E_CHR_RANGE = -5, /* a query's chr >= n_chr (the reference panics: intersect.rs:117) */
    GFFX_E_STATE = -6      /* call order violated (e.g. results read before _wait) */
};

/* what a batch run materialises on the device */
enum gffx_out {
    GFFX_OUT_COUNTS = 1,      /* u32 kept pairs per query, input order (always produced) */
    GFFX_OUT_FIDS = 2,        /* u32 root_fid per kept pair, CSR order */
    GFFX_OUT_TRIPLES = 4,     /* (root_fid, iv.start, iv.end) per kept pair == the reference's
                                 Vec<(u32,u32,u32)> (intersect.rs:162) */
    GFFX_OUT_ROOT_BITMAP = 8, /* one bit per root of the index: set iff the root is in >=1 kept pair */
    GFFX_OUT_OFFSETS = 16,    /* u64 start of every query's pair segment (nq+1 entries; [nq] = number of pairs).
                                 Direct strategy: the exclusive prefix of the counts (CSR in input order).
                                 Partitioned strategy: segments follow the order in which genome tiles were
                                 served, so the offsets are explicit -- they still tile [0, pairs) exactly. */
    GFFX_OUT_OFFSETS32 = 64,  /* the same segment starts as u32 (nq entries), for callers that know the pass keeps
                                 fewer than 2^32 pairs (the engine checks: _wait fails with GFFX_E_INVALID otherwise);
                                 halves the bytes the offsets cost.  Windows strategy only (AUTO picks it). */
    GFFX_OUT_BITMAP_KEEP = 128, /* with GFFX_OUT_ROOT_BITMAP: do not clear the batch's bitmap first -- a caller that streams a
                                 BED file chunk by chunk through one batch accumulates the unique roots of all chunks
                                 (commands/intersect.rs:598-615 dedups over the whole file) */
    GFFX_OUT_SEGBASE = 256,   /* windows strategy (AUTO picks it): per GROUP of 256 consecutive regions (regions 256 g .. 256 g + 255,
                                 a wave's share of a round) the u64 start of the group's run of pairs -- ceil(nq / 256)
                                 entries, 8 bytes per 256 regions.  The segments of a group's regions follow each other in
                                 input order, so region i's segment starts at segbase[i / 256] + the counts of the group's
                                 regions before i: a consumer that reads the counts anyway needs no per-region offsets
                                 (they are not part of the algorithmic bytes).  The runs tile [0, pairs) exactly. */
    GFFX_OUT_NO_COUNTS = 512, /* with GFFX_OUT_ROOT_BITMAP alone (windows strategy): the per-region counts need not be written -- a
                                 caller that only wants the unique roots (the CLI: commands/intersect.rs:598-615) saves their 4 bytes
                                 per region */
    GFFX_OUT_EMIT_ORDER = 32  /* partitioned strategy: leave the per-query results in emission order
                                 ({input row, count, offset} records: gffx_hip_batch_copy_query_records) and
                                 skip the scatter into input-order arrays; _copy_counts / _copy_offsets then
                                 run that scatter on demand */
};

enum gffx_strategy {
    GFFX_STRATEGY_AUTO = 0,   /* the engine picks: windows; fused for a batch of mostly wide regions */
    GFFX_STRATEGY_DIRECT = 1, /* queries in input order; bin directory + gathers from the L2-resident index */
    GFFX_STRATEGY_SORTED = 2, /* "partitioned": one-pass device radix partition of the batch by genome window,
                                 then a fused count+emit join served from LDS-staged index tiles */
    GFFX_STRATEGY_FUSED = 3,  /* queries in input order, ONE kernel: interleaved gathers from the L2-resident
                                 index, count + emit per block round; counts / offsets in input order, pair
                                 segments in the order rounds reserve them (offsets explicit) */
    /* 4 was GFFX_STRATEGY_SLOTS (round 1's slot index, superseded by WINDOWS and removed in round 3: _run rejects it) */
    GFFX_STRATEGY_WINDOWS = 5, /* AUTO's choice.  One 32-byte index LINE per region: the line of the genome window
                                 (<= 2^15 bp) the region ends in lists up to 4 candidate roots {start, end as 16-bit
                                 window-relative coordinates, root_fid}; longer lists, dense windows, wide and
                                 empty-width regions are deferred inside the round and served exactly (list tail /
                                 skip-link sweep).  Root-bitmap passes set bits in an LDS-private bitmap.  Output
                                 contract as FUSED.  Domain: end >= start for every root (an interval with end < start
                                 never leaves the reference's IntervalTree::build, utils/tree.rs:48-50). */
};

enum gffx_kernel_id { /* for gffx_hip_batch_kernel_ms */
    GFFX_K_JOIN_COUNT = 0,
    GFFX_K_JOIN_EMIT = 1,
    GFFX_K_SORT = 2,
    GFFX_K_LINES = 3,
    GFFX_K_FUSED = 4,
    GFFX_K_UNPERMUTE = 5,
    GFFX_K_FUSED_DIRECT = 6,
    GFFX_K_DEPTH = 7,
    GFFX_K_SLOTS = 8, /* (retired with the slots strategy; the number stays reserved) */
    GFFX_K_WINDOWS = 9,    /* k_join_roots: the windows strategy's root passes */
    GFFX_K_BITMAP_OR = 10, /* (k_bitmap_fold runs at gffx_hip_batch_wait, outside the profiled passes; the number stays reserved) */
    GFFX_K_WAVE = 11,      /* k_join_pairs: the windows strategy's pair passes (counts + root_fids / positions) */
    GFFX_K__COUNT = 12
};

typedef struct gffx_hip_index gffx_hip_index;
typedef struct gffx_hip_batch gffx_hip_batch;
typedef struct gffx_hip_lines gffx_hip_lines;
typedef struct gffx_hip_regions gffx_hip_regions;
typedef struct gffx_hip_depth gffx_hip_depth;
typedef struct gffx_hip_bam gffx_hip_bam;
typedef struct gffx_hip_sam gffx_hip_sam;
typedef struct gffx_hip_bed gffx_hip_bed;
typedef struct gffx_hip_union gffx_hip_union;
typedef struct gffx_hip_pileup gffx_hip_pileup;
typedef struct gffx_hip_profile gffx_hip_profile;
typedef struct gffx_hip_closest gffx_hip_closest;

int gffx_hip_abi_version(void);
/* number of visible HIP devices (0 when none / no driver); never fails */
int gffx_hip_device_count(void);
/* optional: pay the process's one-off HIP costs (runtime and context creation, code-object load) now -- a host
 * can call it on a side thread while it still parses its inputs.  Nothing depends on it. */
int gffx_hip_warmup(int device);
/* thread-local, valid until the next failing call on this thread */
const char *gffx_hip_last_error(void);

/* ---- index: replaces TreeIndexData.chr_entries (utils/tree_index.rs:12-16) ----------------
 * chr_offsets has n_chr+1 entries delimiting each seqid's root intervals in start/end/root_fid
 * (0-based half-open coordinates as the builder stores them, index_builder/core.rs:108-109;
 * any order inside a seqid -- the builder's file order is fine).  The library sorts each seqid
 * stably by start, adds the running maximum of `end`, builds the bin directory and uploads
 * everything to `device` once. */
int gffx_hip_index_create(uint32_t n_chr, const uint32_t *chr_offsets, const uint32_t *start,
                          const uint32_t *end, const uint32_t *root_fid, int device,
                          gffx_hip_index **out);
void gffx_hip_index_destroy(gffx_hip_index *);
uint32_t gffx_hip_index_n_chr(const gffx_hip_index *);
/* the index builders' knobs that are not at their defaults, as a JSON object ("{}": all defaults).  snprintf's contract: returns the
 * length the text needs; at most cap - 1 bytes and a NUL are written (buf may be NULL with cap 0). */
int gffx_hip_index_options(const gffx_hip_index *, char *buf, size_t cap);
uint64_t gffx_hip_index_n_roots(const gffx_hip_index *);
int gffx_hip_index_device(const gffx_hip_index *);
/* root_fid of the i-th bit of the root bitmap (i < n_roots), host array owned by the index */
const uint32_t *gffx_hip_index_sorted_fids(const gffx_hip_index *);

/* The same index on another device of the node (multi-GPU hosts replicate the index: the host-side build runs once,
 * the device arrays are copied GPU to GPU). */
int gffx_hip_index_clone(const gffx_hip_index *, int device, gffx_hip_index **out);

/* ---- region stores: streaming BED ingestion (commands/intersect.rs:201-230 parses the whole file into one Vec; a host
 * that parses chunk by chunk hands every chunk over through one of two PINNED staging buffers while it parses the next) --
 * A store keeps regions in HBM as AoS triples (chr, start, end).  keep_all = 1: every appended chunk stays (capacity_rows
 * in total; Join B needs all regions of the run: gffx_hip_lines_test_store); keep_all = 0: a ring of two chunk slots, the
 * chunk appended from staging buffer k overwrites slot k (the caller has waited for the batch that read it). */
int gffx_hip_regions_create(int device, uint64_t capacity_rows, uint64_t chunk_rows, int keep_all, gffx_hip_regions **out);
void gffx_hip_regions_destroy(gffx_hip_regions *);
/* pinned host buffer k (0 or 1), chunk_rows rows of 3 u32 */
uint32_t *gffx_hip_regions_staging(gffx_hip_regions *, int k);
/* block until the last append from staging buffer k has left the host buffer (it may then be refilled) */
int gffx_hip_regions_wait_staging(gffx_hip_regions *, int k);
/* asynchronous H2D copy of the first n_rows rows of staging buffer k to the store */
int gffx_hip_regions_append(gffx_hip_regions *, int k, uint64_t n_rows);
/* the same for a chunk that sits in staging buffer k in n_parts pieces (rows stage_first[p] .. + n_rows[p]: parser threads
 * fill disjoint parts of the buffer); the pieces land back to back in the store and count as ONE append */
int gffx_hip_regions_append_parts(gffx_hip_regions *, int k, uint32_t n_parts, const uint64_t *stage_first, const uint64_t *n_rows);
uint64_t gffx_hip_regions_rows(const gffx_hip_regions *); /* keep_all stores: rows appended so far */
/* The batch borrows rows [first, first + n_rows) of the chunk last appended from staging buffer k (no copy; the batch's
 * stream waits for that append).  They must stay untouched until the batch's pass has finished. */
int gffx_hip_batch_set_regions_store(gffx_hip_batch *, const gffx_hip_regions *, int k, uint64_t first, uint64_t n_rows);

/* ---- multi-GPU exchange step: all-gather of per-device {regions, kept pairs} over RCCL (xGMI), one rank per device,
 * single process (ncclCommInitAll).  counts_in: 2 values per device; counts_out: n_dev x (2 x n_dev) -- what every
 * device holds after the collective (all rows are equal).  `devices` must be distinct. */
int gffx_hip_allgather_counts(int n_dev, const int *devices, const uint64_t *counts_in, uint64_t *counts_out);

/* ---- query batches: replaces query_features (commands/intersect.rs:105-169) --------------- */
int gffx_hip_batch_create(const gffx_hip_index *, uint64_t max_queries, gffx_hip_batch **out);
void gffx_hip_batch_destroy(gffx_hip_batch *);

/* regions = nq AoS triples (chr, start, end): exactly the reference's &[(u32,u32,u32)]
 * (intersect.rs:107).  Copied host -> device on the batch's stream. */
int gffx_hip_batch_set_regions_host(gffx_hip_batch *, const uint32_t *regions, uint64_t nq);
/* same, from three host arrays */
int gffx_hip_batch_set_regions_soa_host(gffx_hip_batch *, const uint32_t *chr,
                                        const uint32_t *start, const uint32_t *end, uint64_t nq);
/* borrow three DEVICE arrays (SoA) already resident in HBM; they must stay valid until _wait */
int gffx_hip_batch_set_regions_device(gffx_hip_batch *, const uint32_t *d_chr,
                                      const uint32_t *d_start, const uint32_t *d_end, uint64_t nq);

/* Enqueue one pass of Join A over the batch on its stream (asynchronous). */
int gffx_hip_batch_run(gffx_hip_batch *, int mode, int invert, uint32_t out_flags, int strategy);
/* Block until the pass finished; grows the output buffers and replays the emit step when the
 * kept-pair count exceeded their capacity.  Returns GFFX_E_CHR_RANGE if a chr was out of range. */
int gffx_hip_batch_wait(gffx_hip_batch *);
/* Cheaper than _wait for pipelines: only checks that the stream drained (no capacity replay). */
int gffx_hip_batch_sync(gffx_hip_batch *);

uint64_t gffx_hip_batch_n_queries(const gffx_hip_batch *);
/* valid after _wait */
uint64_t gffx_hip_batch_total_hits(const gffx_hip_batch *);
/* After _wait: the kept pairs of ALL root passes (GFFX_OUT_ROOT_BITMAP alone, windows strategy) since the batch's last pass without
 * GFFX_OUT_BITMAP_KEEP -- what a caller that streams a BED file chunk by chunk through one batch reports per device
 * (commands/intersect.rs:105-169 returns the pairs of the whole file; the hit-count exchange of `gffx intersect --gpus N` carries
 * this number).  For any other last pass: the pass's own total (= gffx_hip_batch_total_hits). */
int gffx_hip_batch_kept_pairs_accumulated(gffx_hip_batch *, uint64_t *out);
int gffx_hip_batch_copy_counts(gffx_hip_batch *, uint32_t *host /* nq */);
int gffx_hip_batch_copy_offsets(gffx_hip_batch *, uint64_t *host /* nq+1 */);
int gffx_hip_batch_copy_offsets32(gffx_hip_batch *, uint32_t *host /* nq */); /* GFFX_OUT_OFFSETS32 */
int gffx_hip_batch_copy_segbase(gffx_hip_batch *, uint64_t *host /* ceil(nq / 256) */); /* GFFX_OUT_SEGBASE */
/* per-query records in emission order: rows[i] = input row, counts[i] = kept pairs, offsets[i] = start of
 * its segment in fids / triples (needs GFFX_OUT_OFFSETS); any pointer may be NULL; nq entries each */
int gffx_hip_batch_copy_query_records(gffx_hip_batch *, uint32_t *rows, uint32_t *counts, uint64_t *offsets);
int gffx_hip_batch_copy_fids(gffx_hip_batch *, uint32_t *host /* total_hits */);
int gffx_hip_batch_copy_triples(gffx_hip_batch *, uint32_t *host /* 3*total_hits */);
/* n_words = ceil(n_roots/64); bit i <-> gffx_hip_index_sorted_fids()[i] */
int gffx_hip_batch_copy_root_bitmap(gffx_hip_batch *, uint64_t *host, uint64_t n_words);
/* device views of the same buffers (NULL if not produced), for zero-copy consumers */
const uint32_t *gffx_hip_batch_device_counts(const gffx_hip_batch *);
const uint32_t *gffx_hip_batch_device_fids(const gffx_hip_batch *);
const uint64_t *gffx_hip_batch_device_offsets(const gffx_hip_batch *);
const uint32_t *gffx_hip_batch_device_offsets32(const gffx_hip_batch *);
const uint64_t *gffx_hip_batch_device_segbase(const gffx_hip_batch *);
const uint32_t *gffx_hip_batch_device_triples(const gffx_hip_batch *);
/* the batch's own device copy of the regions as AoS triples (after _set_regions_host; NULL for SoA / borrowed regions) */
const uint32_t *gffx_hip_batch_device_regions(const gffx_hip_batch *);
/* pre-size the pair buffers (pairs); avoids the capacity replay on the first run */
int gffx_hip_batch_reserve_hits(gffx_hip_batch *, uint64_t n_pairs);
/* Tuning knobs of the batch's passes ("Tuning knobs" above): set one by its name (with or without the GFFX_HIP_ prefix, any
 * case); GFFX_E_INVALID for an unknown name or a value outside the knob's range.  _options: the non-default ones as JSON. */
int gffx_hip_batch_set_option(gffx_hip_batch *, const char *name, long value);
int gffx_hip_batch_options(const gffx_hip_batch *, char *buf, size_t cap);

/* HIP-event timing of the kernels on the batch's own stream.  While enabled every launch is
 * bracketed by events; _kernel_ms returns the accumulated milliseconds and launch count of
 * one kernel since the last _reset_profile (events are resolved by _wait/_sync). */
int gffx_hip_batch_set_profiling(gffx_hip_batch *, int enabled);
int gffx_hip_batch_kernel_ms(gffx_hip_batch *, int kernel_id, double *total_ms, uint64_t *launches);
int gffx_hip_batch_reset_profile(gffx_hip_batch *);
/* n passes back to back on the batch's stream between ONE pair of HIP events (blocking): total_ms / n = the average
 * launch-to-launch duration of a pass without an event pair per launch */
int gffx_hip_batch_timed_runs(gffx_hip_batch *, int mode, int invert, uint32_t out_flags, int strategy, uint32_t n,
                              double *total_ms);
/* n_passes passes enqueued round-robin over n_batches batches (batch i % n_batches takes pass i) in one call: a host that
 * keeps several batches in flight pays one FFI crossing for the lot (bench.py's timed region: the launch loop runs in C).
 * Round 6: consecutive passes over DISTINCT batches of one index that resolve to the same pass of the windows strategy are served
 * by ONE launch per group of up to 8 batches (every batch a share of the launch's blocks, its rounds handed out by ticket): the
 * index lines are fetched into the L2s once per launch instead of once per batch, ramp and drain are paid once.  The launch runs on
 * a stream of the index; a batch's own stream joins it whenever the batch is used on its own again (_run, _wait, _sync, a new set of
 * regions): per-batch order is what it always was.  Up to three batches run pass by pass (their launches share the chip as in round
 * 5); from four on the batches are cut into groups of equal size (<= 8), half of them on each of two such streams, so that one group's
 * drain overlaps the next one's ramp.  Results are exactly those of n_passes single _run calls.  Knob GFFX_HIP_GROUP of batches[0]
 * ("Tuning knobs" above).
 * On failure: the arguments and every batch that takes a pass (NULL, no regions set, a mode, strategy or flags _run would refuse) are
 * checked before anything runs -- a call that fails there launches nothing, and every batch keeps its last completed pass (a _wait
 * and the results read what that pass left).  A failure after that (a HIP or allocation error of one batch) leaves the passes
 * enqueued before it, and those of the batches already prepared for the same launch, as passes run one by one: every batch the
 * call marked as run has a real pass behind its next _wait; the failing batch itself is in the state a failed _run leaves. */
int gffx_hip_batches_run_n(gffx_hip_batch *const *batches, uint32_t n_batches, int mode, int invert, uint32_t out_flags,
                           int strategy, uint64_t n_passes);
/* How _batches_run_n cuts passes over these batches into launches: *groups per walk over the batches (0: pass by pass), the *largest
 * group's size, the *streams the groups alternate between (any pointer may be NULL). */
int gffx_hip_batches_plan(gffx_hip_batch *const *batches, uint32_t n_batches, uint32_t *groups, uint32_t *largest, uint32_t *streams);
/* n_launches times ONE pass over each of the n_batches (<= 8) batches -- the launch _batches_run_n issues for such a group --, back
 * to back between one pair of HIP events on the stream they run on (blocking): total_ms / n_launches = the duration of the launch.
 * *grouped (may be NULL) = 1 when the passes ran as one launch, 0 when they did not group (then: pass after pass on batches[0]'s
 * stream is NOT what was timed -- the figure is meaningless). */
int gffx_hip_batches_timed_runs(gffx_hip_batch *const *batches, uint32_t n_batches, int mode, int invert, uint32_t out_flags,
                                int strategy, uint32_t n_launches, double *total_ms, uint32_t *grouped);
/* Threads per block of the last windows-strategy pair pass of this batch (512 or 1024; 0: none ran).  The engine takes
 * 1024-thread blocks (one per CU, rounds of 4096 regions) for a batch of 500 000 regions or more while NO other batch of the
 * index has passes in flight, 512-thread blocks (two per CU: kernels of two batches share the CUs) otherwise;
 * The knob GFFX_HIP_WIN_THREADS (512 / 1024) forces one. */
uint32_t gffx_hip_batch_block_threads(const gffx_hip_batch *);
/* Blocks of that launch: as many as the device has slots for (256 blocks of 1024 threads, 512 of 512 threads), fewer for a small
 * batch (a block per round of 4 x threads regions) -- and 256 blocks of 512 threads (one per CU) for a pair pass over at most ~2 M
 * regions launched while TWO OR MORE other batches of the index have passes in flight: kernels of different streams run side by side only when each leaves
 * slots free, and that is where three batches in flight gain (measured; with one other batch in flight the full grid is better).
 * A root pass (GFFX_OUT_ROOT_BITMAP alone) takes one block per CU as soon as ONE other batch is in flight (measured likewise).
 * The knob GFFX_HIP_FUSED_BLOCKS forces a count (GFFX_HIP_BITMAP_BLOCKS: the root passes'). */
uint32_t gffx_hip_batch_block_count(const gffx_hip_batch *);
/* The batch's own blocks of that launch: the whole grid for a launch that serves one batch; for a launch that serves a group of
 * batches (gffx_hip_batches_run_n) _block_count is the launch's grid and this the batch's share of it. */
uint32_t gffx_hip_batch_block_share(const gffx_hip_batch *);
/* A launch that serves a group reads every batch's buffers through buffer descriptors the host put into the batch's record -- the
 * regions, the counts, the pair buffer, the segment bases, each spanning the WHOLE buffer; a round's or a run's place is a 32-bit byte
 * offset and the hardware's range check drops what lies beyond the batch or the capacity.  The rule: only when every descriptor of
 * every batch of the launch spans at most 2^31 bytes (12 bytes per region: n_regions <= 2^31 / 12; 4 per word of the pair buffer:
 * capacity_words <= 2^29 -- ignored for a pass without pair output, has_pair_output 0), so that the offset 2^31 lies beyond every
 * buffer; otherwise the launch runs the instantiations that build a descriptor per round, as a lone batch's launches do.  Results
 * are the same either way.  Returns 1 when a batch of that size takes the descriptors, else 0 (a pure function: no device). */
int gffx_hip_group_descriptors_fit(uint64_t n_regions, uint64_t capacity_words, int has_pair_output);
/* Coverage filter the batch's last windows-strategy launch staged in LDS: 0 none (the mixed form, or nothing fitted), 1 the coarse
 * one (GFFX_HIP_WIN_FILTER_KB), 2 the fine one (GFFX_HIP_WIN_FILTER_FINE_KB).  A launch takes the fine one where it fits beside its
 * other tables and strips and its blocks run four rounds or more (about 4 M regions: the larger bitmap is staged once per block);
 * GFFX_HIP_WIN_FILTER=1 holds a batch's launches to the coarse one, =2 takes the fine one wherever it fits. */
uint32_t gffx_hip_batch_filter_level(const gffx_hip_batch *);
/* 1 when the last run's passes took the MIXED form of the window kernels (every mode, inverted or not; round 4's "wide form" is
 * its all-wide Overlap case): every region is served its own way in one launch -- a region the index lines answer (up to 16 Ki bases by default) from ONE
 * line as in the narrow form, a wider one from two index lines and two rank words, no sweep.  AUTO chooses it for a batch with
 * more than one wide row in 128: found by a sample of the rows gffx_hip_batch_set_regions_host / _soa_host are given (each judged
 * against its own seqid's line width), or -- regions already on the device -- by a previous waited pass of the narrow form, which
 * counts the rows its lines did not answer.  What a wide region keeps in each mode: join_pairs_kernels.hpp, pair_locate_mixed
 * (Contained: its run of roots filtered by their ends; ContainsRegion: the roots over its first base that reach its end).  The knob
 * GFFX_HIP_WIN_WIDE (0 never / 1 AUTO / 2 every eligible pass of the windows strategy) steers it. */
int gffx_hip_batch_wide_form(const gffx_hip_batch *);

/* One-shot drop-in for query_features (commands/intersect.rs:105-111): host regions in, host
 * triples out (malloc'd by the library, release with gffx_hip_free_host). */
int gffx_hip_query_features(const gffx_hip_index *, const uint32_t *regions, uint64_t nq, int mode,
                            int invert, uint32_t **triples_out, uint64_t *n_triples);
void gffx_hip_free_host(void *);

/* ---- Join B: the numeric core of gff_line_overlaps_queries (commands/intersect.rs:500-521) -
 * A line table is the (seqid number, raw column-4 start, raw column-5 end) of GFF lines,
 * in file order, uploaded once.  seq == UINT32_MAX marks a line that can never match (seqid
 * without queries / unparsable columns).  _test evaluates, for every line, whether ANY region
 * of the line's seqid satisfies the literal closed-interval predicate of the given mode
 * (no invert: intersect.rs:232-240 has no such parameter) and writes one byte per line. */
int gffx_hip_lines_create(int device, uint64_t n_lines, const uint32_t *seq, const uint32_t *start,
                          const uint32_t *end, gffx_hip_lines **out);
void gffx_hip_lines_destroy(gffx_hip_lines *);
/* regions = AoS triples as above (all regions of the run, BED order: intersect.rs:621-633);
 * n_seq = number of seqids; keep_host receives n_lines bytes (0/1). */
int gffx_hip_lines_test(gffx_hip_lines *, const uint32_t *regions, uint64_t nq, uint32_t n_seq,
                        int mode, uint8_t *keep_host);
/* the same with the regions already in HBM as AoS triples (e.g. gffx_hip_batch_device_regions of the batch Join A ran on) */
int gffx_hip_lines_test_device(gffx_hip_lines *, const uint32_t *d_regions, uint64_t nq, uint32_t n_seq,
                               int mode, uint8_t *keep_host);
/* ... or in a region store (keep_all = 1): all rows appended so far */
int gffx_hip_lines_test_store(gffx_hip_lines *, const gffx_hip_regions *, uint32_t n_seq, int mode, uint8_t *keep_host);
/* HIP-event duration (ms) of the line kernel (k_lines_exists2; k_lines_exists when regions with start > end exist) in the last
 * _test call, on the table's own stream */
double gffx_hip_lines_last_kernel_ms(const gffx_hip_lines *);
/* ... and of the device preparation of the region tables before it: radix sort by (seqid, start), running max / min of the
 * ends, the bin directory and -- Overlap mode, when the run has regions with start > end -- the sort of those regions' ends
 * (the reference builds `query_ivmap` on the CPU: intersect.rs:621-633) */
double gffx_hip_lines_last_prep_ms(const gffx_hip_lines *);
/* radix passes of the last call's region sort by (seqid, start): 4 when the mixed-radix top digit (seqid, start >> 24) fits 256 values
 * (GRCh38-scale BED files), else 4 + one per byte of the seqid count */
int gffx_hip_lines_last_sort_passes(const gffx_hip_lines *);
/* The region tables of the last _test, for parity checks: q_off (n_seq + 1 entries), then per region in (seqid, start)
 * order (stable: equal starts keep the order of `regions`): QS = start, PM = running max of `end` inside the seqid, SM =
 * running min of `end` from the seqid's last region backwards, CD = regions with start > end before this position (all
 * seqids).  Any pointer may be NULL. */
int gffx_hip_lines_copy_tables(gffx_hip_lines *, uint64_t *q_off, uint32_t *qs, uint32_t *pm, uint32_t *sm, uint32_t *cd);
/* ... the bin directory over QS: d_off (n_seq + 1), shift_nb ({shift, bins} per seqid), dir_qs (d_off[n_seq] entries;
 * dir[d_off[c] + b] = first position of seqid c whose start >= b << shift, entry `bins` = the seqid's end) ... */
int gffx_hip_lines_copy_dirs(gffx_hip_lines *, uint64_t *d_off, uint32_t *shift_nb, uint32_t *dir_qs);
/* ... and, after an Overlap-mode _test, the regions with start > end: their number, dq_off (n_seq + 1) and their ends
 * sorted per seqid (de: *n_deg entries; call with de = NULL first to learn the size). */
int gffx_hip_lines_copy_degenerate(gffx_hip_lines *, uint64_t *n_deg, uint64_t *dq_off, uint32_t *de);

/* ---- `gffx depth` with a BED source: compute_hit_depth / compute_root_depth (commands/depth.rs:121-293) --
 * The host parses every root BLOCK once (the byte range of a .gof record; for a root_fid with several
 * records the LAST one, index_loader/gof.rs:32-37) into the lines that carry an ID, with the 0-based
 * half-open coordinates of depth.rs:145-147.  Inside a block the lines are ordered by ID; a GROUP is one
 * (block, ID) -- the unit depth.rs:202-206 dedups on -- numbered globally.  block_of_fid[root_fid] is
 * the block (UINT32_MAX: no usable record, depth.rs:242-243).
 * _accumulate adds the regions of a finished Join A pass (Overlap, no invert, GFFX_OUT_FIDS |
 * GFFX_OUT_OFFSETS): per group the number of regions with an overlapping line (a region counts a root
 * once, depth.rs:241) and the min start / max end of the overlapped lines (UINT32_MAX / 0 when none). */
int gffx_hip_depth_create(int device, uint32_t n_groups, uint32_t n_blocks, const uint64_t *block_line_off /* n_blocks+1 */,
                          const uint32_t *line_start, const uint32_t *line_end, const uint32_t *line_group,
                          uint32_t n_fid, const uint32_t *block_of_fid, gffx_hip_depth **out);
void gffx_hip_depth_destroy(gffx_hip_depth *);
int gffx_hip_depth_accumulate(gffx_hip_depth *, gffx_hip_batch *);
int gffx_hip_depth_reset(gffx_hip_depth *);
int gffx_hip_depth_copy(gffx_hip_depth *, uint64_t *depth, uint32_t *min_start, uint32_t *max_end /* n_groups each */);

/* ---- `gffx coverage` with a BED source: the covered bases of feature segments (commands/coverage.rs:339-364) --
 * covered_out[i] = |[seg_start[i], seg_end[i])  ∩  union of the regions of seqid seg_seq[i]|  (regions = AoS
 * (chr, start, end) rows with start < end; touching regions merge like merge_intervals, coverage.rs:92-109).
 * For a segment inside its root's interval this equals the reference's per-root figure: a region that overlaps
 * the segment then hits the root.  Segments sticking out of their root are the caller's to handle. */
int gffx_hip_segments_covered(int device, uint64_t n_seg, const uint32_t *seg_seq, const uint32_t *seg_start,
                              const uint32_t *seg_end, const uint32_t *regions, uint64_t nq, uint32_t n_seq,
                              uint32_t *covered_out);

/* ---- union builder: merge_intervals (commands/coverage.rs:92-109) over all rows of a run, on the device --
 * A union holds, per seqid, the rows added so far merged into sorted, disjoint, non-touching spans: sort by start, merge while
 * s <= current end (touching rows merge).  Rows are (seqid, start, end) with seqid < n_seq (else GFFX_E_CHR_RANGE) and
 * start < end (else GFFX_E_INVALID); n_seq may exceed 256.  Every _add sorts its rows together with the spans so far by
 * (seqid, start) on the device and rebuilds the spans; the spans are the connected components of the rows, so ANY grouping of the
 * rows into _add calls, and spans exchanged between unions with _add_spans, give the same spans bit for bit.  Device memory is
 * bounded by the spans plus one internal fold of rows, not by the rows added; the host keeps nothing per row.
 *   _add_host    rows in host memory (copied through a pinned staging buffer inside), any number of calls
 *   _add_store   rows [first, first + n_rows) of the chunk last appended to a region store from staging buffer k: no second
 *                upload.  The call returns when the rows have been read.
 *   _add_spans   the spans of another union as _copy_spans gives them (u_off: n_seq + 1 entries)
 *   _finish      builds pb (covered bases of the seqid's spans before this one), u_off and the directory; the union is
 *                queryable afterwards.  A later _add makes it unfinished again.
 *   _copy_spans  after _finish: u_off (n_seq + 1), us / ue / pb (_n_spans entries each); any pointer may be NULL
 *   _segments_covered  after _finish: as gffx_hip_segments_covered, against the union's spans
 *   _stats       HIP-event milliseconds of the sort and span kernels so far, rows added, device folds run
 * After an error the object only reports it again. */
int gffx_hip_union_create(int device, uint32_t n_seq, gffx_hip_union **out);
int gffx_hip_union_add_host(gffx_hip_union *, const uint32_t *rows /* 3 per row */, uint64_t n_rows);
int gffx_hip_union_add_store(gffx_hip_union *, const gffx_hip_regions *, int k, uint64_t first, uint64_t n_rows);
int gffx_hip_union_add_spans(gffx_hip_union *, const uint64_t *u_off, const uint32_t *us, const uint32_t *ue);
int gffx_hip_union_finish(gffx_hip_union *);
uint64_t gffx_hip_union_n_spans(const gffx_hip_union *);
int gffx_hip_union_copy_spans(gffx_hip_union *, uint64_t *u_off, uint32_t *us, uint32_t *ue, uint64_t *pb);
int gffx_hip_union_segments_covered(gffx_hip_union *, uint64_t n_seg, const uint32_t *seg_seq, const uint32_t *seg_start,
                                    const uint32_t *seg_end, uint32_t *covered_out);
int gffx_hip_union_stats(const gffx_hip_union *, double *kernel_ms, uint64_t *rows, uint64_t *folds);
void gffx_hip_union_destroy(gffx_hip_union *);

/* ---- pileup: the bases the source rows lay on feature segments (`gffx coverage --mean-depth`; an addition, the reference
 * has no such figure) --
 * For segment i = [seg_start[i], seg_end[i]) on seqid seg_seq[i] and the rows (seqid, s, e) added so far (0-based, half-open):
 *     bases[i] = sum over the rows of that seqid of max(0, min(e, seg_end[i]) - max(s, seg_start[i]))
 * a 64-bit integer; a segment with start >= end has 0.  Mean depth = bases / segment length.  The figure is a sum over rows:
 * ANY grouping of the rows into _add calls, and rows spread over several pileups whose totals are added, give the same numbers.
 * Rows must have seqid < n_seq (else GFFX_E_CHR_RANGE) and start < end (else GFFX_E_INVALID), as for the union builder.
 * Nothing is allocated per base: every fold of at most gffx_hip_pileup_fold_rows() rows sorts the rows' starts and ends on the
 * device, takes their prefix sums and answers every segment with four searches (device/pileup_core.hpp).
 *   _create      the segments are copied to the device and stay; seg_seq[i] >= n_seq: GFFX_E_INVALID; n_seg == 0 is legal
 *   _add_host    rows in host memory (copied through a pinned staging buffer inside), any number of calls
 *   _add_store   rows [first, first + n_rows) of the chunk last appended to a region store from staging buffer k, read in place.
 *                Both _add calls return when the rows have been read and checked; the device goes on behind the call.
 *                A call of more than _fold_rows() rows is cut into folds: a refused row keeps its own fold out of the totals,
 *                the folds before it are in (the object has failed by then, so the totals can no longer be read).
 *   _copy        waits for the folds, then bases[0 .. n_seg): the running totals, legal between adds
 *   _reset       the totals back to zero; the segments stay
 *   _stats       HIP-event milliseconds of all kernels so far, rows added, folds run (waits for the folds);
 *   _stage_ms    the same time by stage: the key kernel, the two sorts, the prefix sums and offsets, the segment kernel
 *   _fold_rows / _scan_tile   constants of the build: rows per fold, records per block of the prefix-sum kernels
 * After a refused row or a failed HIP call the object only reports that error again; a refused ARGUMENT (NULL rows, rows beyond
 * the last append, a store on another device) leaves it usable. */
int gffx_hip_pileup_create(int device, uint32_t n_seq, uint64_t n_seg, const uint32_t *seg_seq, const uint32_t *seg_start,
                           const uint32_t *seg_end, gffx_hip_pileup **out);
int gffx_hip_pileup_add_host(gffx_hip_pileup *, const uint32_t *rows /* 3 per row */, uint64_t n_rows);
int gffx_hip_pileup_add_store(gffx_hip_pileup *, const gffx_hip_regions *, int k, uint64_t first, uint64_t n_rows);
int gffx_hip_pileup_copy(gffx_hip_pileup *, uint64_t *bases /* n_seg */);
int gffx_hip_pileup_reset(gffx_hip_pileup *);
int gffx_hip_pileup_stats(const gffx_hip_pileup *, double *kernel_ms, uint64_t *rows, uint64_t *folds);
int gffx_hip_pileup_stage_ms(const gffx_hip_pileup *, double *keys, double *sorts, double *scan, double *segments);
uint64_t gffx_hip_pileup_fold_rows(void);
uint32_t gffx_hip_pileup_scan_tile(void);
void gffx_hip_pileup_destroy(gffx_hip_pileup *);

/* ---- pileup, second consumer: the stranded depth profile around features (`gffx meta`; device/meta_core.hpp has the rule,
 * DESIGN 23) --
 * Features [feat_start[i], feat_end[i]) on seqid feat_seq[i], on the minus strand where feat_minus[i] != 0, and a layout: in
 * point mode (0) B = (up + down) / bin columns of `bin` bases around the anchor (0 tss, 1 tes, 2 center), in scaled mode (1)
 * up / bin columns before the feature, body_bins columns over it, whatever its length, and down / bin behind it.  Columns run in
 * the direction of transcription: a minus feature is the mirror image of a plus one.  Every column boundary is clamped to
 * [0, seq_len[seqid]] (seq_len NULL: 2^32 - 1).  Per feature i and column j, with [a, b) the clamped column,
 *     matrix[i * B + j] = the pileup's bases(a, b) over the rows added so far,  len[i][j] = b - a
 *     col_bases[j] = sum_i matrix[i][j],  col_len[j] = sum_i len[i][j],  col_features[j] = #{i : len[i][j] > 0}
 * all unsigned 64-bit sums over rows: any grouping of the rows into _add calls, and rows spread over several pileups whose
 * totals are added, give the same numbers.  The pileup keeps its segments: _copy gives what it gives without features.
 *   _meta_set          the features are copied to the device and stay (a second call replaces them and zeroes the totals);
 *                      col_len and col_features are computed here.  keep_matrix == 0: only the B column totals exist.
 *                      GFFX_E_INVALID, the handle stays usable: a seqid >= n_seq, start >= end, a layout that is none (bin == 0,
 *                      up or down no multiple of bin, no column), more than _meta_max_columns() columns.  n_feat == 0 is legal.
 *   _meta_copy         waits for the folds; B words each (any may be NULL), and the n_feat x B matrix (NULL unless kept)
 *   _meta_columns      B of a layout, 0 for one that is none (it may exceed the limit)
 *   _meta_ms           HIP-event milliseconds of the meta kernel over all folds so far (not part of _stats)
 *   _meta_max_columns / _meta_tile   constants of the build: the column limit, the features per block of the kernel
 * _reset zeroes the column totals and the matrix too. */
typedef struct {
    uint32_t mode;      /* 0 point, 1 scaled */
    uint32_t anchor;    /* point mode: 0 tss, 1 tes, 2 center */
    uint32_t up, down;  /* bases before / behind, multiples of bin */
    uint32_t bin;
    uint32_t body_bins; /* scaled mode: M */
} gffx_hip_meta_layout;
int gffx_hip_pileup_meta_set(gffx_hip_pileup *, uint64_t n_feat, const uint32_t *feat_seq, const uint32_t *feat_start,
                             const uint32_t *feat_end, const uint8_t *feat_minus, const uint32_t *seq_len /* n_seq or NULL */,
                             const gffx_hip_meta_layout *, int keep_matrix);
int gffx_hip_pileup_meta_copy(gffx_hip_pileup *, uint64_t *col_bases, uint64_t *col_len, uint64_t *col_features /* B each */,
                              uint64_t *matrix /* n_feat x B, NULL unless keep_matrix */);
int gffx_hip_pileup_meta_ms(const gffx_hip_pileup *, double *ms);
uint64_t gffx_hip_pileup_meta_columns(const gffx_hip_meta_layout *);
uint32_t gffx_hip_pileup_meta_max_columns(void);
uint32_t gffx_hip_pileup_meta_tile(void);

/* ---- depth profile: how deep every base is covered (`gffx coverage --thresholds / --bedgraph`; an addition, the reference has
 * no such figure) --
 * Coordinates are 0-based and half-open.  For seqid c and the rows [s, e) added so far, depth_c(x) = #{rows with s <= x < e}.
 * The CANONICAL profile of a seqid is the list of points (pos_i, d_i): pos strictly ascending, d_i the depth on
 * [pos_i, pos_{i+1}), d_i != d_{i-1} (d_{-1} = 0, so d_0 != 0), the last depth 0; a seqid without rows has no points.  It is a
 * function of the multiset of rows only: ANY grouping of the rows into _add calls, any order, and profiles merged with
 * _add_points give the same points bit for bit.  Rows must have seqid < n_seq (else GFFX_E_CHR_RANGE, looked at first) and
 * start < end (else GFFX_E_INVALID), as for the union builder and the pileup.
 * Depths are uint32_t: a profile that has been given 2^32 - 1 rows refuses further rows with GFFX_E_INVALID (for points merged
 * in with _add_points their largest depth counts as that many rows).  One fold sorts the points carried so far plus two records
 * per new row; together they must stay below the device sort's limit of 2^30 records, beyond it the add fails with
 * GFFX_E_INVALID and a message that says so.  Nothing is allocated per base (device/profile.hip, device/profile_core.hpp).
 *   _create       one object per device, on a stream of its own
 *   _add_host     rows in host memory (copied through a pinned staging buffer inside), any number of calls
 *   _add_store    rows [first, first + n_rows) of the chunk last appended to a region store from staging buffer k, read in place.
 *                 Both return when the rows have been read and checked (an event behind the first kernels of the fold): the
 *                 caller may refill the slot, the device goes on behind the call.  A call of more than _fold_rows() rows is cut
 *                 into folds; nothing of a refused fold enters the profile.
 *   _add_points   another profile's points as _copy_points gives them (the merge over devices).  Points that are not canonical
 *                 are refused with GFFX_E_INVALID: positions not strictly ascending inside a seqid, a seqid whose last depth is
 *                 not 0, a first depth of 0, two equal consecutive depths, a p_off that does not ascend from 0.  The points are
 *                 checked on the device through the fold's error word.
 *   _finish       waits for the folds and builds p_off (the points with seqid < c, c = 0 .. n_seq) on the device.  A later add
 *                 makes the profile unfinished again.
 *   _n_points     the points so far (waits for the fold in flight)
 *   _copy_points  p_off[n_seq + 1], pos[n_points], depth[n_points]; any pointer may be NULL.  GFFX_E_STATE before _finish.
 *   _union_at_least   the spans "depth >= T" as a union object on the profile's device: finished, the caller's to use
 *                 (gffx_hip_union_segments_covered, _copy_spans, ...) and to destroy.  The spans are written on the device and
 *                 never leave it.  T == 0: GFFX_E_INVALID; a T above every depth gives a union of no spans.  GFFX_E_STATE
 *                 before _finish.  T = 1 gives exactly the union builder's spans of the same rows.
 *   _reset        no points; the buffers stay
 *   _stats        HIP-event milliseconds of all fold kernels so far, rows added, folds run (waits for the fold in flight)
 *   _stage_ms     the same time by stage: the event kernels, the sort, the running depth, the compaction to points
 *   _fold_rows / _scan_tile   constants of the build: new rows per fold, records per block of the scan kernels
 * After a refused row, refused points or a failed HIP call the object only reports that error again; a refused ARGUMENT (NULL
 * rows, a store on another device, rows beyond the last append, T == 0) leaves it usable. */
int gffx_hip_profile_create(int device, uint32_t n_seq, gffx_hip_profile **out);
int gffx_hip_profile_add_host(gffx_hip_profile *, const uint32_t *rows /* 3 per row */, uint64_t n_rows);
int gffx_hip_profile_add_store(gffx_hip_profile *, const gffx_hip_regions *, int k, uint64_t first, uint64_t n_rows);
int gffx_hip_profile_add_points(gffx_hip_profile *, const uint64_t *p_off, const uint32_t *pos, const uint32_t *depth);
int gffx_hip_profile_finish(gffx_hip_profile *);
uint64_t gffx_hip_profile_n_points(const gffx_hip_profile *);
int gffx_hip_profile_copy_points(gffx_hip_profile *, uint64_t *p_off, uint32_t *pos, uint32_t *depth);
int gffx_hip_profile_union_at_least(gffx_hip_profile *, uint32_t T, gffx_hip_union **out);
int gffx_hip_profile_reset(gffx_hip_profile *);
int gffx_hip_profile_stats(const gffx_hip_profile *, double *kernel_ms, uint64_t *rows, uint64_t *folds);
int gffx_hip_profile_stage_ms(const gffx_hip_profile *, double *events, double *sort, double *scan, double *points);
uint64_t gffx_hip_profile_fold_rows(void);
uint32_t gffx_hip_profile_scan_tile(void);
void gffx_hip_profile_destroy(gffx_hip_profile *);

/* ---- closest: the roots nearest to every region, and how far away (`gffx closest`; an addition, the reference has no such
 * command) --
 * Coordinates are 0-based and half-open.  The roots of the region's seqid are taken in index position order (start ascending,
 * stable); a root [fs, fe) has fe >= fs.  For a region (c, qs, qe) with qs < qe every root of seqid c is in exactly one class:
 *     OVER   fs < qe && fe > qs     gap 0
 *     LEFT   fe <= qs               gap qs - fe + 1
 *     RIGHT  fs >= qe               gap fs - qe + 1        (adjacent intervals: gap 1, as in bedtools; a gap fits 32 bits)
 * GFFX_CLOSEST_IGNORE_OVERLAPS removes the OVER class from the candidates, GFFX_CLOSEST_LEFT_ONLY the RIGHT class,
 * GFFX_CLOSEST_RIGHT_ONLY the LEFT class (OVER counts for every side).  The ANSWER of a region is every candidate of minimal gap,
 * in ascending index position; a region without candidates, and a row with qs >= qe, has an empty answer (no error).  The
 * signed distance of an answered root is -gap for LEFT, +gap for RIGHT, 0 for OVER: it follows from the triple and the region,
 * so one gap per region is stored.  Both _ONLY bits together, or an unknown bit: GFFX_E_INVALID.
 *   _create       on the index's device, with a stream of its own, for runs of at most max_queries regions.  Builds the END TABLE
 *                 on the device (device/closest.hip): the roots' ends sorted stably by (seqid, end) with the position each came
 *                 from -- equal ends keep ascending position.  The index must outlive the handle.
 *   _run_host     regions as AoS triples (chr, start, end) in host memory (free again when the call returns)
 *   _run_store    rows [first, first + n_rows) of the chunk last appended to a region store from staging buffer k, read in place
 *                 (untouched until _wait).  Both run the count pass, wait for it, size the pair buffer from its total and
 *                 enqueue the emit pass.  A row with chr >= n_chr: GFFX_E_CHR_RANGE from the _run call (nothing is read for
 *                 that row; the run is void, the handle stays usable).
 *   _wait         the emit pass has finished; the results below are GFFX_E_STATE before it
 *   _total_pairs  answered roots over all regions
 *   _copy_counts  counts[nq]; _copy_offsets  offsets[nq + 1], the exclusive prefix of the counts in INPUT order (a deterministic
 *                 CSR); _copy_triples  (root_fid, fs, fe) per answered root, 3 * pairs words; _copy_gaps  gaps[nq], undefined
 *                 where the count is 0
 *   _copy_end_table   e_end[n_roots], e_pos[n_roots] (either may be NULL); seqid c's slice is that of its roots' positions
 *   _last_kernel_ms   HIP-event milliseconds of the last run's two kernels
 *   _last_grid    the last run's launch: blocks, and regions per block
 *   _stats        HIP-event milliseconds of the end table's build; how often a run had to grow the pair buffer
 * After a failed HIP call the object only reports that error again; a refused ARGUMENT (bad flags, too many regions, NULL
 * regions, a store on another device, rows beyond the last append) and GFFX_E_CHR_RANGE leave it usable.  Without a device
 * _create returns GFFX_E_NO_DEVICE. */
enum gffx_closest_flags { GFFX_CLOSEST_IGNORE_OVERLAPS = 1, GFFX_CLOSEST_LEFT_ONLY = 2, GFFX_CLOSEST_RIGHT_ONLY = 4 };
int gffx_hip_closest_create(const gffx_hip_index *, uint64_t max_queries, gffx_hip_closest **out);
int gffx_hip_closest_run_host(gffx_hip_closest *, const uint32_t *regions /* 3 per region */, uint64_t nq, uint32_t flags);
int gffx_hip_closest_run_store(gffx_hip_closest *, const gffx_hip_regions *, int k, uint64_t first, uint64_t n_rows, uint32_t flags);
int gffx_hip_closest_wait(gffx_hip_closest *);
int gffx_hip_closest_total_pairs(gffx_hip_closest *, uint64_t *pairs);
int gffx_hip_closest_copy_counts(gffx_hip_closest *, uint32_t *counts /* nq */);
int gffx_hip_closest_copy_offsets(gffx_hip_closest *, uint64_t *offsets /* nq + 1 */);
int gffx_hip_closest_copy_triples(gffx_hip_closest *, uint32_t *triples /* 3 * pairs */);
int gffx_hip_closest_copy_gaps(gffx_hip_closest *, uint32_t *gaps /* nq */);
int gffx_hip_closest_copy_end_table(gffx_hip_closest *, uint32_t *e_end, uint32_t *e_pos);
int gffx_hip_closest_last_kernel_ms(gffx_hip_closest *, double *ms);
int gffx_hip_closest_last_grid(const gffx_hip_closest *, uint32_t *blocks, uint64_t *chunk);
int gffx_hip_closest_stats(const gffx_hip_closest *, double *build_ms, uint64_t *grows);
void gffx_hip_closest_destroy(gffx_hip_closest *);

/* ---- class map: per region the bases of every feature class (`gffx annotate`; an addition, the reference has no such
 * command) --
 * T layers of intervals [start, end) per seqid in priority order, 1 <= T <= 32.  class(x) = the smallest k such that an
 * interval of layer k covers base x, or T ("none").  The CLASS MAP of a seqid is the canonical list of points (pos_i, class_i):
 * pos strictly ascending, class_i the class on [pos_i, pos_{i+1}), class_i != class_{i-1}, the first class not T, the last
 * class T; a seqid without intervals has no points.  It is a function of the multiset of rows: any grouping into calls, any
 * order and duplicates give the same points bit for bit.  For a region (c, qs, qe) with qs < qe, bases_k = the bases of
 * [qs, qe) with class k, k = 0 .. T (they add up to qe - qs), and the region's class is the smallest k < T with bases_k > 0,
 * or T; qs >= qe gives zeros and T (device/classmap.hip, device/classmap_core.hpp).
 *   _create        n_seq * n_layers must fit 32 bits and n_layers be 1 .. 32, else GFFX_E_INVALID
 *   _add_rows_host rows (layer, seqid, start, end), any number of calls.  layer >= n_layers or seqid >= n_seq:
 *                  GFFX_E_CHR_RANGE (looked at first); start >= end: GFFX_E_INVALID -- the union builder's codes.  A refused
 *                  row is an error of the object: it only reports it again
 *   _finish        builds the points, p_off and the running sums on the device; rows added later need another _finish
 *   _n_points, _copy_points   p_off[n_seq + 1], pos[n_points], cls[n_points] (any may be NULL); _copy_bases  cb[k * n_points + i]
 *                  = the bases of class k < T on all points before point i (over all seqids)
 *   _run_host, _run_store     as for closest; GFFX_E_STATE before _finish.  A row with chr >= n_seq: GFFX_E_CHR_RANGE from the
 *                  _run call (nothing is read for that row; the run is void, the object stays usable)
 *   _wait, _copy_counts  counts[nq * (T + 1)], _copy_class  one byte per region (T for none), _last_kernel_ms
 *   _stage_ms      HIP-event milliseconds of the build: union, toggles, sort, scan, points, bases
 *   _scan_tile, _block_size   events per scan tile; regions per block of the regions kernel */
typedef struct gffx_hip_classmap gffx_hip_classmap;
int gffx_hip_classmap_create(int device, uint32_t n_seq, uint32_t n_layers, gffx_hip_classmap **out);
int gffx_hip_classmap_add_rows_host(gffx_hip_classmap *, const uint32_t *rows /* 4 per row: layer, seqid, start, end */, uint64_t n_rows);
int gffx_hip_classmap_finish(gffx_hip_classmap *);
uint64_t gffx_hip_classmap_n_points(const gffx_hip_classmap *);
int gffx_hip_classmap_copy_points(gffx_hip_classmap *, uint64_t *p_off, uint32_t *pos, uint8_t *cls);
int gffx_hip_classmap_copy_bases(gffx_hip_classmap *, uint64_t *cb /* T x n_points */);
int gffx_hip_classmap_run_host(gffx_hip_classmap *, const uint32_t *regions /* 3 per region */, uint64_t nq);
int gffx_hip_classmap_run_store(gffx_hip_classmap *, const gffx_hip_regions *, int k, uint64_t first, uint64_t n_rows);
int gffx_hip_classmap_wait(gffx_hip_classmap *);
int gffx_hip_classmap_copy_counts(gffx_hip_classmap *, uint32_t *counts /* nq x (T + 1) */);
int gffx_hip_classmap_copy_class(gffx_hip_classmap *, uint8_t *cls /* nq */);
int gffx_hip_classmap_last_kernel_ms(gffx_hip_classmap *, double *ms);
int gffx_hip_classmap_stage_ms(const gffx_hip_classmap *, double *ms /* 6: union, toggles, sort, scan, points, bases */);
uint32_t gffx_hip_classmap_scan_tile(void);
uint32_t gffx_hip_classmap_carry_tiles(void); /* tiles per step of the three single-block carry walks */
uint32_t gffx_hip_classmap_block_size(void);
void gffx_hip_classmap_destroy(gffx_hip_classmap *);

/* ---- permutation totals on a finished class map (`gffx enrich`; device/enrich.hip, device/enrich_core.hpp) --
 * Regions (c, qs, qe) with a global row i (their place in the input), a length L[c] per seqid, n_perm permutations and a seed.
 * Row 0 of the totals is the observed data; in row p = 1 .. n_perm a region of width w = qe - qs <= L[c] lies at
 * [s', s' + w), s' = (r(p, i) * (L[c] - w + 1)) >> 64, r(p, i) = mix64(mix64(seed + GOLD * p) + GOLD * (i + 1)) with the
 * splitmix64 finalizer mix64 and GOLD = 0x9E3779B97F4A7C15 (a bias of at most 2^-32, not corrected).  A region with
 * qs >= qe is empty (class T, no bases); one with w > L[c] is unplaceable: it stays where it is and is counted in `unplaced`.
 * bases[p * (T + 1) + k] = the sum of bases_k over the regions, regions[p * (T + 1) + k] = the regions of class k.  Integer
 * sums: any split of the regions into runs gives the same totals.
 *   _perm_begin    allocates and zeroes the totals (a second call starts over; so does _finish of new rows, which drops them).
 *                  GFFX_E_STATE before _finish, GFFX_E_INVALID for n_perm > 2^20
 *   _perm_run_host, _perm_run_store   add regions to the totals, asynchronous on the object's stream; first_row = the global
 *                  row of the first region.  GFFX_E_STATE before _perm_begin.  _run_store reads the slot in place: _perm_wait
 *                  before the staging buffer is appended again.  A run with a row chr >= n_seq is void (it adds nothing):
 *   _perm_wait     waits for the runs; GFFX_E_CHR_RANGE once if a run since the last wait was void (the object stays usable)
 *   _perm_copy_totals   bases, regions: (n_perm + 1) x (T + 1) each, unplaced: one word (any may be NULL); after _perm_wait
 *   _perm_last_kernel_ms   HIP-event milliseconds of the runs the last _perm_wait waited for
 *   _perm_group    rows of the totals per block of k_classmap_permute (regions per block: _block_size) */
int gffx_hip_classmap_perm_begin(gffx_hip_classmap *, const uint32_t *seq_len /* n_seq */, uint32_t n_perm, uint64_t seed);
int gffx_hip_classmap_perm_run_host(gffx_hip_classmap *, const uint32_t *regions /* 3 per region */, uint64_t nq, uint64_t first_row);
int gffx_hip_classmap_perm_run_store(gffx_hip_classmap *, const gffx_hip_regions *, int k, uint64_t first, uint64_t n_rows, uint64_t first_row);
int gffx_hip_classmap_perm_wait(gffx_hip_classmap *);
int gffx_hip_classmap_perm_copy_totals(gffx_hip_classmap *, uint64_t *bases, uint64_t *regions, uint64_t *unplaced);
int gffx_hip_classmap_perm_last_kernel_ms(gffx_hip_classmap *, double *ms);
uint32_t gffx_hip_classmap_perm_group(void);

/* ---- BAM sources of `gffx depth` / `gffx coverage` (commands/depth.rs:297-427, commands/coverage.rs:125-204) --
 * BGZF members are inflated on the device (one wave per member, device/bgzf.hip; the decoder, device/bgzf_core.hpp, is
 * shared with the host).  A bad member fails the call with a message naming its file offset: a header that is not BGZF,
 * a truncated member, an invalid DEFLATE stream, an ISIZE or CRC32 mismatch.
 *
 * gffx_hip_bgzf_inflate: the members of bgzf[0, n_bytes) into out[0, *n_out).  out == NULL: *n_out = the decompressed
 * size (the sum of the ISIZEs), no device needed.
 *
 * gffx_hip_bam_*: the rows of a BAM file.  _create takes the header's size in the decompressed stream (the caller
 * decodes the header: magic, l_text, n_ref, names) and ref_seq[tid] = the index's seqid number of reference tid, or
 * UINT32_MAX when the index has no such seqid; chunk_bytes bounds the compressed bytes per device pass (0: 256 MiB).
 * _feed takes whole members in file order from byte 0, any number per call; _finish fails if the file ends inside
 * the header or inside a record.  Rows are (seqid, start, end), 3 x u32 each, in file order: a record is kept unless
 * flag & 0x4, refID < 0, ref_seq[refID] == UINT32_MAX or pos < 0 (depth.rs:335-364); start = pos, end = bam_endpos
 * clamped to UINT32_MAX.  ASSUMPTION (htslib's sam.c restated from memory): bam_endpos = pos + the summed lengths of the
 * CIGAR ops M/D/N/=/X, where a sum of 0 (no CIGAR, or only I/S/H/P) counts as 1.  A malformed record (block_size < 32,
 * l_read_name == 0, read name + CIGAR beyond block_size, refID outside [-1, n_ref)) fails the call, as bam_read1 does.
 * _counts: records framed, unmapped ones, mapped ones whose refID is < 0 or not in the index, rows kept.
 * _stage_ms: device time of the inflate, framing and rows kernels so far (HIP events).
 * After an error the object only reports it again. */
int gffx_hip_bgzf_inflate(int device, const uint8_t *bgzf, uint64_t n_bytes, uint8_t *out, uint64_t cap, uint64_t *n_out);
int gffx_hip_bam_create(int device, uint32_t n_ref, const uint32_t *ref_seq, uint64_t header_bytes, uint64_t chunk_bytes,
                        gffx_hip_bam **out);
int gffx_hip_bam_feed(gffx_hip_bam *, const uint8_t *bgzf, uint64_t n_bytes);
int gffx_hip_bam_finish(gffx_hip_bam *);
uint64_t gffx_hip_bam_rows(const gffx_hip_bam *);
int gffx_hip_bam_counts(const gffx_hip_bam *, uint64_t *records, uint64_t *unmapped, uint64_t *no_seq, uint64_t *kept);
int gffx_hip_bam_stage_ms(const gffx_hip_bam *, double *inflate_ms, double *frame_ms, double *rows_ms);
int gffx_hip_bam_copy_rows(gffx_hip_bam *, uint32_t *rows /* 3 per row */);
void gffx_hip_bam_destroy(gffx_hip_bam *);

/* ---- SAM sources of `gffx depth` / `gffx coverage` (commands/depth.rs:588-591, commands/coverage.rs:520-541: the ----
 * reference reads .sam through the reader it uses for .bam).  The text is cut into lines, the lines into fields, and
 * FLAG, RNAME, POS and CIGAR are read on the device (device/sam.hip; the rules of one line, device/sam_core.hpp, are
 * shared with the host).  The text is plain, or BGZF-compressed (bgzf != 0): then its members are inflated on the
 * device as for BAM and the inflated bytes never leave it.
 *
 * _create takes the references of the header's @SQ lines in order (the order defines the tid): reference i's name is
 * names[name_off[i], name_off[i + 1]) (no terminator), ref_seq[i] = the index's seqid number of it, or UINT32_MAX when
 * the index has no such seqid (as for gffx_hip_bam_create); a name that occurs twice fails the call, as htslib's header
 * parser does.  header_bytes = the offset, in the (inflated) text, of the first line that does not begin with '@'; the
 * caller finds it and the names.  chunk_bytes bounds the fed bytes per device pass (0: 64 MiB).
 * _feed takes the stream in file order from byte 0: text in pieces of any size, cut anywhere; BGZF in whole members.
 * _finish reads a last line that does not end in '\n'.
 * Rows are (seqid, start, end), 3 x u32 each, in file order.  A line needs 11 TAB-separated fields; of them FLAG (decimal,
 * <= 65535, no leading zero, no 0x), RNAME, POS (1 to 18 decimal digits) and CIGAR (`*`, or <length><op> with op in
 * MIDNSHP=XB and length < 2^28) are read, anything else in them fails the call with a message "line <n>: <reason>",
 * n counted from 1 over the whole file, header lines included, and always the first such line of the file.  DEVIATION:
 * fields 5 and 7 to 11 and the tags are not validated (htslib rejects e.g. a SEQ whose length differs from the CIGAR's).
 * A line is kept unless flag & 0x4, CIGAR is `*`, RNAME is `*` or names no reference, ref_seq of it is UINT32_MAX, or
 * POS is 0; start = POS - 1, end = start + the summed lengths of M/D/N/=/X (a sum of 0 counts as 1), both clamped to
 * UINT32_MAX.  ASSUMPTION (htslib's sam.c sam_parse1 restated from memory): (1) a line without flag 0x4 whose CIGAR is
 * `*` is treated as unmapped ("mapped query must have a CIGAR"); (2) a CIGAR length of 2^28 or more is an error; (3) an
 * RNAME without @SQ line gets a warning and tid -1, so the line is dropped.
 * _counts: lines read (header lines not counted), unmapped ones (flag 0x4 or `*` CIGAR), mapped ones without a seqid of
 * the index, rows kept.  _stage_ms: device time of the inflate (plain text: the copy behind the unfinished line), the
 * line scan and the rows kernels so far (HIP events).  After an error the object only reports it again. */
int gffx_hip_sam_create(int device, uint32_t n_ref, const char *names /* concatenated */, const uint64_t *name_off /* n_ref + 1 */,
                        const uint32_t *ref_seq, uint64_t header_bytes, uint64_t chunk_bytes, int bgzf, gffx_hip_sam **out);
int gffx_hip_sam_feed(gffx_hip_sam *, const uint8_t *bytes, uint64_t n_bytes); /* bgzf: whole members; text: any split */
int gffx_hip_sam_finish(gffx_hip_sam *);
uint64_t gffx_hip_sam_rows(const gffx_hip_sam *);
int gffx_hip_sam_counts(const gffx_hip_sam *, uint64_t *lines, uint64_t *unmapped, uint64_t *no_seq, uint64_t *kept);
int gffx_hip_sam_stage_ms(const gffx_hip_sam *, double *inflate_ms, double *lines_ms, double *rows_ms);
int gffx_hip_sam_copy_rows(gffx_hip_sam *, uint32_t *rows /* 3 per row */);
void gffx_hip_sam_destroy(gffx_hip_sam *);

/* ---- BED sources of `gffx intersect -b`, `gffx depth -s` and `gffx coverage -s`: the text is cut into lines, the lines ----
 * into fields, the two coordinates are read and the name is looked up on the device (device/bed.hip; the rules of one line,
 * device/bed_core.hpp, are shared with the host).  The text is plain, or BGZF-compressed (bgzf != 0): then its members are
 * inflated on the device as for BAM and the inflated bytes never leave it.
 *
 * _create takes the index's seqids in order: seqid number i's name is names[name_off[i], name_off[i + 1]) (no terminator);
 * a name that occurs twice fails the call.  chunk_bytes bounds the fed bytes per device pass (0: 64 MiB).  dialect names
 * the host parser whose rules hold, checked in this order:
 *   GFFX_BED_INTERSECT (commands/intersect.rs:201-230): lines are the pieces between '\n'.  Empty or first byte '#':
 *     skipped.  The whole line not valid UTF-8 (overlong forms, surrogates and > U+10FFFF are invalid): ERROR "invalid
 *     utf-8 sequence in BED line".  Fields split on space, \t, \x0C, \r (not \x0B); fewer than three: skipped.  A name
 *     the table does not have: no_seq -- before the coordinates are looked at.  A coordinate is an optional '+', at least
 *     one digit, the whole field, <= 4294967295; else ERROR `lexical parse error: invalid BED coordinate in "<the line>"`.
 *     Rows with start >= end are kept.
 *   GFFX_BED_DEPTH (commands/depth.rs:450-495, commands/coverage.rs:230-256): the line includes its '\n'.  Empty or '#':
 *     skipped.  Fields split on \t and space only; fewer than three: skipped.  One of the three fields not valid UTF-8:
 *     skipped.  Field 2 by the same number rule, field 3 the same after its trailing Unicode White_Space is cut; not a
 *     number, or start >= end: skipped.  A name the table does not have: no_seq.  Nothing is an error.
 * _feed takes the stream in file order from byte 0: text in pieces of any size, cut anywhere; BGZF in whole members.
 * _finish reads a last line that does not end in '\n'.
 * Rows are (seqid, start, end), 3 x u32 each, in file order.  An ERROR fails the call with GFFX_E_INVALID and exactly the
 * message above, always for the first such line of the file; after it every call on the object, _copy_rows included,
 * returns the same code and message.
 * _counts: lines read, lines skipped, lines whose name the table does not have, rows kept; each line is tallied once, by
 * the first rule of its dialect that decides it, so lines == skipped + no_seq + kept on a run without error.
 * _stage_ms: device time of the inflate (plain text: the copy behind the unfinished line), the line scan and the rows
 * kernels so far (HIP events). */
#define GFFX_BED_INTERSECT 0
#define GFFX_BED_DEPTH 1
int gffx_hip_bed_create(int device, uint32_t n_seq, const char *names /* concatenated */, const uint64_t *name_off /* n_seq + 1 */,
                        int dialect, uint64_t chunk_bytes, int bgzf, gffx_hip_bed **out);
int gffx_hip_bed_feed(gffx_hip_bed *, const uint8_t *bytes, uint64_t n_bytes); /* bgzf: whole members; text: any split */
int gffx_hip_bed_finish(gffx_hip_bed *);
uint64_t gffx_hip_bed_rows(const gffx_hip_bed *);
int gffx_hip_bed_counts(const gffx_hip_bed *, uint64_t *lines, uint64_t *skipped, uint64_t *no_seq, uint64_t *kept);
int gffx_hip_bed_stage_ms(const gffx_hip_bed *, double *inflate_ms, double *lines_ms, double *rows_ms);
int gffx_hip_bed_copy_rows(gffx_hip_bed *, uint32_t *rows /* 3 per row */);
void gffx_hip_bed_destroy(gffx_hip_bed *);

/* ---- `gffx extract`: feature-ID lookup, parent chase and the per-line ID filter (commands/extract.rs:37-162, ------------
 * index_loader/fts.rs:16-31, index_loader/prt.rs:54-72, utils/common.rs:289-465; device/ids.hip, the rules of one name,
 * one chase and one line in device/ids_core.hpp, shared with the host).
 *
 * _create builds the ID table on the device from the `.fts` strings -- name f is names[name_off[f], name_off[f + 1]) (no
 * terminator), f = its line number = its fid -- and keeps the `.prt` words (prt[f] = the parent of f).  A name's fid is the
 * LAST line that holds the string (fts.rs:16-22).  hash_bits < 0 or 32: the whole 32-bit hash; 0 to 31: only its low bits
 * (a test hook: it forces the names onto few probe chains; results never depend on it); _options reports a non-default
 * value as {"hash_bits": k}.  _n: the number of names.
 * _resolve: per query name (bytes + offsets, as for _create) fid_out = its fid and root_out = the root the parent chase
 * ends at (prt.rs:54-72: cur >= n_prt invalid; prt[cur] == cur the root; prt[cur] >= n_prt invalid), UINT32_MAX for a name
 * that is not in the table / a fid without a valid root.  DEVIATION: a parent cycle that no root closes never ends in the
 * reference; here the chase ends after n_prt steps and the fid is invalid.  Every found fid sets a bit of the requested
 * bitmap, every valid root a bit of the root bitmap; both accumulate over calls until _reset.  _copy_*_bitmap: bit i of
 * word i / 64, ceil(max(n_names, n_prt) / 64) words (n_words must be at least that).
 * _filter_lines: text[0, n_bytes) holds n_lines whole lines back to back, line i = text[line_off[i], line_off[i + 1]) with its
 * line ending (the last one may have none), line_root[i] = the root fid of the block the line lies in.  keep_out[i] = 1 iff
 * write_gff_output_filtered keeps the line for the key "ID" (common.rs:418-431): its first byte is not '#'; with a type
 * filter (by_type != 0; the n_types allowed strings already split at ',', trimmed and the empty ones dropped; none allowed
 * keeps nothing) it has three TABs and column 3 is allowed; it has eight TABs, and the value after the first "ID=" behind
 * the eighth TAB, up to the next ';' or the end of the line less a final "\n" and then "\r", is a name of the table whose
 * fid was requested (in a _resolve since the last _reset) and whose root is line_root[i].
 * _stage_ms: HIP-event milliseconds of the table build, the resolve and the filter kernels so far. */
typedef struct gffx_hip_ids gffx_hip_ids;
int gffx_hip_ids_create(int device, uint64_t n_names, const uint8_t *names /* concatenated */, const uint64_t *name_off /* n_names + 1 */,
                        uint64_t n_prt, const uint32_t *prt, int hash_bits, gffx_hip_ids **out);
void gffx_hip_ids_destroy(gffx_hip_ids *);
uint64_t gffx_hip_ids_n(const gffx_hip_ids *);
int gffx_hip_ids_options(const gffx_hip_ids *, char *buf, size_t cap);
int gffx_hip_ids_resolve(gffx_hip_ids *, uint64_t n_queries, const uint8_t *names, const uint64_t *name_off /* n_queries + 1 */,
                         uint32_t *fid_out, uint32_t *root_out);
int gffx_hip_ids_reset(gffx_hip_ids *);
int gffx_hip_ids_copy_root_bitmap(gffx_hip_ids *, uint64_t *host, uint64_t n_words);
int gffx_hip_ids_copy_requested_bitmap(gffx_hip_ids *, uint64_t *host, uint64_t n_words);
int gffx_hip_ids_filter_lines(gffx_hip_ids *, const uint8_t *text, uint64_t n_bytes, uint64_t n_lines, const uint64_t *line_off /* n_lines + 1 */,
                              const uint32_t *line_root, int by_type, uint32_t n_types, const uint8_t *types /* concatenated */,
                              const uint32_t *type_off /* n_types + 1 */, uint8_t *keep_out);
int gffx_hip_ids_stage_ms(const gffx_hip_ids *, double *build_ms, double *resolve_ms, double *filter_ms);

/* ---- `gffx search`: attribute-value and regex lookup, fid / root resolution and the per-line value filter ---------------
 * (commands/search.rs:55-252, index_loader/core.rs:37-89, index_loader/a2f.rs:77-113, index_loader/prt.rs:54-72,
 * utils/common.rs:289-465; device/search.hip, the rules of one value, one chase and one line in device/search_core.hpp and
 * device/ids_core.hpp, shared with the host).
 *
 * _create keeps the `.atn` values -- value a is values[value_off[a], value_off[a + 1]) (no terminator), a = its position in
 * the loaded list = its aid --, the `.a2f` words (a2f[f] = the aid of fid f, UINT32_MAX: none), the `.prt` words and the
 * attribute name key[0, key_len) (without '='), and builds on the device a string table over the values and the class of
 * every aid: the largest aid with the same string.  hash_bits as for gffx_hip_ids_create (a test hook for both the value
 * table and the table of wanted strings).  dfa_path: 0 = k_attr_match_dfa stages its tables in LDS when they fit 64 KiB
 * and reads them from global memory otherwise; 1 = LDS (tables that do not fit fail the call); 2 = global (a test hook).
 * _options reports non-default values as {"hash_bits": k, "dfa_path": "lds" | "global"}.  _n: the number of values.
 * _match_exact: every aid whose value equals one of the n_wanted strings (bytes + offsets, as for _create) gets its bit in
 * the matched bitmap (search.rs:105-110: every duplicate of a wanted string matches).
 * _match_dfa: every aid whose value the DFA accepts gets its bit.  The DFA is host/regex_dfa.cpp's: cls[256] maps a byte to a
 * column < n_classes - 1, the last column is the end of the text, trans[s * n_classes + c] < n_states, state 0 accepts and
 * is absorbing, the walk starts in init; tables that break these bounds fail the call.  Values are valid UTF-8 from the
 * loader; on other bytes the answer is unspecified, the walk is bounded all the same.  _dfa_kernel names the form the last
 * _match_dfa took: "k_attr_match_dfa<lds>" or "k_attr_match_dfa<global>".
 * Matches accumulate (OR) over calls until _reset, which clears all four bitmaps and the pair set.
 * _resolve: from the matched bitmap as it stands, per fid f with a matched aid: bit f of the fid bitmap; the root of f
 * (prt.rs:54-72; DEVIATION as for gffx_hip_ids_resolve: the chase ends after n_prt steps) sets a bit of the root bitmap, or
 * f a bit of the invalid bitmap; (class of the aid, root) enters the pair set.  Each call starts from empty results.
 * _copy_matched_bitmap: ceil(n_values / 64) words; the other three: ceil(max(n_a2f, n_prt) / 64) words; bit i of word i / 64.
 * _filter_lines: as gffx_hip_ids_filter_lines, with this test of the value: the bytes after the first "<key>=" behind the
 * eighth TAB, up to the next ';' or the end of the line, are a string of `.atn` whose class forms a pair with line_root[i]
 * -- that is: some fid whose root is line_root[i] carries a matched value with exactly these bytes (search.rs:209-218).
 * _stage_ms: HIP-event milliseconds of the table build, the match, the resolve and the filter kernels so far. */
typedef struct gffx_hip_attrs gffx_hip_attrs;
int gffx_hip_attrs_create(int device, uint64_t n_values, const uint8_t *values /* concatenated */, const uint64_t *value_off /* n_values + 1 */,
                          uint64_t n_a2f, const uint32_t *a2f, uint64_t n_prt, const uint32_t *prt, const uint8_t *key, uint32_t key_len,
                          int hash_bits, int dfa_path, gffx_hip_attrs **out);
void gffx_hip_attrs_destroy(gffx_hip_attrs *);
uint64_t gffx_hip_attrs_n(const gffx_hip_attrs *);
int gffx_hip_attrs_options(const gffx_hip_attrs *, char *buf, size_t cap);
int gffx_hip_attrs_match_exact(gffx_hip_attrs *, uint64_t n_wanted, const uint8_t *wanted, const uint64_t *wanted_off /* n_wanted + 1 */);
int gffx_hip_attrs_match_dfa(gffx_hip_attrs *, uint32_t n_states, uint32_t n_classes, uint32_t init, const uint8_t *cls /* 256 */,
                             const uint16_t *trans /* n_states x n_classes */);
const char *gffx_hip_attrs_dfa_kernel(const gffx_hip_attrs *);
int gffx_hip_attrs_reset(gffx_hip_attrs *);
int gffx_hip_attrs_resolve(gffx_hip_attrs *);
int gffx_hip_attrs_copy_matched_bitmap(gffx_hip_attrs *, uint64_t *host, uint64_t n_words);
int gffx_hip_attrs_copy_fid_bitmap(gffx_hip_attrs *, uint64_t *host, uint64_t n_words);
int gffx_hip_attrs_copy_root_bitmap(gffx_hip_attrs *, uint64_t *host, uint64_t n_words);
int gffx_hip_attrs_copy_invalid_bitmap(gffx_hip_attrs *, uint64_t *host, uint64_t n_words);
int gffx_hip_attrs_filter_lines(gffx_hip_attrs *, const uint8_t *text, uint64_t n_bytes, uint64_t n_lines, const uint64_t *line_off /* n_lines + 1 */,
                                const uint32_t *line_root, int by_type, uint32_t n_types, const uint8_t *types /* concatenated */,
                                const uint32_t *type_off /* n_types + 1 */, uint8_t *keep_out);
int gffx_hip_attrs_stage_ms(const gffx_hip_attrs *, double *build_ms, double *match_ms, double *resolve_ms, double *filter_ms);

/* ---- `gffx index --gpu`: the GFF3 text to the arrays of the side-cars .fts .prt .a2f .atn .sqs .gof and the root list of ----
 * .rit / .rix (index_builder/core.rs:41-242; device/gff.hip, the rules of one line in device/gff_core.hpp, shared with
 * the host).  The bytes are what host/index_builder.cpp writes for the same text.
 *
 * _create takes the attribute key (a C string, without '=') and the skip strings of --skip-types already split at ','
 * (string k = skip[skip_off[k], skip_off[k + 1]), not trimmed, an empty one a member like any other).  chunk_bytes bounds the
 * fed bytes per device pass (0: 64 MiB; at most 1 GiB).  hash_bits as for gffx_hip_ids_create (a test hook).
 * _feed takes the text in file order from byte 0, in pieces of any size, cut anywhere; the unfinished line is carried into
 * the next pass.  _finish reads a last line that does not end in '\n' and runs the steps that need the whole file.
 * One line, without its '\n', in this order: empty or first byte '#' (before any trimming): skipped.  Not valid UTF-8: error
 * 4 BAD_UTF8.  Unicode White_Space (U+0009-000D, 0020, 0085, 00A0, 1680, 2000-200A, 2028, 2029, 202F, 205F, 3000) trimmed at
 * both ends; empty then: skipped.  Not exactly 9 TAB-separated fields: error 5 COLUMNS.  Column 3 equal to a skip string:
 * skipped by type.  Columns 4 / 5 not an optional '+' and decimal digits <= 2^32 - 1: error 6 DIGITS.  end == 0: skipped;
 * start > end swapped; the row is [start ? start - 1 : 0, end).  ID = the leftmost match of ID=([^;\s]+) over the whole
 * trimmed line (\s: the White_Space set; an empty value makes the search go on: `ID=;ID=z` yields z, `geneID=x;ID=y`
 * yields x); none: error 7 NO_ID.  Parent: the same with `Parent`, optional.  The attribute value: the leftmost match of
 * <key>=([^;]+); a value that holds ' ' or ',' flags the row (the [WARN] line of the command).
 * The first bad line of the file and the first failing check on it fail the call (whatever the chunking); _error reports
 * its file offset and kind (0: none).  After an error the object only reports it again and copies nothing out.
 * Over the whole file: a row's number is its `.fts` line; fid[row] = the LAST row with the row's ID (an earlier duplicate's
 * fid is not its own row); prt[row] = the fid of its Parent where it has one and that string is some row's ID (a comma
 * list names none), else fid[row]; a row is a root iff prt == fid.  Seqids are numbered by their first appearance as column
 * 1 of a ROOT row, attribute values by their first appearance on any row; a2f[row] = the value's number, UINT32_MAX: none.
 * _counts: lines read; empty, comment and white-space-only lines; lines skipped by type; lines with end == 0; rows; roots;
 * distinct seqids; distinct attribute values (the last three after _finish).
 * After _finish, each with its size query: _copy_fts (the IDs, a '\n' after each: the `.fts` file; _fts_bytes), _copy_fid /
 * _copy_prt / _copy_a2f (a word per row; _n_rows), _copy_atn / _copy_seqids (the names in number order, a '\n' after each;
 * _atn_bytes / _seqids_bytes), _copy_gof (24 bytes per root in file order: fid u32, seqid u32, the root's line offset u64,
 * the next root's -- the fed byte count for the last -- u64, little-endian: the `.gof` file; _n_roots), _copy_roots
 * (start, end, fid, seqid per root, in file order; _n_roots), _copy_skipped_lines (file offsets of the lines skipped by type;
 * _n_skipped_lines), _copy_warn_rows (the flagged rows; _n_warn_rows).
 * _stage_ms: HIP-event milliseconds of the line scan, the rows kernels, the ID table's build, the resolve and the numbering
 * (with the root list) so far.
 * LIMITS: more than 2^30 rows fail the call; a pass with its carry has no 4 GiB bound (line ends are 64-bit, the text
 * buffer grows with a line longer than a pass), but the strings of one kind of the lines that END within one 4 KiB tile of
 * a pass must total less than 4 GiB.  DEVIATION: none in what is computed; the passes run one after the other (no
 * double-buffered staging as in the BAM / SAM readers). */
typedef struct gffx_hip_gff gffx_hip_gff;
int gffx_hip_gff_create(int device, const char *attr_key, uint32_t n_skip, const char *skip /* concatenated */,
                        const uint32_t *skip_off /* n_skip + 1 */, uint64_t chunk_bytes, int hash_bits, gffx_hip_gff **out);
int gffx_hip_gff_feed(gffx_hip_gff *, const uint8_t *bytes, uint64_t n_bytes);
int gffx_hip_gff_finish(gffx_hip_gff *);
int gffx_hip_gff_error(const gffx_hip_gff *, uint64_t *line_offset, int *kind);
int gffx_hip_gff_counts(const gffx_hip_gff *, uint64_t *lines, uint64_t *blank, uint64_t *skipped_type, uint64_t *zero_end, uint64_t *rows,
                        uint64_t *roots, uint64_t *seqids, uint64_t *attr_values);
int gffx_hip_gff_stage_ms(const gffx_hip_gff *, double *scan_ms, double *rows_ms, double *table_ms, double *resolve_ms, double *number_ms);
uint64_t gffx_hip_gff_n_rows(const gffx_hip_gff *);
uint64_t gffx_hip_gff_n_roots(const gffx_hip_gff *);
uint64_t gffx_hip_gff_fts_bytes(const gffx_hip_gff *);
uint64_t gffx_hip_gff_atn_bytes(const gffx_hip_gff *);
uint64_t gffx_hip_gff_seqids_bytes(const gffx_hip_gff *);
uint64_t gffx_hip_gff_n_skipped_lines(const gffx_hip_gff *);
uint64_t gffx_hip_gff_n_warn_rows(const gffx_hip_gff *);
int gffx_hip_gff_copy_fts(const gffx_hip_gff *, uint8_t *out);
int gffx_hip_gff_copy_fid(const gffx_hip_gff *, uint32_t *out);
int gffx_hip_gff_copy_prt(const gffx_hip_gff *, uint32_t *out);
int gffx_hip_gff_copy_a2f(const gffx_hip_gff *, uint32_t *out);
int gffx_hip_gff_copy_atn(const gffx_hip_gff *, uint8_t *out);
int gffx_hip_gff_copy_seqids(const gffx_hip_gff *, uint8_t *out);
int gffx_hip_gff_copy_gof(const gffx_hip_gff *, uint8_t *out);
int gffx_hip_gff_copy_roots(const gffx_hip_gff *, uint32_t *out /* 4 per root */);
int gffx_hip_gff_copy_skipped_lines(const gffx_hip_gff *, uint64_t *out);
int gffx_hip_gff_copy_warn_rows(const gffx_hip_gff *, uint32_t *out);
void gffx_hip_gff_destroy(gffx_hip_gff *);

/* ---- Genome: a plain FASTA text packed into one arena of bases on the device (`gffx seq`; device/genome.hip) ----------------
 * The rule of a line is device/seq_core.hpp's: a line ends at '\n', a '\r' directly before it is not part of it; empty lines
 * are ignored; '>' opens a sequence named up to the first blank or TAB; every other line adds all of its bytes, as they are.
 *   _create    chunk_bytes: the text per device pass (0: 64 MiB; at most 1 GiB)
 *   _reserve   optional: room for n_bytes of bases at once (the arena otherwise grows as the text arrives)
 *   _feed      the next bytes of the text, cut ANYWHERE: inside a header, inside "\r\n", before a last line without '\n'
 *   _finish    the text is complete; the tables below are GFFX_E_STATE before it
 * ERRORS (GFFX_E_INVALID, the message names the line, the object keeps the failure): a non-empty line before the first '>', a
 * '>' line without a name, a name given twice, a sequence of 2^32 bases or more (GFF coordinates are 32-bit).  The arena itself
 * has 64-bit offsets: a genome may exceed 4 GiB.
 *   _copy_names  the names concatenated and their n_seq + 1 offsets; _copy_seqs: per sequence where it begins in the arena
 *                (n_seq + 1 offsets, the last one the base total) and its length; _copy_bases: bases [at, at + n) of the arena
 *   _stage_ms    HIP-event milliseconds of the line scan and of classify + prefix sums + copy, so far
 * gffx_hip_scan64_tile / _carry_tiles: the values per block of the 64-bit prefix sum behind the genome, the seq plan and the
 * effect build (device/scan64.hpp), and the tile sums its single carry block takes per step */
typedef struct gffx_hip_genome gffx_hip_genome;
int gffx_hip_genome_create(int device, uint64_t chunk_bytes, gffx_hip_genome **out);
int gffx_hip_genome_reserve(gffx_hip_genome *, uint64_t n_bytes);
int gffx_hip_genome_feed(gffx_hip_genome *, const uint8_t *bytes, uint64_t n_bytes);
int gffx_hip_genome_finish(gffx_hip_genome *);
int gffx_hip_genome_device(const gffx_hip_genome *);
uint32_t gffx_hip_genome_n_seq(const gffx_hip_genome *);
uint64_t gffx_hip_genome_n_bases(const gffx_hip_genome *);
uint64_t gffx_hip_genome_name_bytes(const gffx_hip_genome *);
int gffx_hip_genome_copy_names(const gffx_hip_genome *, uint8_t *names, uint64_t *name_off /* n_seq + 1 */);
int gffx_hip_genome_copy_seqs(const gffx_hip_genome *, uint64_t *offset /* n_seq + 1 */, uint32_t *length /* n_seq */);
int gffx_hip_genome_copy_bases(const gffx_hip_genome *, uint64_t at, uint64_t n, uint8_t *out);
int gffx_hip_genome_stage_ms(const gffx_hip_genome *, double *lines_ms, double *pack_ms);
void gffx_hip_genome_destroy(gffx_hip_genome *);
uint32_t gffx_hip_scan64_tile(void);
uint32_t gffx_hip_scan64_carry_tiles(void);

/* ---- Seq: feature and spliced sequences of a genome, wrapped FASTA bodies (`gffx seq`; device/seq.hip, seq_core.hpp) ----------
 * rows: (record, sequence number of the genome, start - 1, end) per segment, start - 1 < end, any order; a sequence number
 * >= n_seq stands for a sequence the FASTA lacks.  Every record 0 .. n_records - 1 has at least one row.  rec_flags[r]:
 * GFFX_SEQ_MINUS | phase << 1 (0 .. 2: bases skipped before the first codon with `translate`) | GFFX_SEQ_DROPPED (dropped by
 * the caller).  A record's segments are ordered by (start, input order) and concatenated; a minus record is the reverse
 * complement of that; a record with a member the genome cannot serve is dropped.  The body of a record is its characters in
 * lines of `width` (0: one line), each ended by '\n'; a dropped record has none.
 *   _create        the plan: sort, lengths, drops, body sizes and their 64-bit prefix sums (waits for them)
 *   _copy_offsets  body_off[n_records + 1] into the concatenation of all bodies, dropped[n_records]
 *   _emit_start    bytes [at, at + n) of that concatenation into slot 0 or 1 (any cut: inside a record, a line, before a
 *                  newline), enqueued; _emit_wait: the slot's bytes in pinned host memory, valid until the slot's next start
 *   _tile          the output bytes per block of the emit kernel
 *   _stage_ms      HIP-event milliseconds of the plan and of the emit kernels so far
 * The genome must outlive the object. */
enum { GFFX_SEQ_MINUS = 1, GFFX_SEQ_DROPPED = 8 };
typedef struct gffx_hip_seq gffx_hip_seq;
uint32_t gffx_hip_seq_tile(void);
int gffx_hip_seq_create(const gffx_hip_genome *, uint64_t n_rows, const uint32_t *rows /* 4 per row */, uint64_t n_records,
                        const uint8_t *rec_flags, int translate, uint32_t width, gffx_hip_seq **out);
uint64_t gffx_hip_seq_body_bytes(const gffx_hip_seq *);
int gffx_hip_seq_copy_offsets(const gffx_hip_seq *, uint64_t *body_off /* n_records + 1 */, uint8_t *dropped /* n_records */);
int gffx_hip_seq_emit_start(gffx_hip_seq *, int slot, uint64_t at, uint64_t n);
int gffx_hip_seq_emit_wait(gffx_hip_seq *, int slot, const uint8_t **bytes);
int gffx_hip_seq_stage_ms(const gffx_hip_seq *, double *plan_ms, double *emit_ms);
void gffx_hip_seq_destroy(gffx_hip_seq *);

/* ---- Effect: what a single-base substitution does to every transcript it hits (`gffx effect`; device/effect.hip, the rules:
 * effect_core.hpp) ----
 * rows: (transcript, sequence number of the genome, start - 1, end, kind) per member line, kind 0 a CDS line and 1 an exon line,
 * start - 1 < end, any order; a sequence number >= n_seq stands for a sequence the FASTA lacks.  Every transcript
 * 0 .. n_transcripts - 1 has at least one row.  tr_flags[t]: GFFX_SEQ_MINUS | phase of the leading CDS segment << 1 |
 * GFFX_SEQ_DROPPED (dropped by the caller), as for gffx_hip_seq.  A transcript whose members lie on more than one sequence, on a
 * sequence the genome lacks or beyond its end is dropped; the others are KEPT.  The span of a transcript is [smallest start,
 * largest end] over all its members.
 * alleles: (sequence number, x, REF | ALT << 8) per row, x 1-based; sequence number UINT32_MAX: a sequence the FASTA lacks (no
 * pair, ref_match 0).  Any other number >= n_seq, or x = 0, fails the run with GFFX_E_CHR_RANGE, and the failure sticks.
 * A chunk's result is a CSR: offsets[n + 1] (u64) over the pairs (allele, kept transcript whose span contains x), the alleles
 * in input order and an allele's transcripts by number; per pair one 32-byte record
 *     u64 q (cds_pos - 1), u64 c (aa_pos - 1), u32 transcript, u8 class, k, ref_match, aa_ref, aa_alt, codon_ref[3],
 *     codon_alt[3], pad                                  (class: enum gffx_effect_class; the unused fields of a class are 0)
 * and per allele ref_match[n] (u8): REF, case folded, is the genome's base at x.
 *   _create           sorts the rows and builds the transcripts on the device, then a private interval index over the kept
 *                     spans (waits for it); max_alleles: the largest chunk
 *   _copy_transcripts dropped[n_transcripts], span[2 * n_transcripts] (first and last base, 1-based); either may be NULL
 *   _run_start        a chunk into slot 0 or 1: the pair CSR from the engine's direct pass (waited for: the caller's rows are
 *                     free on return; the pair buffer grows and the pass replays as for a batch), then the classify kernel and
 *                     the copies, enqueued; _run_wait: the slot's results in pinned host memory, valid until its next start
 *   _stage_ms         HIP-event milliseconds of the build, the pair passes and the classify kernel so far
 *   _stats            kept transcripts; how often a slot's record buffer had to grow
 * INDELS (`gffx effect --indels`): _run_any_start takes rows of 6 words (sequence number, x0, d, m, offset low, offset high) and
 * a byte arena; a row's d reference bases R' (from x0 on, 1-based) and its m alternate bytes A' stand at arena[offset,
 * offset + d + m), trimmed by the caller so that they share no first and no last base.  Its footprint is [x0, x0 + d - 1], for
 * d = 0 the flanking bases [x0 - 1, x0]; it pairs with every kept transcript whose span meets the footprint, provided the
 * footprint lies inside the sequence.  ref_match: R', case folded, is the genome's (1 for d = 0).  A row with d = m = 1 gives
 * the record of _run_start; every other row one of the classes 0 .. 19 with q, c and k where the coding rule was reached and
 * the codon and amino-acid bytes 0.  A bad sequence number, x0 = 0, d = m = 0, d or m above 65535 or d = 0 with x0 = 1 fails
 * with GFFX_E_CHR_RANGE; a row whose bytes leave the arena with GFFX_E_INVALID; both stick.  _run_wait serves both starts.
 *   _arena_grows      how often a slot's pinned arena staging had to grow
 * The genome must outlive the object. */
enum gffx_effect_class {
    GFFX_EFFECT_PARTIAL_CODON = 0, GFFX_EFFECT_CODING_UNKNOWN = 1, GFFX_EFFECT_STOP_RETAINED = 2, GFFX_EFFECT_SYNONYMOUS = 3,
    GFFX_EFFECT_STOP_GAINED = 4, GFFX_EFFECT_STOP_LOST = 5, GFFX_EFFECT_START_LOST = 6, GFFX_EFFECT_MISSENSE = 7,
    GFFX_EFFECT_NONCODING_EXON = 8, GFFX_EFFECT_5_PRIME_UTR = 9, GFFX_EFFECT_3_PRIME_UTR = 10, GFFX_EFFECT_INTRON = 11,
    GFFX_EFFECT_SPLICE_DONOR = 12, GFFX_EFFECT_SPLICE_ACCEPTOR = 13, GFFX_EFFECT_INTERGENIC = 14,
    /* _run_any_start only */
    GFFX_EFFECT_FRAMESHIFT = 15, GFFX_EFFECT_INFRAME_INSERTION = 16, GFFX_EFFECT_INFRAME_DELETION = 17,
    GFFX_EFFECT_TRANSCRIPT_ABLATION = 18, GFFX_EFFECT_UNCLASSIFIED_MODEL = 19
};
typedef struct gffx_hip_effect gffx_hip_effect;
uint32_t gffx_hip_effect_record_bytes(void);
int gffx_hip_effect_create(const gffx_hip_genome *, uint64_t n_rows, const uint32_t *rows /* 5 per row */, uint64_t n_transcripts,
                           const uint8_t *tr_flags, uint64_t max_alleles, gffx_hip_effect **out);
int gffx_hip_effect_copy_transcripts(const gffx_hip_effect *, uint8_t *dropped /* n_transcripts */, uint32_t *span /* 2 per transcript */);
int gffx_hip_effect_run_start(gffx_hip_effect *, int slot, const uint32_t *alleles /* 3 per row */, uint64_t n);
int gffx_hip_effect_run_any_start(gffx_hip_effect *, int slot, const uint32_t *rows /* 6 per row */, uint64_t n, const uint8_t *arena,
                                  uint64_t arena_bytes);
int gffx_hip_effect_run_wait(gffx_hip_effect *, int slot, const uint64_t **offsets, const uint8_t **ref_match, const uint8_t **records,
                             uint64_t *n_pairs);
int gffx_hip_effect_stage_ms(const gffx_hip_effect *, double *build_ms, double *pairs_ms, double *classify_ms);
int gffx_hip_effect_stats(const gffx_hip_effect *, uint64_t *kept, uint64_t *grows);
int gffx_hip_effect_arena_grows(const gffx_hip_effect *, uint64_t *grows);
void gffx_hip_effect_destroy(gffx_hip_effect *);

#ifdef __cplusplus
}
#endif
#endif /* GFFX_HIP_H */
