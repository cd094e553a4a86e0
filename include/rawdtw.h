/*
 * rawdtw.h -- C ABI of the MI355X-native DTW alignment engine (librawdtw.so).
 *
 * This is the drop-in boundary for RawAlign's DTW hot path.  The reference has
 * no plugin API; its boundary is the C++ free-function interface of
 * src/dtw.hpp:21-29, called from exactly one place, align_chain
 * (src/rmap.cpp:211,215,221,273,277,284).  Each entry point below names the
 * reference interface it replaces.  Plain pointers and sizes only; every
 * function returns a status code (no exceptions cross the ABI, no abort()).
 *
 * Threading: a rawdtw_ctx owns one HIP stream and is NOT re-entrant; use one
 * ctx per host thread (or serialise).  Different ctxs are independent.
 *
 * Arithmetic contract: fp32, local distance |x-y|, cell = min3 + dist; device
 * code is built with -ffp-contract=off and flushes nothing.  Costs, paths and
 * scores are bit-identical to the reference for finite inputs whose sums stay
 * finite (NaN or infinite inputs, and sums that overflow: unspecified).
 *  - The banded functions (DTW_global_slantedbanded_antidiagonalwise,
 *    dtw.cpp:273-520) read every absent neighbour -- guarded, clipped or outside
 *    the band -- as float(1e10), as the reference does: it is an operand of the
 *    min like any other, and costs may exceed it (it then wins the min, there
 *    as here).
 *  - The full-matrix functions (DTW_global, DTW_global_tb: dtw.cpp:37-66,
 *    595-667) have no sentinel: row 0 and column 0 are running sums, whatever
 *    they pass.
 *  - The semiglobal functions (DTW_semiglobal, DTW_semiglobal_slow,
 *    DTW_semiglobal_tb: dtw.cpp:526-593, 669-753) run the sentinel-free
 *    recurrence of _slow and _tb: row 0 is ASSIGNED the distance, column 0 is
 *    a running sum.  DTW_semiglobal itself carries a float(1e10) in its first
 *    column and its running best; the device equals it wherever every prefix
 *    sum of column 0 and the result stay below 1e10.
 *  - Subnormal inputs, distances and sums are preserved, and -0.0 inputs cost
 *    +0.0, in every body.
 * tests/test_value_domain_gpu.py holds every body to this on costs below, around
 * and far above 1e10, on subnormals and on zeros of either sign.
 */
#ifndef RAWDTW_H
#define RAWDTW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAWDTW_ABI_VERSION 2

typedef enum {
    RAWDTW_OK = 0,
    RAWDTW_ERR_INVALID = 1,     /* zero length / negative radius: the reference assert()s (dtw.cpp:79,274-277) */
    RAWDTW_ERR_DEVICE = 2,      /* HIP runtime error; see rawdtw_last_error */
    RAWDTW_ERR_OOM = 3,
    RAWDTW_ERR_RANGE = 4,       /* a job window lies outside the uploaded arenas */
    RAWDTW_ERR_UNSUPPORTED = 5, /* e.g. traceback of a banded global job (rmap.cpp:223-225 assert(false)) */
    RAWDTW_ERR_NO_DEVICE = 6,
    RAWDTW_ERR_INTERNAL = 7     /* a check the library makes on its own device work failed: nothing was built */
} rawdtw_status;

#define RAWDTW_FULL (-1) /* band_radius value selecting DTW_global (dtw.hpp:21) */

/* One DTW sub-problem = one call of DTW_global / DTW_global_slantedbanded_antidiagonalwise
 * (dtw.hpp:21,25) as align_chain issues it: a = read events window, b = reference
 * signal window.  32 bytes. */
typedef struct {
    uint64_t ref_off;      /* element offset of b[0] in the reference arena (rawdtw_reference_offset) */
    uint32_t read_off;     /* element offset of a[0] in the batch's event arena */
    uint32_t n;            /* a_length: read events in the window (>=1) */
    uint32_t m;            /* b_length: reference signals in the window (>=1) */
    int32_t band_radius;   /* the band_radius argument (>=0), or RAWDTW_FULL */
    uint32_t exclude_last; /* exclude_last_element */
    uint32_t reserved;     /* 0 */
} rawdtw_job_t;

typedef struct rawdtw_ctx rawdtw_ctx;
typedef struct rawdtw_plan rawdtw_plan;

/* ---- lifetime ---------------------------------------------------------- */
int rawdtw_abi_version(void);
int rawdtw_device_count(int *count);
int rawdtw_create(int device_ordinal, rawdtw_ctx **out);
/* Teardown order is free.  rawdtw_destroy waits for the context's stream, then detaches every plan and batch still alive
 * on it: their device memory and pooled workspaces are released there and then, and rawdtw_plan_destroy /
 * rawdtw_batch_destroy called afterwards only delete the host records (every other entry point refuses a detached
 * batch with RAWDTW_ERR_INVALID).  tests/abi/host_shim.cpp --teardown exercises exactly this. */
int rawdtw_destroy(rawdtw_ctx *ctx);
const char *rawdtw_last_error(const rawdtw_ctx *ctx);
const char *rawdtw_status_string(int status);
int rawdtw_sync(rawdtw_ctx *ctx);
/* ---- options: a context's named integer settings.  Every one is listed here once, with the values it takes and its default, and is a row of
 * rawalign_amd/csrc/rawdtw_options.h, which is where its rule lives.  rawdtw_set_option passes the value through the option's rule: a range
 * written lo..hi CLAMPS a value outside it, a list a/b/c takes the largest entry that is at most the value (the first one below them all), 0/1
 * stores value != 0, and `refuses' means RAWDTW_ERR_INVALID with nothing stored and the reason in rawdtw_last_error.  A name that is not
 * listed, or is read-only, is refused with "unknown option NAME".
 * Tuning knobs -- results never depend on them (tests/test_gpu_parity.py checks that):
 *   "plan_threads"  0..64 (default 0 = from the job count and the machine, <= 16): host threads of the batch planner
 *   "serial_launches"  0/1 (default 0): with side streams, run a batch's launches in sequence anyway
 *   "lane_max_radius"  0..3 (default 3): largest post-slant radius on the tile kernel
 *   "lane_max_n"  8..73 (default 73): longest side there
 *   "lane_hi"  0/1 (default 0): an optional second tile instance for radii up to 8 ...
 *   "lane_hi_max_n"  8..200 (default 96): ... and sides up to this
 *   "micro_max_n"  0/4/8 (default 8): shapes with a longer side up to this take the micro paths
 *   "grp16"  0/1 (default 1): bands of at most 16 offsets, four jobs a wave
 *   "grp8"  0/1 (default 1): bands of at most 8 offsets, eight jobs a wave
 *   "full_wg"  0/1 (default 1): full-matrix jobs of three strips and more, four waves a job
 *   "tile_lds_floats"  1024..40000 (default 4800): the LDS image of a job-list tile; once given, also that of a device-planned batch's pass
 *       (5800 otherwise)
 *   "tile_max_jobs"  64..65535 (default 1024): jobs of a job-list tile
 *   "tile_max_spans"  8..4096 (default 96): arena spans of a job-list tile
 *   "tile_threads"  256/512/1024 (default 256): workgroup size of the tile kernel
 *   "sort_n"  0..255 (default 0 = never): tile jobs with a longer side from this on are tiled by shape, not in job order
 *   "sort_r1_n"  0..255 (default 0 = never): so are those of radius 1 with a longer side from this on
 *   "sort_r3"  0/1 (default 0): and those of radius 3
 *   "sorted_tile_jobs"  16..1024 (default 64): jobs of a by-shape tile
 *   "merge_small"  0/1 (default 1): a sparse batch's tile, 16-lane-row and register-wave kernels as ONE launch
 *   "fold_mode"  0..4 (default 4): chain fold as a wave per chain (0), a lane per chain with 16 / 32 parts per round (1, 2), a lane per chain
 *       plus a wave for each long chain (3), or device-planned batches fold and select in one launch (a read a lane) and job-list batches as 3
 *       (4); a batch keeps the form it was created under
 *   "fold_long_parts"  1..2^30 (default 768): fold mode 3, the parts from which a chain is a long one
 *   "device_plan"  0/1 (default 1): rawdtw_batch_create takes the sync-free path (planning on the device, in LDS)
 *   "device_plan_min_jobs"  0.. (default 0): smaller batches go through the job list
 *   "stream_tile_radius"  1..3 (default 3): the device-planned batch's tiles (512 consecutive anchors) take radii up to this; the radii between
 *       it and "lane_max_radius" are scored a lane per job from the side list, bucketed by length over the whole batch
 *   "stream_threads"  256/512 (default 256): workgroup size of that batch's DTW launch over the tiles' passes (k_runs)
 *   "stream_blocks_per_cu"  0..16 (default 4; 0 = as many as fit): its workgroups a CU
 *   "pass_pool"  -1..2^24 (default -1 = three a tile + 64): copy-order slots beyond one a tile; a batch that runs out is redone through the
 *       job list (tests)
 *   "wide_blocks"  1..65535 (default 256): workgroups of the side list's launch (k_wide)
 *   "wide_beside"  0/1 (default 0): that launch on the context's second stream beside the tiles' launch instead of in line (measured slower)
 *   "wide_order"  0..2 (default 0): that launch between the scan and the pass planning, in front of k_runs, or behind it
 *   "wide_at_create"  0/1 (default 0): that launch goes out with a plain rawdtw_batch_create's planning too (the arenas stay as they are
 *       until the run)
 *   "resident_arrays"  0/1 (default 0): rawdtw_batch_create's anchors / ref_base / read_base are device pointers, used in place
 *   "time_plan"  0/1 (default 0): event pair around a batch's planning kernels (rawdtw_batch_plan_ms)
 *   "debug_skip_kinds"  a mask, cut to 32 bits (default 0): timing experiments only -- launches of the masked kinds are not issued (results wrong)
 *   "debug_skip_tail"  a mask, cut to 32 bits (default 0): the same for a device-planned batch's fold (1) and select (2) launches
 *   "stream_debug"  a mask, cut to 32 bits (default 0): k_runs' debug word
 *   "tb_workspace_mb"  0..2^30 (default 0): the direction-buffer budget of one traceback sub-batch in MiB (rawdtw_traceback_batch*).  0: the
 *       environment variable RAWDTW_TB_WORKSPACE_MB if set, else 16 384.  A non-zero value goes before the variable, which is read at
 *       every call.  A call whose jobs' direction buffers (plus 256 bytes a job) pass the budget is cut, in job order, into sub-batches
 *       that each fit -- a job over the budget goes alone -- and these run as a two-deep pipeline; the results do not depend on the cut.
 * Opt-ins, each described beside the entry points it changes:
 *   "seed_minimizer"  0/1 (default 0): see rawdtw_seed_begin
 *   "chain_long_seeds"  0..2^20 (default 0): see rawdtw_chain_round
 *   "chain_max_chains"  0..4096 (default 0), refuses any other value: see rawdtw_chain_round
 *   "chain_decline_reads"  0 or 1 (default 0), refuses any other value: see rawdtw_chain_round_declined
 *   "device_round_end"  0/1 (default 0): see rawdtw_batch_round_end_begin
 *   "resident_chains"  0..2^20 (default 0): see rawdtw_batch_round_end_keep
 *   "signal_cigar"  0 or 1 (default 0), refuses any other value: see rawdtw_mapper_round_signal_resident
 *   "signal_events_cap"  0.. (default 0 = the mapper's guess): see rawdtw_mapper_round_signal_resident
 * Read-only, computed by the library:
 *   "tb_sub_batches"  read-only: the number of sub-batches of this context's most recent rawdtw_traceback_batch* call; 0 before any.  It is
 *       known once the call has cut its jobs, before the first plan is built: a call refused while it plans (a banded job, say) reports
 *       its cut all the same.
 *   "round_end_kernel_us"  read-only: see rawdtw_batch_round_end_fetch
 *   "round_keep_kernel_us"  read-only: see rawdtw_batch_round_keep_fetch
 * The environment variable RAWDTW_OPTS="name=value,..." applies options at rawdtw_create through rawdtw_set_option; a pair it refuses is
 * ignored.  RAWDTW_LANE_HI, RAWDTW_LANE_HI_MAX_N and RAWDTW_LANE_MAX_R are older spellings of their options, applied the same way before it. */
int rawdtw_set_option(rawdtw_ctx *ctx, const char *name, int64_t value);
/* The value of any option above: a settable one as it is stored -- what rawdtw_set_option made of the value it was given, or the default --,
 * a read-only one as the library computes it.  RAWDTW_ERR_INVALID for a null argument or any other name. */
int rawdtw_get_option(const rawdtw_ctx *ctx, const char *name, int64_t *value);
/* the ctx's hipStream_t, as void* (for event timing on the stream kernels run on) */
int rawdtw_stream(rawdtw_ctx *ctx, void **stream);
/* the device ordinal the context was created on */
int rawdtw_context_device(const rawdtw_ctx *ctx, int *device_ordinal);

/* ---- reference signals: replaces ri_idx_t.forward_signals / reverse_signals
 * (src/rawindex.h:32-34) as the `b` operand.  Uploaded once, resident in HBM.
 * strand uses the reference's convention: chain.strand==1 selects fwd
 * (rmap.cpp:182-188). ---- */
int rawdtw_upload_reference(rawdtw_ctx *ctx, uint32_t n_seq, const float *const *fwd,
                            const float *const *rev, const uint32_t *len);
int rawdtw_reference_offset(const rawdtw_ctx *ctx, uint32_t seq, int strand, uint64_t *off);
/* Adopt a device-resident arena instead (caller keeps ownership; 16-byte aligned, and readable up to the next multiple
 * of four floats: the kernels copy whole 16-byte pieces of it). */
int rawdtw_set_reference_device(rawdtw_ctx *ctx, const float *d_ref, uint64_t n_floats);
/* Several contexts on one device (one per pipeline worker, rmap.cpp:1033) share ONE resident copy: `ctx` adopts the
 * arena and the sequence table of `owner`.  An arena the library allocated (rawdtw_upload_reference, rawdtw_index_upload)
 * is reference-counted: it lives until the last context using it uploads another reference or is destroyed, so the
 * owner may go first.  An arena adopted with rawdtw_set_reference_device stays the caller's to keep alive. */
int rawdtw_share_reference(rawdtw_ctx *ctx, const rawdtw_ctx *owner);

/* ---- index file reader: the part of ri_idx_load (src/rawindex.cpp:317-377) the DTW path needs --
 * header, sequence table and the per-sequence forward/reverse signal arrays of a RawAlign `.ind`
 * file (format written by ri_idx_dump, src/rawindex.cpp:275-315: magic "RI" (2 bytes, rawindex.h:7-8), 8 x u32 parameters
 * {w,e,n,q,lq,k,n_seq,flag}, then per sequence {u8 name_len, name, u32 len, len fwd floats, len rev
 * floats}; the hash buckets that follow are not read).  rawdtw_index_upload streams the signal
 * arrays straight into the ctx's reference arena, so a human-size index never sits in host memory. */
typedef struct rawdtw_index rawdtw_index;
int rawdtw_index_open(const char *path, rawdtw_index **out);
int rawdtw_index_info(const rawdtw_index *idx, uint32_t *n_seq, uint32_t pars[8]);
int rawdtw_index_seq(const rawdtw_index *idx, uint32_t i, const char **name, uint32_t *len);
int rawdtw_index_upload(rawdtw_ctx *ctx, const rawdtw_index *idx);
/* host copy of one strand's array (tests / CPU baseline); out must hold len floats */
int rawdtw_index_read_signal(const rawdtw_index *idx, uint32_t i, int strand, float *out);
int rawdtw_index_close(rawdtw_index *idx);

/* ---- read events: the `a` operand (p->events[read].values, rmap.cpp:517) of all
 * reads of a batch, concatenated by the caller. ---- */
int rawdtw_upload_events(rawdtw_ctx *ctx, const float *h_events, uint64_t n_floats);
/* (a caller's device array: 16-byte aligned, readable up to the next multiple of four floats) */
int rawdtw_set_events_device(rawdtw_ctx *ctx, const float *d_events, uint64_t n_floats);
/* Incremental form.  A read's event array only grows (ri_map_frag appends each chunk's events, rmap.cpp:554-567), so a
 * mapper that keeps one slot per read in the arena uploads only the round's NEW events: reserve grows the arena to
 * n_floats (contents kept; the arena's logical size, against which job windows are checked, becomes at least
 * n_floats); append copies h_new[seg_src_off[s] .. seg_src_off[s+1]) to arena offset seg_dst_off[s] for every
 * segment s (one H2D copy of the packed new events + a scatter kernel), asynchronously on the ctx stream.  h_new and
 * the segment tables must stay valid until the stream has passed the call (rawdtw_sync / a fetch); memory from
 * rawdtw_host_alloc makes the copies asynchronous. */
int rawdtw_events_reserve(rawdtw_ctx *ctx, uint64_t n_floats);
int rawdtw_events_append(rawdtw_ctx *ctx, const float *h_new, uint64_t n_new, uint32_t n_segments,
                         const uint64_t *seg_src_off, const uint32_t *seg_dst_off);
/* The way back: stretches of the arena to the host.  Segment q is arena[seg_start[q] .. seg_start[q] + seg_len[q]); the segments
 * (overlapping or empty ones too) arrive densely in order in out, out_off[0 .. n_segments] is written with their prefix sum.  One
 * gather launch; the call waits for it.  An `out` from rawdtw_host_alloc is written by the device itself, any other memory takes a
 * staging block of the context and one copy.  Before anything is enqueued: RAWDTW_ERR_INVALID for a null argument, a context without
 * an arena, a segment that ends beyond the arena's logical size, and a page-locked `out` whose allocation does not hold out_cap
 * floats from `out` on; RAWDTW_ERR_RANGE when the segments' total is above out_cap -- out_off is filled then too, out is not
 * touched.  Nothing is written behind the total. */
int rawdtw_events_fetch(rawdtw_ctx *ctx, uint32_t n_segments, const uint32_t *seg_start, const uint32_t *seg_len,
                        uint64_t *out_off /* n_segments+1, written */, float *out, uint64_t out_cap);
/* Page-locked host memory for the arrays handed to rawdtw_batch_create / rawdtw_events_append and for the result
 * arrays of rawdtw_batch_fetch.  Any host memory works; with pinned memory the copies do not block the caller. */
int rawdtw_host_alloc(uint64_t bytes, void **out);
int rawdtw_host_free(void *p);
/* 1 when p points into page-locked host memory (rawdtw_host_alloc's, or any the HIP runtime knows), else 0 */
int rawdtw_host_is_page_locked(const void *p);

/* ---- score-only batches: replaces the calls at rmap.cpp:211,215,273,277 ---- */
/* One shot: upload events, bin + launch, copy costs back (out_cost[k] for jobs[k]). */
int rawdtw_score_batch(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs,
                       const float *h_events, uint64_t n_events, float *out_cost);

/* Split form, for callers that keep inputs resident (and for benchmarking):
 * plan_create validates and size-bins the jobs and uploads device descriptors;
 * plan_run only launches kernels on the ctx stream (asynchronous); costs stay in
 * HBM, out[k] for jobs[k]; plan_fetch waits and copies them to the host. */
typedef struct {
    uint64_t n_jobs;
    uint64_t cells;            /* DP cells the batch evaluates (exact, band cell sets counted) */
    uint64_t algorithmic_bytes; /* sum over jobs of 4(n+m)+4+32 */
    uint64_t n_lane_jobs;      /* jobs on the lane-per-job banded kernel */
    uint64_t n_wave_band_jobs; /* jobs on the wave-per-job banded kernel */
    uint64_t n_full_jobs;      /* jobs on the full-matrix wavefront kernel */
    uint64_t workspace_bytes;
    uint32_t n_launches;
} rawdtw_plan_info_t;

int rawdtw_plan_create(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs,
                       rawdtw_plan **out);
int rawdtw_plan_info(const rawdtw_plan *plan, rawdtw_plan_info_t *info);
/* Host half of rawdtw_plan_create only -- no device is touched and nothing is scored.  Bins the
 * jobs against arenas of n_events / n_reference floats with `threads` planner threads and the
 * given planner options (names as for rawdtw_set_option), then checks every invariant the
 * kernels rely on (each job planned exactly once, launches partition the plan, every tile's
 * windows staged inside its LDS budget at the right place).  Returns the status plan_create
 * would return; `message` (optional) receives the reason of a failure.  The extra option
 * "verify" = 0 skips the self-check and the cell count (to time the planner alone).  For
 * host-side tests and for sizing a batch before a device is attached. */
int rawdtw_plan_dry_run(uint64_t n_events, uint64_t n_reference, const rawdtw_job_t *jobs,
                        uint64_t n_jobs, int threads, const char *const *option_names,
                        const int64_t *option_values, uint32_t n_options,
                        rawdtw_plan_info_t *info, uint64_t *n_tiles, char *message,
                        uint32_t message_cap);
int rawdtw_plan_run(rawdtw_ctx *ctx, rawdtw_plan *plan);
int rawdtw_plan_fetch(rawdtw_ctx *ctx, rawdtw_plan *plan, float *out_cost);
/* device pointer to the costs (job order) and the host array mapping launch order -> job index */
int rawdtw_plan_device_costs(const rawdtw_plan *plan, const float **d_cost,
                             const uint32_t **h_order);
/* per-launch kernel names and HIP-event durations (ms) of the most recent
 * rawdtw_plan_run_timed; arrays hold up to n_launches entries */
int rawdtw_plan_run_timed(rawdtw_ctx *ctx, rawdtw_plan *plan, float *launch_ms,
                          uint32_t *launch_kind, uint32_t cap);
int rawdtw_plan_destroy(rawdtw_plan *plan);

/* ---- traceback batches: replaces DTW_global_tb (dtw.hpp:28) at rmap.cpp:221,284.
 * Jobs must have band_radius == RAWDTW_FULL.  The direction matrix is kept as a
 * packed 2-bit buffer in HBM and walked on the GPU.  path_off[k] (caller
 * supplied, elements) locates job k's path inside path_i/path_j/path_d, which
 * must have room for n+m-1 entries per job; entries come out in forward order,
 * i indexing a (read window), j indexing b (reference window). ---- */
int rawdtw_traceback_batch(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs,
                           const float *h_events, uint64_t n_events, float *out_cost,
                           const uint64_t *path_off, uint32_t *path_len, uint32_t *path_i,
                           uint32_t *path_j, float *path_d);

/* The same with the paths in the form they leave the device in: per element ONE byte, the step from the element before it
 * (bit 0: i advanced, bit 1: j advanced; element 0 of a global path is (0, 0): dtw.cpp:640-655, its step byte is 0), and its
 * distance -- 5 bytes an element over the bus and into the caller's arrays instead of 12.  A consumer that walks the path in
 * order (the aln:s: writer, rmap.cpp:580-592) needs nothing else. */
int rawdtw_traceback_batch_steps(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs,
                                 const float *h_events, uint64_t n_events, float *out_cost,
                                 const uint64_t *path_off, uint32_t *path_len, uint8_t *path_step, float *path_d);

/* rawdtw_traceback_batch_steps over the context's event arena AS IT LIES: the jobs' read_off index the arena whatever filled it
 * (rawdtw_upload_events, rawdtw_set_events_device, rawdtw_events_reserve / _append, a resident detection).  Nothing is uploaded and
 * nothing is written into the arena.  RAWDTW_ERR_INVALID before anything is enqueued for a context without an arena and for a job
 * whose read_off + n lies beyond the arena's logical size; otherwise the statuses, the path layout, the sub-batches
 * ("tb_workspace_mb") and the timing counters are those of the steps form. */
int rawdtw_traceback_arena_steps(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, float *out_cost,
                                 const uint64_t *path_off, uint32_t *path_len, uint8_t *path_step, float *path_d);

/* Device time of the most recent rawdtw_traceback_batch on this context (HIP events on its stream, summed over its
 * sub-batches): fill = the full-matrix kernels that write the packed 2-bit directions, walk = the traceback walk and the
 * path finish; direction_bytes = the packed direction buffers of its jobs; path_elements = the elements of all paths. */
int rawdtw_traceback_timing(const rawdtw_ctx *ctx, float *fill_ms, float *walk_ms, uint64_t *direction_bytes,
                            uint64_t *path_elements);

/* ---- aln text: the aln:s: string of paths (dtwresult_to_string, rmap.cpp:580-592), defined once and made on the device.
 * Element q of job k is (i, j, d).  (pi, pj) starts at (0, j0) and advances by bits 0 and 1 of the element's step byte before the
 * element is read (element 0's step byte is 0).  mode 1 (the sparse and the local way, rmap.cpp:286-289): i = pi + off_i,
 * j = pj + off_j on every element.  mode 0 (the global branch's quirk, rmap.cpp:230-233): only the job's last element moves, by
 * len * off_i and len * off_j, len the job's element count; the arithmetic is unsigned 64-bit and wraps.  The element's text is
 *     "(" i "," j "," g ")"     i, j in decimal, g the bytes of snprintf("%g", (double)d) under the C locale (= ostream << float)
 * for EVERY bit pattern of d (0, -0, inf, -inf, nan, -nan, denormals; nothing is declined).  Jobs' texts are packed in job order with
 * no separator and no terminating NUL: job k occupies text[text_off[k] .. text_off[k + 1]), text_off has n_jobs + 1 entries, a job of
 * 0 elements occupies nothing.  rawalign_amd/csrc/rawdtw_fmt_g.h is the one formatter behind all of the entry points below. ---- */
typedef struct {
    uint64_t off_i, off_j;
    uint32_t j0;
    uint32_t mode; /* 0 or 1 */
    uint64_t pad;  /* not read */
} rawdtw_aln_rec_t; /* 32 bytes */

/* The definition restated on host threads (threads 0: as many as the machine has, at most 16); needs no GPU.  Job k's path is the
 * path_len[k] step bytes and distances from path_off[k] on (the layout of rawdtw_traceback_batch_steps).  text_off (n_jobs + 1
 * entries) and *text_bytes are always written; text == NULL: sizes only.  RAWDTW_ERR_RANGE when text_cap is below *text_bytes: text is
 * not written at all.  RAWDTW_ERR_INVALID for a null argument or a mode other than 0 and 1. */
int rawdtw_aln_text_host(const uint8_t *path_step, const float *path_d, const uint64_t *path_off, const uint32_t *path_len,
                         const rawdtw_aln_rec_t *recs, uint64_t n_jobs, int threads, uint64_t *text_off, char *text,
                         uint64_t text_cap, uint64_t *text_bytes);
/* An upper bound on the text of these jobs' paths whatever the paths are: n + m - 1 elements a job, the digits of the largest i and j
 * an element of that job can have, 12 bytes for the distance, 4 of punctuation.  A buffer of this size is never too small. */
uint64_t rawdtw_aln_text_bound(const rawdtw_job_t *jobs, const rawdtw_aln_rec_t *recs, uint64_t n_jobs);
/* The same contract as rawdtw_aln_text_host on the device, from host arrays: upload, k_aln_count, k_aln_scan, k_aln_write, text
 * home.  The kernels alone; statuses as the host form, and RAWDTW_ERR_OOM / RAWDTW_ERR_DEVICE. */
int rawdtw_aln_text_steps(rawdtw_ctx *ctx, const uint8_t *path_step, const float *path_d, const uint64_t *path_off,
                          const uint32_t *path_len, const rawdtw_aln_rec_t *recs, uint64_t n_jobs, uint64_t *text_off, char *text,
                          uint64_t text_cap, uint64_t *text_bytes);
/* rawdtw_traceback_batch_steps / rawdtw_traceback_arena_steps whose paths never leave the device: the jobs, events, arena, refusals,
 * statuses and sub-batches ("tb_workspace_mb") of those, and one rec a job.  What comes home a sub-batch is its costs and lengths,
 * 8 bytes a job of text offsets, and the text, behind the walk.  path_len[k] is the path's element count after exclude_last dropped
 * its last element -- the text is made of those elements, and under mode 0 len is that count.  The text does not depend on how the
 * batch was cut.  text == NULL: sizes only.  RAWDTW_ERR_RANGE, with out_cost, path_len, text_off and *text_bytes filled, when text_cap
 * is below *text_bytes; a text buffer of rawdtw_aln_text_bound bytes never is.  A null recs, text_off or text_bytes is refused as a
 * null argument of the steps form is. */
int rawdtw_traceback_batch_text(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events, uint64_t n_events,
                                const rawdtw_aln_rec_t *recs, float *out_cost, uint32_t *path_len, uint64_t *text_off, char *text,
                                uint64_t text_cap, uint64_t *text_bytes);
int rawdtw_traceback_arena_text(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const rawdtw_aln_rec_t *recs,
                                float *out_cost, uint32_t *path_len, uint64_t *text_off, char *text, uint64_t text_cap,
                                uint64_t *text_bytes);
/* Device time of the text launches of the most recent of the three calls above on this context (HIP events, summed over
 * sub-batches): count_ms = k_aln_count and k_aln_scan, write_ms = k_aln_write; text_bytes = the text they made. */
int rawdtw_aln_text_timing(const rawdtw_ctx *ctx, float *count_ms, float *write_ms, uint64_t *text_bytes);

/* ---- single-call drop-ins with the reference's own signatures flattened
 * (dtw.hpp:21,25,28).  Host pointers; convenient, not fast. ---- */
int rawdtw_dtw_global(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m,
                      int exclude_last, float *cost);
int rawdtw_dtw_global_slantedbanded_antidiagonalwise(rawdtw_ctx *ctx, const float *a, uint32_t n,
                                                     const float *b, uint32_t m, int band_radius,
                                                     int exclude_last, float *cost);
int rawdtw_dtw_global_tb(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m,
                         int exclude_last, float *cost, uint32_t *path_len, uint32_t *path_i,
                         uint32_t *path_j, float *path_d);

/* ---- semiglobal (subsequence) DTW: replaces DTW_semiglobal, DTW_semiglobal_slow and DTW_semiglobal_tb (dtw.hpp; dtw.cpp:526-593,
 * 669-753).  a (the job's read window) is aligned end to end against the best-matching substring of b (its reference window):
 *   D(0, j) = d(0, j);  D(i, 0) = D(i-1, 0) + d(i, 0);  D(i, j) = min(min(D(i-1, j), D(i, j-1)), D(i-1, j-1)) + d(i, j)
 * in fp32 with d = |a[i] - b[j]|.  The cost is the minimum of row n - 1 and end_j the FIRST column that attains it.  The path starts
 * at (n - 1, end_j), walks by the three-way rule of the global traceback (at j == 0 it moves up) and stops as soon as i == 0: its
 * first element is (0, j0), it has at most n + m - 1 elements.  Jobs are rawdtw_job_t with band_radius == RAWDTW_FULL; they are
 * bucketed by n alone (a always lies over the lanes of the kernel, also when n > m) and every (n, m) with n, m >= 1 runs.
 * h_events == NULL: the jobs' read_off index the context's event arena as it lies (as rawdtw_traceback_arena_steps) and n_events is
 * not looked at; else the arena is replaced by h_events first.  Refused before anything is enqueued: RAWDTW_ERR_INVALID for n == 0,
 * m == 0, a banded job, a null argument and a context without the arena it needs; RAWDTW_ERR_RANGE for a window outside the arenas.
 * n_jobs == 0 is RAWDTW_OK and touches nothing.
 *   rawdtw_semiglobal_batch            cost and end_j of every job.  exclude_last subtracts d(n - 1, end_j), as DTW_semiglobal_slow
 *        and DTW_semiglobal_tb do (DTW_semiglobal takes the argument and ignores it).
 *   rawdtw_semiglobal_traceback_steps  the paths too, in the step form of rawdtw_traceback_batch_steps: room for n + m - 1 elements a
 *        job from path_off[k] on, start first; per element its distance and one byte (bit 0: i advanced, bit 1: j advanced; element
 *        0 is (0, out_j0[k]), its byte is 0).  With exclude_last the last element is dropped and the cost reduced by its distance.
 *        Sub-batches under "tb_workspace_mb" ("tb_sub_batches" says how many) as the global traceback.
 *   rawdtw_semiglobal_timing           device time of the most recent of those calls (or of a span call, below) on the context: the fill kernels, and the
 *        walk and finish kernels (0 for a cost-only call); the direction bytes written and the path elements that came home.
 *   rawdtw_dtw_semiglobal, rawdtw_dtw_semiglobal_tb   the single-call drop-ins (host pointers; convenient, not fast).  The first
 *        ignores exclude_last as its namesake does; the second writes (path_i, path_j, path_d) like rawdtw_dtw_global_tb.
 *   rawdtw_semiglobal_host, rawdtw_semiglobal_tb_host   the recurrence restated on the host (no device work): the yardstick of the
 *        tests where a shape is too large for a recorded answer.  end_j and the path arrays may be NULL.
 *
 * The span of a job is (cost, j0, end_j): both ends of the matched substring of b, without a direction matrix.  cost and end_j are
 * exactly rawdtw_semiglobal_batch's, the exclude_last subtraction included.  j0 is the column of element 0 of the path that
 * DTW_semiglobal_tb (dtw.cpp:669-753) returns: bit for bit out_j0 of rawdtw_semiglobal_traceback_steps; exclude_last does not change
 * it.  Stated forwards, with S(i, j) the start column of the path that ends in (i, j):
 *   S(0, j) = j;  S(i, 0) = 0, whatever the values (at j == 0 the walk moves up without reading a neighbour);  elsewhere, with
 *   up = D(i-1, j), lf = D(i, j-1), dg = D(i-1, j-1):  up < min(lf, dg) -> S(i-1, j);  else lf < min(up, dg) -> S(i, j-1);  else
 *   S(i-1, j-1) (the reference's quirk included: up == lf < dg takes the diagonal);  j0 = S(n-1, end_j).
 * The comparisons are the walk's own, so j0 equals the traceback's on every value domain.  One pass, O(m) boundary state a job.
 *   rawdtw_semiglobal_span_batch   cost, j0 and end_j of every job: rawdtw_semiglobal_batch's contract word for word (h_events == NULL,
 *        the refusals and their statuses, n_jobs == 0).  No sub-batches: there is no direction workspace, "tb_sub_batches" is not
 *        touched.  rawdtw_semiglobal_timing afterwards: the span launches as fill_ms, 0 for the walk, the bytes and the elements.
 *   rawdtw_dtw_semiglobal_span     the single-call drop-in (host pointers; convenient, not fast).
 *   rawdtw_semiglobal_span_host    the definition restated on the host in O(m) memory (two rows of cost and of start): the yardstick
 *        where rawdtw_semiglobal_tb_host's n x m matrix is too large.  cost, j0 and end_j may be NULL. ---- */
int rawdtw_semiglobal_batch(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events, uint64_t n_events,
                            float *out_cost, uint32_t *out_end_j);
int rawdtw_semiglobal_traceback_steps(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events,
                                      uint64_t n_events, float *out_cost, uint32_t *out_j0, const uint64_t *path_off,
                                      uint32_t *path_len, uint8_t *path_step, float *path_d);
int rawdtw_semiglobal_timing(const rawdtw_ctx *ctx, float *fill_ms, float *walk_ms, uint64_t *direction_bytes,
                             uint64_t *path_elements);
int rawdtw_dtw_semiglobal(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m, int exclude_last, float *cost);
int rawdtw_dtw_semiglobal_tb(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m, int exclude_last, float *cost,
                             uint32_t *path_len, uint32_t *path_i, uint32_t *path_j, float *path_d);
int rawdtw_semiglobal_host(const float *a, uint32_t n, const float *b, uint32_t m, int exclude_last, float *cost, uint32_t *end_j);
int rawdtw_semiglobal_tb_host(const float *a, uint32_t n, const float *b, uint32_t m, int exclude_last, float *cost, uint32_t *end_j,
                              uint32_t *path_len, uint32_t *path_i, uint32_t *path_j, float *path_d);
int rawdtw_semiglobal_span_batch(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events, uint64_t n_events,
                                 float *out_cost, uint32_t *out_j0, uint32_t *out_end_j);
int rawdtw_dtw_semiglobal_span(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m, int exclude_last, float *cost,
                               uint32_t *j0, uint32_t *end_j);
int rawdtw_semiglobal_span_host(const float *a, uint32_t n, const float *b, uint32_t m, int exclude_last, float *cost, uint32_t *j0,
                                uint32_t *end_j);

/* ---- semiglobal, in windows: the traceback above without n x m directions (opt-in by rawdtw_set_semiglobal_window).  The path touches
 * the columns j0 .. end_j only; cell values do not depend on evaluation order, row 0 is assigned, and everything left of a column
 * reaches the cells right of it through that column alone.  For a job (a, n, b, m) and a window width C (a multiple of 64):
 *   checkpoints   column k C - 1 of D is kept, n floats, for every k >= 1 with k C - 1 < m; the cost-only pass writes them.
 *   window        of a walk position (i, j), i > 0: the columns c_lo .. j with c_lo = (j / C) C.  Its cells are D's own: column
 *                 c_lo - 1 is read from the checkpoint (for c_lo == 0 there is no column -1, as above), row 0 is assigned, and a cell's
 *                 direction is coded by the walk's own two comparisons, exactly as the n x m form codes it.
 *   walk          the rule above; "moves up without reading a neighbour" is GLOBAL column 0 only.  A step from column c_lo to column
 *                 c_lo - 1 (left or diagonal) is emitted, and the walk goes on in the window of the new position.  It ends at i == 0.
 *   result        the n x m form's on every value domain -- cost, end_j, j0, the path, exclude_last: the same cell values and the same
 *                 comparisons, nothing numeric.
 * Direction memory is one window a job (n C / 4 bytes in place of n m / 4) and (m / C) n floats of checkpoints; the cells filled with
 * directions are those of the windows the walk enters, rows 0 .. i of each.
 *   rawdtw_set_semiglobal_window, rawdtw_get_semiglobal_window   the window width of the context: 0 = off, the default; else a multiple
 *        of 64 in [64, 2^20]; anything else is RAWDTW_ERR_INVALID and nothing is stored.  A setter, not an option.  Honoured by
 *        rawdtw_semiglobal_traceback_steps, rawdtw_dtw_semiglobal_tb and, through its context, rawdtw_mapper_finish's local finish.
 *        Refusals, statuses, path room (n + m - 1 a job) and the out arrays' contracts are those above, word for word.  A job with
 *        m <= C is not windowed: it takes the n x m form's records and launches, in the same call.
 *        rawdtw_semiglobal_timing afterwards: fill_ms is every fill launch (the cost form with checkpoints, and the n x m fills of the
 *        jobs not windowed); walk_ms is the window launches -- refill and walk are one kernel and cannot be told apart -- plus the finish
 *        launches and the other jobs' walks; direction_bytes is the workspace the jobs took (a windowed job: its window's directions
 *        and its checkpoints, each rounded up to 256).
 *   rawdtw_semiglobal_window_stats   of the context's most recent semiglobal traceback call: the jobs that were windowed, the windows
 *        they entered in all and the most one job entered, and the bytes of their checkpoints (part of direction_bytes).  Any may be NULL.
 *   rawdtw_semiglobal_tb_window_host   the definition restated on the host in O(n m / C + n C) memory (no device work): the yardstick
 *        where rawdtw_semiglobal_tb_host's matrix is too large.  columns as the setter's (0 or m <= columns: the n x m form, *windows 0);
 *        end_j and windows may be NULL. ---- */
int rawdtw_set_semiglobal_window(rawdtw_ctx *ctx, uint32_t columns);
int rawdtw_get_semiglobal_window(const rawdtw_ctx *ctx, uint32_t *columns);
int rawdtw_semiglobal_window_stats(const rawdtw_ctx *ctx, uint64_t *jobs_windowed, uint64_t *windows, uint64_t *max_windows_a_job,
                                   uint64_t *checkpoint_bytes);
int rawdtw_semiglobal_tb_window_host(const float *a, uint32_t n, const float *b, uint32_t m, int exclude_last, uint32_t columns,
                                     float *cost, uint32_t *end_j, uint32_t *path_len, uint32_t *path_i, uint32_t *path_j, float *path_d,
                                     uint32_t *windows);

/* ---- banded traceback: the path of a banded global job.  The reference has none (rmap.cpp:223-225 is assert(false)); this is the
 * one definition that agrees with both reference functions it sits between.  For a job (a, n, b, m, R), R = band_radius >= 0, i
 * indexing a and j indexing b, also when n < m and the reference swaps the two:
 *   cell set S(n, m, R)  the cells DTW_global_slantedbanded_antidiagonalwise evaluates (dtw.cpp:273-520).
 *   matrix   B(0, 0) = d(0, 0); every other cell of S is min(min(B(i-1, j), B(i, j-1)), B(i-1, j-1)) + d(i, j) in fp32,
 *            d = |a[i] - b[j]|; a neighbour outside the matrix or outside S is read as float(1e10).  These are the values of the
 *            reference's three rotating buffers.
 *   cost     B(n-1, m-1): the reference's banded cost, bit for bit.
 *   walk     from (n-1, m-1) until (0, 0), by dtw.cpp:625-647 with absent neighbours read as 1e10: if i == 0, j--; else if j == 0,
 *            i--; else with L = B(i-1, j), T = B(i, j-1), X = B(i-1, j-1): L < min(T, X) moves i--; else T < min(L, X) moves j--;
 *            else both (the reference's quirk included: L == T < X steps diagonally).  With a band that holds the whole matrix
 *            (R = n + m) cost and path are DTW_global_tb's, below 1e10.
 *   no path  a step that lands on a cell outside S: path_len = 0, nothing is written to the job's path stretch, the cost is still
 *            written.  It happens only where sums reach 1e10 (a smallest case: a = [0, 0, 0], b = [0, 3e10, 0], R = 1); it is no error status.
 *   exclude_last  as DTW_global_tb: the last element is dropped and the cost reduced by its distance.
 *
 *   rawdtw_banded_traceback_steps   the step form and path room (n + m - 1 a job) of rawdtw_traceback_batch_steps.  h_events == NULL:
 *        the jobs' read_off index the event arena as it lies; else the arena is replaced by h_events first.  Sub-batches under
 *        "tb_workspace_mb" by the jobs' direction bytes ("tb_sub_batches" says how many).  Refused before anything is enqueued, the
 *        out arrays untouched: RAWDTW_ERR_INVALID for n == 0, m == 0, band_radius < 0 (RAWDTW_FULL included: rawdtw_traceback_batch*
 *        serves it), a null argument, a missing arena; RAWDTW_ERR_RANGE for a window outside the arenas; RAWDTW_ERR_UNSUPPORTED for
 *        a slant-corrected radius + 1 above 13 000 slots (the planner's limit and wording).  n_jobs == 0 is RAWDTW_OK.
 *   rawdtw_banded_traceback_timing  device time of the most recent such call: the fill kernel, the walk and finish kernels; the
 *        direction bytes its jobs took and the path elements that came home.
 *   rawdtw_dtw_global_banded_tb     the single-call drop-in (host pointers; convenient, not fast), arrays as rawdtw_dtw_global_tb.
 *   rawdtw_banded_tb_host           the definition restated on the host, O((n + m) K) memory, no device: the tests' yardstick where a
 *        shape is too large for a matrix.  RAWDTW_ERR_INVALID for a null argument, a zero length or a negative radius,
 *        RAWDTW_ERR_UNSUPPORTED above the device entry's 13 000 slots, RAWDTW_ERR_OOM where its memory cannot be had. ---- */
int rawdtw_banded_traceback_steps(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events, uint64_t n_events,
                                  float *out_cost, const uint64_t *path_off, uint32_t *path_len, uint8_t *path_step, float *path_d);
int rawdtw_banded_traceback_timing(const rawdtw_ctx *ctx, float *fill_ms, float *walk_ms, uint64_t *direction_bytes,
                                   uint64_t *path_elements);
int rawdtw_dtw_global_banded_tb(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m, int band_radius,
                                int exclude_last, float *cost, uint32_t *path_len, uint32_t *path_i, uint32_t *path_j, float *path_d);
int rawdtw_banded_tb_host(const float *a, uint32_t n, const float *b, uint32_t m, int band_radius, int exclude_last, float *cost,
                          uint32_t *path_len, uint32_t *path_i, uint32_t *path_j, float *path_d);

/* ---- host-side mirror of align_chain / the DTW block of gen_chains
 * (src/rmap.cpp:181-313, 509-530): job decomposition and exact replay.  Pure
 * host code, no device work. ---- */
typedef struct {
    uint32_t target_position;
    uint32_t query_position;
} rawdtw_anchor_t; /* ri_anchor_t, rmap.h:21-27; stored end-first like the reference */

typedef struct {
    int border_constraint;  /* 0 global, 1 sparse, 2 local (roptions.h:21-23; 2: "local border" below) */
    int fill_method;        /* 0 full, 1 banded (roptions.h:25-26) */
    float band_radius_frac; /* roptions.c:51 */
    float match_bonus;      /* roptions.c:52 */
    float min_score;        /* roptions.c:53 */
    int fused_score;        /* 1: score = fmaf(n, bonus, -cost) as the reference's -O3 -march=native build contracts it */
} rawdtw_align_opt_t;

/* ---- local border: border_constraint == 2.  The reference's command line offers --dtw-border-constraint local and align_chain exits on
 * it ("invalid border constraint", rmap.cpp:301-304); this is the one definition the library gives it.  For a chain with anchors
 * end-first, s = anchors[n_anchors - 1], e = anchors[0]:
 *   windows   the global branch's (rmap.cpp:198-202): a = read events s.q .. e.q, n = e.q - s.q + 1; b = the strand's signals
 *             s.t .. e.t, m = e.t - s.t + 1.  No flanks.  The read window stays pinned, the reference ends are free.
 *   jobs      one a chain (rawdtw_chain_job_count is 1): the global job with band_radius = RAWDTW_FULL and exclude_last = 0, with and
 *             without `cigar`.  fill_method and band_radius_frac are NOT looked at: dtw.hpp has no banded semiglobal.
 *   cost      DTW_semiglobal_slow(a, n, b, m, false), i.e. rawdtw_semiglobal_batch's cost: the sentinel-free recurrence, end_j the
 *             first minimum of the last row.
 *   score     the global branch's: the early exit (float)n * match_bonus < min_score gives -1e10 (rmap.cpp:205-209), num_aligned = n,
 *             the final score by rmap.cpp:306 under fused_score.  rawdtw_chain_replay takes the global branch.
 *   cigar     DTW_semiglobal_tb(a, n, b, m): every element offset by (s.q, s.t), the sparse branch's way (rmap.cpp:285-289; the global
 *             branch's add-to-back() quirk is not used); the first element is (s.q, s.t + j0), the last (e.q, s.t + end_j); the cost
 *             bits are the score-only job's.
 *   after     the sequential accept/cut of gen_chains, primary chains, MAPQ, the stop rule and the PAF columns (the chain's own start
 *             and end) are unchanged.
 *   property  for finite inputs a chain's local cost is at most its global full-matrix cost, bit for bit as floats: both run the same
 *             recurrence, row 0 of the local one is cell by cell at most the global one's running sum, the last row's minimum is at
 *             most its last cell -- min is exact and fp32 add is monotone.  The two are equal when m == 1.
 * Opt-in: off (the default) every entry point that takes a context refuses 2 with the status and the wording it always had.  After
 * rawdtw_set_border_local(ctx, 1), rawdtw_batch_create / _submit / _submit_device / _submit_compact and rawdtw_mapper_create on that
 * context accept 2 (a mapper's second read group copies the setting); rawdtw_batch_submit_carry and rawdtw_batch_can_carry answer as
 * they do for global.  rawdtw_mapper_create without a context (a scorer-only mapper) and the functions that take no context --
 * rawdtw_chain_job_count, _build_jobs, _replay, rawdtw_batch_build_jobs, rawdtw_batch_replay -- accept 2 always.  Any other value is
 * refused as before.  A local batch is a job-list batch whose launches are semiglobal fills (launch kind 11, param = rows a lane);
 * from device arrays its job records are written on the device (two anchors a chain are read, none comes home).  A setter, not a
 * context option. ---- */
int rawdtw_set_border_local(rawdtw_ctx *ctx, int on);
int rawdtw_get_border_local(const rawdtw_ctx *ctx, int *on);

/* Number of DTW jobs align_chain issues for a chain (before any early exit). */
uint32_t rawdtw_chain_job_count(const rawdtw_align_opt_t *opt, uint32_t n_anchors);
/* Emit those jobs. ref_base = arena offset of the chain's strand array
 * (rawdtw_reference_offset), read_base = arena offset of the read's events. */
int rawdtw_chain_build_jobs(const rawdtw_align_opt_t *opt, const rawdtw_anchor_t *anchors,
                            uint32_t n_anchors, uint64_t ref_base, uint32_t read_base, int cigar,
                            rawdtw_job_t *jobs_out);
/* Fold per-job costs back into align_chain's result, replaying its early exits
 * (rmap.cpp:205-209, 265-268) with min_score. Returns the alignment score. */
float rawdtw_chain_replay(const rawdtw_align_opt_t *opt, const rawdtw_anchor_t *anchors,
                          uint32_t n_anchors, const float *job_cost, float min_score);
/* The sequential loop of rmap.cpp:515-524 over one read's chains, given in
 * evaluation order; chain c owns job_cost[job_off[c]..job_off[c+1]).  Writes
 * score[c], keep[c]; returns the number kept. */
uint32_t rawdtw_read_replay(const rawdtw_align_opt_t *opt, uint32_t n_chains,
                            const uint32_t *anchor_off, const rawdtw_anchor_t *anchors,
                            const uint64_t *job_off, const float *job_cost, float *score,
                            uint8_t *keep);


/* ---- consumers of alignment_score downstream of the DTW block (pure host code) ---- */
typedef struct {
    float chaining_score;
    float alignment_score;
    uint32_t reference_sequence_index;
    uint32_t start_position;
    uint32_t end_position;
    uint32_t n_anchors;
    int32_t strand;
    uint32_t mapq; /* out: comp_mapq's value for the first kept chain */
    uint32_t tag;  /* caller's handle; travels with the record through the sort */
} rawdtw_chain_t; /* the scalar fields of ri_chain_t (src/rmap.h:29-46) */

typedef struct {
    int evaluate_chains;      /* opt->flag & RI_M_DTW_EVALUATE_CHAINS */
    float min_bestmap_ratio;  /* roptions.c:28 (1.2) */
    float min_meanmap_ratio;  /* roptions.c:31 (5)   */
    uint32_t min_chain_anchor; /* roptions.c:25 (2)  */
} rawdtw_select_opt_t;

/* gen_primary_chains + comp_mapq (src/rmap.cpp:90-128, 65-88): sorts `chains` in place exactly as
 * std::sort(..., std::greater<ri_chain_t>()) does, writes the indices (into the SORTED array) of
 * the primary chains to kept[] and sets chains[kept[0]].mapq.  Returns the number kept. */
uint32_t rawdtw_gen_primary_chains(rawdtw_chain_t *chains, uint32_t n_chains,
                                   const rawdtw_select_opt_t *opt, uint32_t *kept);
/* is_mapped_with_high_confidence (src/rmap.cpp:594-665) over the primary chains, best first. */
int rawdtw_is_mapped_with_high_confidence(const rawdtw_chain_t *primary, uint32_t n_chains,
                                          const rawdtw_select_opt_t *opt);
/* find_outlier (src/sequence_until.c:4-18): x[point][dim], n dims, m points.  The first form is the source's
 * arithmetic (one rounded product and one rounded add per element, in order; equal bit for bit to the reference
 * file compiled with -ffp-contract=off).  The second is what the reference's default build computes when the
 * compiler has FMA (GCC -O3 -march=native on AVX2 hosts): same order, but elements past the last full group
 * of four are accumulated with one fused multiply-add each; equal bit for bit to that build. */
float rawdtw_find_outlier(const float *const *x, uint32_t n, uint32_t m);
float rawdtw_find_outlier_contracted(const float *const *x, uint32_t n, uint32_t m);

/* ---- sequence-until (RI_M_SEQUENCEUNTIL, rmap.cpp:918-944): the real-time relative-abundance stop, as a state of its own.
 * A record is one read's (mapped, ref_id, fragment_length) as rmap.cpp:750-756 leaves them in reg0; it counts only when it is
 * mapped and ref_id < n_seq.  The counters are uint32_t and wrap as the reference's do (rmap.h:74-76).  Every ttest_freq
 * counted reads past tmin_reads an estimation (float)c / ab_count goes into a ring of tn_samples rows; from the
 * (tn_samples+1)-th estimation on, find_outlier over the ring (rawdtw_find_outlier, or rawdtw_find_outlier_contracted when
 * `contracted`) at or below t_threshold stops the run. ---- */
typedef struct {
    float t_threshold;         /* roptions.c:43 (1.5) */
    uint32_t tn_samples;       /* roptions.c:44 (5) */
    uint32_t ttest_freq;       /* roptions.c:45 (500) */
    uint32_t tmin_reads;       /* roptions.c:46 (500) */
    int contracted;            /* 1: find_outlier as the reference's FMA build computes it */
} rawdtw_su_opt_t;
typedef struct rawdtw_su rawdtw_su;
/* opt NULL: the defaults above.  n_seq, tn_samples or ttest_freq of 0: RAWDTW_ERR_INVALID (the reference divides by zero or
 * writes into calloc(0)). */
int rawdtw_su_create(uint32_t n_seq, const rawdtw_su_opt_t *opt, rawdtw_su **out);
/* n records in read order.  *stop = 0: keep going; k + 1: the test passed at record k (p->su_stop = k+1) and the accounting
 * ends there.  Once stopped, every later call counts nothing and returns the same *stop. */
int rawdtw_su_feed(rawdtw_su *su, uint32_t n, const uint8_t *mapped, const uint32_t *ref_id, const uint32_t *fragment_length,
                   uint32_t *stop);
/* su_nreads, su_nestimations, ab_count and su_c_estimations[n_seq] (any of them may be NULL) */
int rawdtw_su_state(const rawdtw_su *su, uint32_t *n_reads, uint32_t *n_estimations, uint32_t *ab_count, uint32_t *c_estimations);
int rawdtw_su_destroy(rawdtw_su *su);

/* ---- chaining DP of gen_chains (src/rmap.cpp:430-507) and traceback_chains (src/rmap.cpp:130-173) for
 * one (reference sequence, strand): anchors must be sorted by (target_position, query_position) as
 * rmap.cpp:396-401 does.  Emits up to num_best_chains chains; chain k owns
 * out_anchors[out_off[k]..out_off[k+1]) (end-first).  max_chaining_score is the running maximum over
 * all (sequence, strand) pairs of the read and is updated in place (rmap.cpp:431,485-487).
 * Returns the number of chains written, or a negative value when an output array is too small. */
typedef struct {
    int max_gap_length;        /* roptions.c:13 (2000) */
    int max_target_gap_length; /* roptions.c:14 (5000) */
    int chaining_band_length;  /* roptions.c:15 (5000) */
    int max_num_skips;         /* roptions.c:16 (25)   */
    int min_num_anchors;       /* roptions.c:17 (2)    */
    int num_best_chains;       /* roptions.c:18 (3)    */
    float min_chaining_score;  /* roptions.c:19 (10)   */
    int e;                     /* ri->e: events per seed */
    int disable_score_filtering; /* RI_M_DISABLE_CHAININGSCORE_FILTERING */
} rawdtw_chain_opt_t;

typedef struct {
    float chaining_score;
    uint32_t start_position, end_position, n_anchors;
} rawdtw_chain_out_t;

int rawdtw_chain_anchors(const rawdtw_chain_opt_t *opt, const rawdtw_anchor_t *anchors, uint32_t n_anchors,
                         float *max_chaining_score, rawdtw_chain_out_t *out_chains, uint64_t *out_off,
                         rawdtw_anchor_t *out_anchors, uint32_t chains_cap, uint64_t anchors_cap);

/* The evaluation order of one read's chains: the permutation std::sort (libstdc++, unstable)
 * produces for the comparator a.chaining_score > b.chaining_score (rmap.cpp:512). */
int rawdtw_sort_by_chaining_score(const float *chaining_score, uint32_t n_chains, uint32_t *perm_out);
/* The same permutation without std::sort: libstdc++'s introsort restated (rawdtw_sort_order.h: introsort loop with the median-of-three
 * partition, heap sort where the depth budget runs out, one final insertion sort), the function the device's chaining orders a read's
 * chains with under "chain_max_chains".  The function above stays on std::sort and is what this one is tested against.
 * *phases_out (may be NULL): bit 0 a partition ran, bit 1 the heap sort ran. */
int rawdtw_sort_by_chaining_score_restated(const float *chaining_score, uint32_t n_chains, uint32_t *perm_out, uint32_t *phases_out);

/* ---- the same on the device for a whole chunk round (rawdtw_chain.hip): per read the anchor sort
 * (rmap.cpp:396-401), the chaining DP and traceback_chains per (sequence, strand) list (rmap.cpp:430-507, 130-173) with the
 * read's running maximum carried from list to list, and the evaluation order (rmap.cpp:512) -- a wave a read -- and all
 * reads' chains laid out in device memory as ONE candidate batch: what rawdtw_batch_submit_device takes, so the anchors
 * never cross PCIe on their way into the DTW.
 *   in  (host): read r's seeds seeds[seed_off[r] .. seed_off[r+1]), UNSORTED (key = sequence * 2 + strand as the caller numbers
 *        its reference arrays); read_base[r] = the read's first event in the event arena; key_base[key] = the arena offset of
 *        that key's reference array (rawdtw_reference_offset)
 *   out (host): chain_off[n_reads + 1]; anchor_off[n_chains + 1] and recs[n_chains] (at most chains_cap chains; 32 a read -- or "chain_max_chains", below -- is the
 *        device's own limit), chains of a read in evaluation order; anchors[...] (end-first per chain; may be NULL: room for
 *        seed_off[n_reads] entries)
 *   out (device, the context's, valid until its next rawdtw_chain_round): *d_anchors, *d_ref_base, *d_read_base
 * The call returns when the host arrays are filled.  Results equal rawdtw_chain_anchors list by list and
 * rawdtw_sort_by_chaining_score read by read, bit for bit.  RAWDTW_ERR_UNSUPPORTED (the out arrays hold nothing of use): a read with more than
 * 2 048 seeds (with the option below: more than its value), with more than 32 chains, or with more than 16 chains two of which have
 * equal scores (std::sort's order of equal elements is an insertion sort's only up to 16) -- chain that round on the host, or see
 * "chain_max_chains" below, which lifts the last two, and "chain_decline_reads" further down, under which such a read is declined alone.
 * RAWDTW_ERR_INVALID: a chain on a key that is not below n_keys.
 *   rawdtw_set_option(ctx, "chain_long_seeds", N)  0 (the default): as above.  N > 0 (at most 1 << 20): a read with more than 2 048 and at
 *        most N seeds no longer declines the round; it is chained by a second path that keeps its state in device memory (21 bytes a seed
 *        of the context's workspace), with the same results.  A read above N declines the round in _begin, before anything is enqueued;
 *        the limits on chains decline it in _end, as without the option.
 *   rawdtw_chain_round_stats  cumulative, a context: rounds begun, the reads and the seeds that second path chained, and its 64-candidate
 *        steps that read a candidate from device memory because it lay behind the path's window in LDS.  Any pointer may be NULL.
 *   rawdtw_set_option(ctx, "chain_max_chains", N)  0 (the default): as above.  1 <= N <= 4096 (anything else: RAWDTW_ERR_INVALID): a read
 *        with up to N chains no longer declines the round, however many of them have equal scores -- its chains are ordered on the device by
 *        std::sort's own algorithm (rawdtw_sort_by_chaining_score_restated), with the same results.  chains_cap and the out arrays must
 *        then hold min(n_reads * N, seed_off[n_reads] / max(1, min_num_anchors) + 1) chains (chains of a read share no anchor), and the
 *        context's workspace grows by 68 bytes for each of them instead of 64 * 32 bytes a read.
 *        WHAT STILL DECLINES with it (RAWDTW_ERR_UNSUPPORTED from _end): a read with more than N chains; from _begin, as before, a read with
 *        more seeds than 2 048 / "chain_long_seeds".  Further down the flow k_round_end ("device_round_end") leaves a read with more than 64
 *        chains taking part to the host on its own, read by read; that is not this call's limit and does not decline the round.
 *   rawdtw_chain_order_stats  cumulative, a context, over the rounds that were not declined: the reads with more than 32 chains, the reads with
 *        more than 16 chains that "chain_max_chains" ordered with the restated sort (up to 16 it is the insertion sort it always was), and
 *        the most chains a read had.  Any pointer may be NULL. */
typedef struct { uint32_t key, target_position, query_position; } rawdtw_seed_t;                       /* 12 bytes */
typedef struct { float chaining_score; uint32_t key, start_position, end_position, n_anchors; } rawdtw_chain_rec_t; /* 20 bytes */
int rawdtw_chain_round(rawdtw_ctx *ctx, const rawdtw_chain_opt_t *opt, uint64_t n_reads, const uint64_t *seed_off,
                       const rawdtw_seed_t *seeds, const uint32_t *read_base, uint32_t n_keys, const uint64_t *key_base,
                       uint64_t *chain_off, uint64_t *anchor_off, rawdtw_chain_rec_t *recs, uint64_t chains_cap,
                       rawdtw_anchor_t *anchors, const rawdtw_anchor_t **d_anchors, const uint64_t **d_ref_base,
                       const uint32_t **d_read_base);
/* The same in two halves, for a host that has other work while the device chains: _begin enqueues everything (the input
 * arrays must stay as they are until _end) and returns; _end waits and reports.  When chain_off, anchor_off, recs and
 * anchors are page-locked (rawdtw_host_alloc) the device writes them itself and _end is one wait; else they are copied in
 * _end.  One round at a time a context. */
int rawdtw_chain_round_begin(rawdtw_ctx *ctx, const rawdtw_chain_opt_t *opt, uint64_t n_reads, const uint64_t *seed_off,
                             const rawdtw_seed_t *seeds, const uint32_t *read_base, uint32_t n_keys, const uint64_t *key_base,
                             uint64_t *chain_off, uint64_t *anchor_off, rawdtw_chain_rec_t *recs, uint64_t chains_cap,
                             rawdtw_anchor_t *anchors);
int rawdtw_chain_round_end(rawdtw_ctx *ctx, const rawdtw_anchor_t **d_anchors, const uint64_t **d_ref_base,
                           const uint32_t **d_read_base);
int rawdtw_chain_round_stats(const rawdtw_ctx *ctx, uint64_t *rounds, uint64_t *long_reads, uint64_t *long_seeds, uint64_t *far_steps);
int rawdtw_chain_order_stats(const rawdtw_ctx *ctx, uint64_t *reads_above_32, uint64_t *reads_ordered_restated, uint64_t *max_chains_a_read);

/* ---- declining a read, not the round: rawdtw_set_option(ctx, "chain_decline_reads", 1).  0 (the default): everything above, launch for launch.
 * 1 (anything but 0 and 1: RAWDTW_ERR_INVALID): a read the device cannot chain is declined alone -- the rest of the round is chained as before, and
 * rawdtw_chain_round_begin* / _end never return RAWDTW_ERR_UNSUPPORTED (RAWDTW_ERR_RANGE and RAWDTW_ERR_INVALID stay as they are).  A declined read's
 * stretch of chain_off is empty.  The reason is a set of bits: 1 more seeds than 2 048 / "chain_long_seeds" (or than RAWDTW_CHAIN_MAX_SEEDS, the
 * tests' lowered cap), 2 more chains than 32 / "chain_max_chains", 4 more than 16 chains with two equal scores among the first 32 as generated
 * (never with "chain_max_chains").  The caller chains those reads on the host and puts their chains behind the device's own:
 *   rawdtw_chain_round_declined  after a successful _end: the declined reads, ascending, and their reasons -- the context's arrays, valid until
 *        its next chaining begin.  *n_declined = 0 with the option off.  reads / why may be NULL.
 *   rawdtw_chain_round_declined_seeds  the declined reads' seed lists from the device, as the round laid them down (what a resident round's
 *        seeds are made of never was on the host: the kept store, the previous anchors and the hits; a round whose seeds the caller sent up has
 *        them already).  seed_off_out[n_declined + 1] from 0, seeds_out[cap]: written by a kernel, a wave a read, straight into seeds_out when it
 *        is page-locked.  RAWDTW_ERR_RANGE, with the offsets filled, when cap is below seed_off_out[n_declined].
 *   rawdtw_chain_round_append  once a round, n_declined = the round's (anything else: RAWDTW_ERR_INVALID, as is a call after the context's next
 *        begin): the declined reads' chains, read by read in the list's order and each read's in evaluation order -- chain_off[n_declined + 1]
 *        and anchor_off[n_chains + 1] from 0, recs, anchors end-first.  They go up behind the round's chains in the five device arrays
 *        (ref_base from the round's key_base, read_base from the read's).  A round never has more than seed_off[n_reads] / max(1,
 *        min_num_anchors) chains, whoever made them (chains of a read share no anchor), and with the option on the context's workspace is
 *        sized for that (40 bytes for each of them): RAWDTW_ERR_RANGE, with nothing written, for more chains or anchors than that.  Out,
 *        the caller's: chain_off_ext[n_reads + n_declined + 1], the batch's read list -- the round's reads, the declined ones with their
 *        empty stretches, then one pseudo-read for each declined read, in the list's order, which owns its chains --, and
 *        anchor_off_ext[round's chains + n_chains + 1], the round's anchor_off continued (the chain_off and anchor_off _begin was given are
 *        read here and must still be the round's; anchor_off_ext may be that anchor_off itself where it has the room).  The host's recs and
 *        anchors of the appended chains are the caller's own.  rawdtw_batch_submit_device takes n_reads + n_declined reads, chain_off_ext,
 *        anchor_off_ext and the three device pointers, which are those _end gave.
 *   rawdtw_chain_decline_host  no device: which reads of a round the device declines, and why (why_out[n_reads], 0: chained; n_chains_out, may be
 *        NULL: the read's chains, 0 for a read declined for its seeds), from the seed lists, the chaining options and the three caps -- seeds a
 *        read (0: 2 048), "chain_long_seeds" and "chain_max_chains" as the context has them.  Made of rawdtw_chain_anchors, list by list in key
 *        order; what the tests predict the device with, and a debugging aid. */
int rawdtw_chain_round_declined(rawdtw_ctx *ctx, uint64_t *n_declined, const uint32_t **reads, const uint32_t **why);
int rawdtw_chain_round_declined_seeds(rawdtw_ctx *ctx, uint64_t *seed_off_out, rawdtw_seed_t *seeds_out, uint64_t cap);
int rawdtw_chain_round_append(rawdtw_ctx *ctx, uint64_t n_declined, const uint64_t *chain_off, const rawdtw_chain_rec_t *recs,
                              const uint64_t *anchor_off, const rawdtw_anchor_t *anchors, uint64_t *chain_off_ext, uint64_t *anchor_off_ext,
                              const rawdtw_anchor_t **d_anchors, const uint64_t **d_ref_base, const uint32_t **d_read_base);
int rawdtw_chain_decline_host(const rawdtw_chain_opt_t *opt, uint64_t n_reads, const uint64_t *seed_off, const rawdtw_seed_t *seeds,
                              uint32_t seed_cap, uint32_t long_seeds, uint32_t max_chains, uint32_t *why_out, uint32_t *n_chains_out);

/* Batched forms over many reads (what rmap.cpp's per-read worker does for every read of a
 * mini-batch, hoisted around one GPU submission).  Chains are listed read by read, each read's
 * chains already in the reference's evaluation order (std::sort by chaining_score descending,
 * rmap.cpp:512).  chain c owns anchors[anchor_off[c]..anchor_off[c+1]); read r owns chains
 * [chain_off[r], chain_off[r+1]).  ref_base[c]/read_base[c]: arena offsets for chain c.
 * job_off (n_chains+1 entries) is written by build and read by replay. */
int rawdtw_batch_build_jobs(const rawdtw_align_opt_t *opt, uint64_t n_chains, const uint64_t *anchor_off,
                            const rawdtw_anchor_t *anchors, const uint64_t *ref_base,
                            const uint32_t *read_base, uint64_t *job_off, rawdtw_job_t *jobs_out,
                            uint64_t jobs_cap, uint64_t *n_jobs_out);
int rawdtw_batch_replay(const rawdtw_align_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off,
                        const uint64_t *anchor_off, const rawdtw_anchor_t *anchors,
                        const uint64_t *job_off, const float *job_cost, float *score, uint8_t *keep);


/* ---- whole-batch form: the DTW block of gen_chains (rmap.cpp:509-530) for every read of a
 * mini-batch in one submission -- job decomposition on the host, DTW scoring, the align_chain
 * fold and the per-read accept/cut loop all on the device.  Inputs as rawdtw_batch_build_jobs;
 * events and reference arenas must already be set on the ctx.  Outputs per chain: score[c]
 * (chain.alignment_score, -1e10 when cut) and keep[c] (survives dtw_min_score). ---- */
/* rawdtw_batch_create is asynchronous for sparse + banded batches (the default options): it enqueues the copies of the
 * five arrays and the planning kernels on the ctx stream and returns -- no host synchronisation, and no allocation
 * once the context's workspace pool is warm.  Consequences for the caller: the five arrays must stay valid and
 * unchanged until rawdtw_batch_fetch has returned (or the batch is destroyed); an invalid batch (anchors not ascending,
 * a window outside the arenas) is reported by rawdtw_batch_fetch with the status and message rawdtw_plan_create would
 * give.  Other modes (global border constraint, full fill) and "device_plan"=0 plan on the host inside create.
 * The arenas may be re-uploaded or grown between create and run (every run reads the context's current arrays); a run
 * after an arena SHRANK below the size the batch was planned against returns RAWDTW_ERR_INVALID. */
typedef struct rawdtw_batch rawdtw_batch;
int rawdtw_batch_create(rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_reads,
                        const uint64_t *chain_off, const uint64_t *anchor_off,
                        const rawdtw_anchor_t *anchors, const uint64_t *ref_base,
                        const uint32_t *read_base, rawdtw_batch **out);
/* Self-check of a batch's plan (tests, bring-up): downloads the tile records the kernels will read and
 * checks them against `jobs` (the batch's job list as rawdtw_batch_build_jobs gives it): every job in
 * exactly one launch, every window staged inside its tile's LDS image at the right place.
 * *device_planned tells whether the tile class was planned on the device. */
int rawdtw_batch_verify_plan(rawdtw_ctx *ctx, const rawdtw_batch *batch, const rawdtw_job_t *jobs,
                             uint64_t n_jobs, int *device_planned, char *message, uint32_t message_cap);
int rawdtw_batch_info(const rawdtw_batch *batch, rawdtw_plan_info_t *info, uint64_t *n_chains);
int rawdtw_batch_run(rawdtw_ctx *ctx, rawdtw_batch *batch);
/* as rawdtw_plan_run_timed, with two more launches (kinds 6, 7) for fold and select */
int rawdtw_batch_run_timed(rawdtw_ctx *ctx, rawdtw_batch *batch, float *launch_ms,
                           uint32_t *launch_kind, uint32_t cap, uint32_t *n_launches);
/* `reps` back-to-back runs with no host synchronisation in between, one at the end.  When
 * launch_ms != NULL a HIP event pair brackets every launch on the ctx stream and launch_ms[i]
 * receives launch i's MEAN duration over the reps. */
int rawdtw_batch_run_reps(rawdtw_ctx *ctx, rawdtw_batch *batch, uint32_t reps, float *launch_ms,
                          uint32_t *launch_kind, uint32_t cap, uint32_t *n_launches);
/* Pipelined form of the above: enqueue one run without any host synchronisation (with a HIP
 * event pair per launch when timed != 0), call it as often as wanted, also alternating between
 * batches of different contexts so that several mini-batches are in flight (the reference keeps two,
 * rmap.cpp:1033); then, after rawdtw_sync(), collect the mean per-launch durations of all runs
 * enqueued since the last collect.  launch_kind names the launches as rawdtw_batch_launch_stats does (the tile launch that
 * carries the small banded classes as kind 10).  A batch that rawdtw_batch_fetch redid through the job list reports that
 * form's launches and no runs: the timed runs enqueued before timed the form it no longer has. */
int rawdtw_batch_enqueue(rawdtw_ctx *ctx, rawdtw_batch *batch, int timed);
int rawdtw_batch_collect(rawdtw_ctx *ctx, rawdtw_batch *batch, float *launch_ms, uint32_t *launch_kind,
                         uint32_t cap, uint32_t *n_launches, uint32_t *n_runs);
/* static facts about launch i of the batch (same indexing as launch_ms): kind, parameter
 * (band radius / rows per lane / LDS floats), jobs, their algorithmic bytes and DP cells.  Every job and cell is counted in
 * one launch: a sync-free batch's launch 0 is the side list's (kind 8), launch 1 the tiles' passes (kind 10) */
int rawdtw_batch_launch_stats(const rawdtw_batch *batch, uint32_t i, uint32_t *kind, int32_t *param,
                              uint64_t *n_jobs, uint64_t *algorithmic_bytes, uint64_t *cells);
/* job_cost may be NULL; otherwise receives the per-job costs too */
int rawdtw_batch_fetch(rawdtw_ctx *ctx, rawdtw_batch *batch, float *score, uint8_t *keep,
                       float *job_cost);
/* What the hand-over of a batch from device arrays (rawdtw_batch_submit_device, "resident_arrays") that is not planned on the device moved
 * over the link, beside the plan's own records: the job records the device wrote (a local batch: one a chain, k_local_jobs; else 0), the
 * bytes that went up for them (8 a chain of offsets) and the bytes that came home (32 a chain of records -- or, where the anchors are
 * brought home instead, 8 an anchor and 12 a chain of bases).  The environment variable RAWDTW_LOCAL_JOBS=host, read when a context is
 * created, makes a local batch take the second way (tests, A/B measurements). */
int rawdtw_batch_hand_over_stats(const rawdtw_batch *batch, uint64_t *records_on_device, uint64_t *bytes_to_device, uint64_t *bytes_to_host);
/* GPU time of the batch's planning kernels (HIP events; 0 unless the option "time_plan" was set before create): the scan of
 * the anchor list, the side list's class order, the passes' records and copy orders.  The wide bands' launch that goes out
 * between them for the batch's first run is DTW work: rawdtw_batch_wide_ms. */
int rawdtw_batch_plan_ms(rawdtw_ctx *ctx, rawdtw_batch *batch, float *ms);
int rawdtw_batch_wide_ms(rawdtw_ctx *ctx, rawdtw_batch *batch, float *ms);
/* Diagnostics of a device-planned batch (waits for its planning kernels): the planner's counter block (rawdtw_internal.h,
 * StreamCounter).  The layout is the library's own and moves between versions: look a word up by NAME with
 * rawdtw_batch_stream_counter_index -- "bad" first invalid part (~0 none), "overflow" first tile over a capacity (~0 none),
 * "unsupported" parts with a band nobody takes, "side_jobs" side-list entries, "class0" the first of the per-class totals,
 * "cells", "tile_jobs" / "tile_bytes" / "side_bytes" (reporting, filled on request), "todo" listed tiles, "reused" parts
 * taken over from the round before, "pool" passes beyond one a tile, "stamp0" the first of ten phase-stamp words -- which
 * returns -1 for a name it does not know.  *n_out = 0 for a batch planned on the host. */
int rawdtw_batch_stream_counter_index(const char *name);
int rawdtw_batch_stream_counters(rawdtw_ctx *ctx, rawdtw_batch *batch, uint64_t *out, uint32_t cap, uint32_t *n_out);
/* Diagnostics of a device-planned batch (waits for its planning kernels): how the tile launch's waves are filled.  A pass's
 * sorted job records are taken in chunks (sixteen radius-3 records, four lanes a job; then 64 records a wave, the radius-1
 * records from a chunk boundary of their own); a chunk runs the body its radii ask for, for as many columns as its longest
 * job has.  out[4 c .. 4 c + 3] for body class c = 0 quad radius 3, 1 radius 2, 2 radii 1 and 2 mixed, 3 radius 1,
 * 4 generic: jobs, chunks, the sum of the chunks' columns, the sum of the jobs' own columns; out[20] = passes.  Lane
 * occupancy of a class = job columns / (64 (class 0: 16) x chunk columns).  flat_map != 0 counts the chunks cut every
 * 64 records with no boundary at the first radius-1 record (the map of earlier versions), from the same records.
 * *n_out = 0 for a batch planned on the host or declined by the stream path. */
int rawdtw_batch_chunk_profile(rawdtw_ctx *ctx, rawdtw_batch *batch, int flat_map, uint64_t *out, uint32_t cap, uint32_t *n_out);
int rawdtw_batch_destroy(rawdtw_batch *batch);
/* ---- compact hand-over of the anchor lists.  A mini-batch's anchors are its largest array (8 bytes an anchor: as much
 * as the round's new events), and consecutive anchors of a chain differ by little: the chaining DP bounds the gaps
 * (rmap.cpp:456-472, roptions.c:13-15).  The compact form sends, per chain, its first entry whole (= the chain's END:
 * chains are stored end-first, rmap.cpp:193-196) and for every further entry the step back from the entry before it as
 * two bytes (query step, target step), 2 bytes an anchor instead of 8; every RAWDTW_COMPACT_STRIDE-th entry of the flat
 * list is sent whole as well (the decoder works in units of that many); a step of 255 or more in either component is an
 * escape: the entry's two steps are listed in `wide`, ascending by index.  rawdtw_anchors_pack builds the form (pure host
 * code; RAWDTW_ERR_INVALID when a chain's positions do not descend along its list -- such a chain no mapper produces, send
 * the batch with rawdtw_batch_submit -- and RAWDTW_ERR_RANGE when wide_cap is too small, *n_wide then says how many).
 * rawdtw_batch_submit_compact = rawdtw_batch_submit with the lists in that form: they are decoded on the device, inside the
 * scan of the anchor list. ---- */
#define RAWDTW_COMPACT_STRIDE 8192u
typedef struct {
    uint32_t index;                  /* position in the flat anchor list */
    uint32_t query_step, target_step; /* anchors[index - 1] - anchors[index], per component */
} rawdtw_wide_step_t;
int rawdtw_anchors_pack(uint64_t n_chains, const uint64_t *anchor_off, const rawdtw_anchor_t *anchors,
                        rawdtw_anchor_t *heads /* n_chains */, rawdtw_anchor_t *unit_abs /* ceil(n_anchors / STRIDE) */,
                        uint16_t *steps /* n_anchors: query step | target step << 8 */, rawdtw_wide_step_t *wide,
                        uint64_t wide_cap, uint64_t *n_wide);
/* the inverse, on the host (tests; the library's own fallback paths) */
int rawdtw_anchors_unpack(uint64_t n_chains, const uint64_t *anchor_off, const rawdtw_anchor_t *heads,
                          const rawdtw_anchor_t *unit_abs, const uint16_t *steps, const rawdtw_wide_step_t *wide,
                          uint64_t n_wide, rawdtw_anchor_t *anchors_out);
int rawdtw_batch_submit_compact(rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off,
                                const uint64_t *anchor_off, const rawdtw_anchor_t *heads, const rawdtw_anchor_t *unit_abs,
                                const uint16_t *steps, const rawdtw_wide_step_t *wide, uint64_t n_wide,
                                const uint64_t *ref_base, const uint32_t *read_base, rawdtw_batch **out);

/* ---- chunk rounds.  A read is consumed chunk by chunk (rmap.cpp:685-693) and every round re-aligns every surviving chain
 * from scratch over all its anchors (rmap.cpp:516-517), although a part between two anchors that were there the round before
 * has the same operands (events are append-only, rmap.cpp:554-567; the read keeps its place in the event arena) and
 * therefore the same cost.  A chain grows at its END from round to round (rmap.cpp:344-357 re-seeds the chaining with the
 * previous chains' anchors), i.e. at the FRONT of its end-first list: what a chain shares with the chain it continues is a
 * run of leading parts counted from its START = the tail of its list.
 *
 * rawdtw_round_match_chains (pure host code) finds, per chain of the new round, the chain of the round before it continues
 * (same read, same bases, same start anchor, the longest common tail) and VALIDATES the common tail anchor by anchor:
 * carry[c] says how many leading parts are taken over and where their costs lie in the previous batch.  It also packs what
 * the device still needs of the chain's list -- its first n_anchors - (parts + 1) entries (the NEW anchors) followed, when
 * parts > 0, by ONE more entry, the junction (the end anchor of the carried stretch: the new part behind it starts there) --
 * into new_anchors (chain c owns new_anchors[new_off[c] .. new_off[c + 1])).  A part that was not its chain's last then
 * and is now cannot be taken over (exclude_last_element, rmap.cpp:270: there is no exact way back) and is counted out; a part
 * that was the last then and is not now loses its last cell's distance on the device exactly as the DTW functions take it off
 * (dtw.cpp:514-519).
 *
 * rawdtw_batch_submit_carry = rawdtw_batch_submit for such a round.  ONLY the new anchors and the junctions cross the bus, and
 * the device's whole planning and scoring pipeline (scan, side list, passes, DTW launches) runs on that SHORT list -- a carried
 * round costs what its new parts cost; one gather launch then lays every chain's costs out in full (the carried stretch out
 * of `prev`'s cost array, one contiguous copy a chain, then the new parts') for the unchanged fold and accept/cut loop.
 * Results are bit-identical to scoring everything again.  Preconditions (else RAWDTW_ERR_UNSUPPORTED, nothing enqueued:
 * submit the round whole with rawdtw_batch_submit): `prev` is a batch of this context that was scored on the device-planned
 * path with the same options (rawdtw_batch_can_carry tells), has been run and is not destroyed.  carry[] is trusted as
 * rawdtw_round_match_chains wrote it -- the device only checks that the counts add up and stay inside `prev`'s cost array; a
 * caller that invents it gets wrong costs.  `anchor_off` are the offsets of the FULL lists (n_chains + 1 entries); `anchors` the
 * full lists themselves on the host, read only if the batch has to be redone through the job-list path (a band nobody takes,
 * a list over a capacity): they may be NULL, the fetch then fails with RAWDTW_ERR_UNSUPPORTED instead.  All host arrays must
 * stay valid until the batch is fetched; `prev` until this batch is fetched or destroyed (its cost array is read by this
 * batch's gather launch).  rawdtw_batch_round_stats: the parts scored and the parts taken over. ---- */
#define RAWDTW_NO_CHAIN (~(uint64_t)0)
typedef struct {
    uint64_t prev_src;     /* index in the previous batch's (full) anchor list of the carried stretch's first entry; RAWDTW_NO_CHAIN: none */
    uint32_t parts;        /* leading parts (from the chain's start) whose costs are taken over; 0: none */
    uint32_t flags;        /* bit 0: the stretch's first part was its chain's last then and is not now (loses its last cell's distance) */
    rawdtw_anchor_t start; /* the chain's start anchor (the last entry of its full list): the fold's span needs it (rmap.cpp:245) */
} rawdtw_carry_t;
/* read r of the new round is read prev_read[r] of the previous one (or RAWDTW_NO_CHAIN: a new read); new_anchors must have
 * room for anchor_off[n_chains] entries, new_off for n_chains + 1 */
int rawdtw_round_match_chains(uint64_t n_reads, const uint64_t *chain_off, const uint64_t *anchor_off, const rawdtw_anchor_t *anchors,
                              const uint64_t *ref_base, const uint32_t *read_base, const uint64_t *prev_read,
                              const uint64_t *prev_chain_off, const uint64_t *prev_anchor_off, const rawdtw_anchor_t *prev_anchors,
                              const uint64_t *prev_ref_base, const uint32_t *prev_read_base, rawdtw_carry_t *carry, uint64_t *new_off,
                              rawdtw_anchor_t *new_anchors);
/* 1 when `prev` can serve as the previous batch of a rawdtw_batch_submit_carry with options `opt` (waits for nothing; a batch
 * not fetched yet may still turn out declined: the carried batch then falls back by itself) */
int rawdtw_batch_can_carry(const rawdtw_ctx *ctx, const rawdtw_batch *prev, const rawdtw_align_opt_t *opt);
int rawdtw_batch_submit_carry(rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off,
                              const uint64_t *anchor_off, const rawdtw_anchor_t *anchors /* full lists: fallback only, may be NULL */,
                              const uint64_t *new_off, const rawdtw_anchor_t *new_anchors, const uint64_t *ref_base,
                              const uint32_t *read_base, const rawdtw_batch *prev, const rawdtw_carry_t *carry, rawdtw_batch **out);
int rawdtw_batch_round_stats(rawdtw_ctx *ctx, rawdtw_batch *batch, uint64_t *parts_scored, uint64_t *parts_reused);

/* The two calls a pipelined host makes per mini-batch: submit = rawdtw_batch_create +
 * rawdtw_batch_run (everything enqueued, nothing waited for; O(1) host work for sparse + banded batches), and, when the
 * worker's slot comes round again, fetch_destroy = rawdtw_batch_fetch of score / keep + rawdtw_batch_destroy. */
int rawdtw_batch_submit(rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off,
                        const uint64_t *anchor_off, const rawdtw_anchor_t *anchors, const uint64_t *ref_base,
                        const uint32_t *read_base, rawdtw_batch **out);
int rawdtw_batch_fetch_destroy(rawdtw_ctx *ctx, rawdtw_batch *batch, float *score, uint8_t *keep);
/* rawdtw_batch_submit with anchors / ref_base / read_base in DEVICE memory (rawdtw_chain_round's arrays, or the caller's
 * own): used in place, they must stay as they are until the batch is fetched.  chain_off / anchor_off are host arrays. */
int rawdtw_batch_submit_device(rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off,
                               const uint64_t *anchor_off, const rawdtw_anchor_t *d_anchors, const uint64_t *d_ref_base,
                               const uint32_t *d_read_base, rawdtw_batch **out);

/* ---- event detection: detect_events (src/revent.c:190-210), called once a chunk by ri_map_frag (rmap.cpp:551), bit for bit.
 *   prefix sums    revent.c:22-32    fp32, serial in sample order (contracted: the squares' sum with one fmaf a sample)
 *   t-statistics   revent.c:34-75    per window w: all 0 when s_len < 2w or w < 2; else at i in [w, s_len - w] the fp32 means and
 *                                    variance (contracted: two fmaf), fmaxf(var, FLT_MIN), a double sqrt and a double division
 *   peaks          revent.c:77-138   the short (window_length1 / threshold1) and long (window_length2 / threshold2) detectors,
 *                                    whichever window is really shorter; peaks in emission order, never sorted
 *   events         revent.c:140-188  fp32 segment means, double sums in order, (float)((e - mean) / std) (contracted: one fma in the std)
 * No peak: no events (*n = 0, as rmap.cpp:547 starts the count).  s_len == 0 (revent.c:24 asserts), a window above 65 535 (our own
 * bound: the reference's 2 * w_len wraps near 2^31) and offsets that do not ascend strictly: RAWDTW_ERR_INVALID.  A chunk has at most
 * s_len - 1 peaks and at most as many events as peaks, so s_len slots a chunk (events_cap = sig_off[n_chunks]) always suffice. ---- */
typedef struct {
    uint32_t window_length1, window_length2; /* roptions.c:37-38 (3, 6) */
    float threshold1, threshold2;            /* roptions.c:39-40 (4.30265f, 2.57058f) */
    float peak_height;                       /* roptions.c:41 (1.0f) */
    int contracted;                          /* 1: as the reference's Makefile builds revent.c on an FMA host (-O3 -march=native) */
} rawdtw_event_opt_t;                        /* NULL anywhere = these defaults, contracted 0 */

/* host restatement, one chunk: events has room for s_len; *n = 0 when no boundary is found */
int rawdtw_detect_events(const rawdtw_event_opt_t *opt, uint32_t s_len, const float *sig, float *events, uint32_t *n);
/* host, many chunks (chunk k = sig[sig_off[k] .. sig_off[k+1])) on `threads` threads (<= 1: the caller's).  A total above
 * events_cap: RAWDTW_ERR_RANGE with event_off filled and no event written. */
int rawdtw_detect_events_host(const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *sig_off, const float *sig,
                              uint64_t *event_off /* n_chunks+1 */, float *events, uint64_t events_cap, int threads);
/* device, in two halves like rawdtw_chain_round_begin/_end: one detection at a time a context.  _begin checks everything
 * (nothing is enqueued when it refuses), enqueues the upload and the launches on the context's stream and returns; the host
 * arrays must stay valid until _end.  _end waits and fills event_off and events: page-locked ones (rawdtw_host_alloc) the
 * device writes itself, others are copied.  A total above events_cap: RAWDTW_ERR_RANGE from _end with event_off filled; the
 * device checks the total before it writes a single event.  The detection has its own grow-only workspace on the context. */
int rawdtw_detect_begin(rawdtw_ctx *ctx, const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *sig_off,
                        const float *sig, uint64_t *event_off, float *events, uint64_t events_cap);
int rawdtw_detect_end(rawdtw_ctx *ctx, float *kernel_ms /* may be NULL: the launches' device time */);

/* ---- raw signal in: the int16 DAC samples of a signal file to pA, and the outlier filter (ri_read_sig, src/rsig.cpp:216-224),
 * bit for bit.  Per read, with the channel's three numbers as floats (ri_sig_t, src/rsig.h:16):
 *   scale = range / digitisation             one fp32 division
 *   pA    = ((float)raw[i] + offset) * scale one fp32 add, then one fp32 multiply (nothing to contract)
 *   kept  iff pA > 30 && pA < 200            ordered compares: NaN and infinities are dropped
 * sig = the kept pA values in order, l_sig = how many.  A digitisation of 0 and non-finite channel values are not refused:
 * IEEE arithmetic decides, the same on the host and on the device.  The filter runs BEFORE map_worker_for cuts chunks
 * (rmap.cpp:685-690), so a chunk's place in raw positions depends on the data: rawdtw_signal_chunk_table finds it in one pass. ---- */
typedef struct {
    float digitisation, range, offset; /* ri_sig_t dig, ran, offset */
} rawdtw_channel_t;

/* one read on the host.  pa: n_raw slots (the first *l_sig are written), or NULL to count only.  *l_sig = the kept samples. */
int rawdtw_signal_to_pa(const rawdtw_channel_t *ch, uint64_t n_raw, const int16_t *raw, float *pa, uint64_t *l_sig);
/* one pass over a read when it is taken in: *l_sig of the WHOLE read (the PAF line's read length, rmap.cpp:678; what
 * rawdtw_mapper_add_read takes as qlen), *n_chunks = min(max_num_chunk, ceil(l_sig / chunk_size)), and where each chunk begins
 * in raw positions: raw_start[c] = the index of kept sample number c * chunk_size, raw_start[n_chunks] = 1 + the index of the
 * last kept sample of the last chunk (raw_start[0] = 0 when nothing is kept).  The kept samples of
 * raw[raw_start[c] .. raw_start[c+1]) are exactly chunk c.  raw_start has max_num_chunk + 1 slots.  chunk_size 0: INVALID. */
int rawdtw_signal_chunk_table(const rawdtw_channel_t *ch, uint64_t n_raw, const int16_t *raw, uint32_t chunk_size,
                              uint32_t max_num_chunk, uint64_t *l_sig, uint32_t *n_chunks, uint64_t *raw_start);
/* host, many windows on `threads` threads: window k = raw[raw_off[k] .. raw_off[k+1]) with channel chan[k]; its kept pA
 * samples are the chunk, s_len[k] how many (0, an empty or all-outlier window: no events, not an error), events as
 * rawdtw_detect_events_host's.  events_cap = raw_off[n_chunks] - raw_off[0] always suffices. */
int rawdtw_detect_raw_host(const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *raw_off, const int16_t *raw,
                           const rawdtw_channel_t *chan /* n_chunks */, uint32_t *s_len /* n_chunks */,
                           uint64_t *event_off /* n_chunks+1 */, float *events, uint64_t events_cap, int threads);
/* device: rawdtw_detect_begin for raw windows.  The int16 samples go up as they are (2 bytes a sample), are converted,
 * filtered and compacted in order on the device, and the kept samples run through the same detection launches.  One detection
 * at a time a context, of either kind; rawdtw_detect_end ends this one too and fills s_len, event_off and events (page-locked
 * arrays the device writes itself, others are copied).  Refused before anything is enqueued: null arguments, offsets that
 * descend, a window of 2^32 samples or more, a detection already begun, a window length above 65 535.  An EMPTY window
 * (raw_off[k+1] == raw_off[k]) is allowed: s_len 0 and no events. */
int rawdtw_detect_raw_begin(rawdtw_ctx *ctx, const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *raw_off,
                            const int16_t *raw, const rawdtw_channel_t *chan /* n_chunks */, uint32_t *s_len /* n_chunks */,
                            uint64_t *event_off /* n_chunks+1 */, float *events, uint64_t events_cap);

/* ---- the chunk-round mapping loop on the host side of the library: the control flow of map_worker_for / ri_map_frag /
 * gen_chains (src/rmap.cpp:667-822, 545-578, 315-541) turned inside out so that every chunk round makes ONE device
 * submission for all active reads, and the PAF line of a read (src/rmap.cpp:696-801, 950-965).  The caller keeps reading the
 * signal file (the int16 samples and the channel's three numbers: rsig.cpp up to line 215), the calls of event detection
 * (rawdtw_detect_raw_begin on the raw samples, which takes ri_read_sig's pA conversion and outlier filter, rsig.cpp:216-224,
 * with it; rawdtw_signal_chunk_table gives the read's qlen and its chunks' places) and seeding (rsketch.c, rawindex.cpp:
 * rawdtw_seed_begin, or rawdtw_mapper_round_seeded, which seeds the round itself), and
 * hands in, per round and active read, the chunk's events and seed hits; the mapper appends the events to the read's slot in the event arena (rmap.cpp:554-567), re-seeds with the
 * previous chains' anchors (344-357), chains (396-507), orders the chains (512), scores them all in one batch on the
 * device (509-530; with `carry` the unchanged parts' costs are taken over from the round before), and finishes the round:
 * gen_primary_chains, comp_mapq, the stop rule (532-541, 692).  rawdtw_mapper_finish runs the --dtw-output-cigar
 * traceback of every mapped read's best chain (715-717); rawdtw_mapper_paf writes a read's line (mt:f:, wall-clock in
 * the reference, as 0).  The reference arrays must be on the context (rawdtw_upload_reference / rawdtw_index_upload);
 * seq_len[s] is the length of sequence s's signal arrays.  rawalign_amd/mapper.py is the Python mirror. ---- */
typedef struct rawdtw_mapper rawdtw_mapper;
typedef struct {
    int flag;                  /* RI_M_SEQUENCEUNTIL 0x1 | RI_M_DTW_EVALUATE_CHAINS 0x2 | RI_M_DTW_OUTPUT_CIGAR 0x4 | RI_M_DTW_LOG_SCORES 0x8 |
                                  RI_M_OUTPUT_CHAINS 0x20 (roptions.h:9-20) */
    rawdtw_align_opt_t align;
    rawdtw_chain_opt_t chain;
    float min_bestmap_ratio, min_meanmap_ratio; /* roptions.c:28,31 */
    uint32_t min_chain_anchor;                  /* roptions.c:25 */
    uint32_t bp_per_sec, sample_rate, chunk_size, max_num_chunk; /* roptions.c:9-11, 24 */
    uint32_t slot_events;      /* events a read may reach: its slot in the event arena */
    uint32_t max_reads;        /* reads the mapper holds at a time (rawdtw_mapper_release_read gives a finished read's slot back) */
    int carry;                 /* 1: a round takes the unchanged parts' costs over from the round before (rawdtw_batch_submit_carry) */
    uint32_t min_events;       /* roptions.c:23 (50): a chunk with fewer events is appended to the read's events, but the round leaves
                                  the read's chains and its offset alone (rmap.cpp:569-575) */
    int threads;               /* host threads of a round's per-read work (re-seeding, sort, chaining DP, carry matching, primary
                                  chains): the reference runs kt_for over n_threads reads (rmap.cpp:916).  <= 1: the calling thread */
    int groups;                /* 1 or 2 read groups, each on a context of its own (the second is created by the mapper and shares
                                  the reference arena): one group's host phase runs while the other's batch is on the device, as the
                                  reference's two pipeline workers overlap (rmap.cpp:1015,1033) */
    int device_chain;          /* 1: the anchor sort and the chaining DP of a round run on the device too (rawdtw_chain_round) and hand
                                  their chains to the DTW in device memory; the host phase is then the events and the seed lists.  Costs
                                  are not carried in this mode (nothing of the anchor lists crosses PCIe either way).  A round the
                                  device declines is chained on the host: same lines. */
} rawdtw_mapper_opt_t;
typedef struct {
    uint32_t ref_seq;
    int32_t strand;
    uint32_t target_position;
    uint32_t query_position;   /* inside the chunk */
} rawdtw_seed_hit_t;
/* `ctx` may be NULL for a mapper that scores through rawdtw_mapper_set_scorer only (no device is touched then) */
int rawdtw_mapper_create(rawdtw_ctx *ctx, const rawdtw_mapper_opt_t *opt, uint32_t n_seq, const char *const *seq_names,
                         const uint32_t *seq_len, rawdtw_mapper **out);
int rawdtw_mapper_add_read(rawdtw_mapper *m, const char *name, uint32_t qlen /* samples */, uint32_t n_chunks_available,
                           uint32_t *read_id);
/* a finished read whose line has been written: its slot in the event arena goes to the next rawdtw_mapper_add_read */
int rawdtw_mapper_release_read(rawdtw_mapper *m, uint32_t read_id);
/* one chunk round: read read_ids[k] gets events[event_off[k] .. event_off[k+1]) and hits[hit_off[k] .. hit_off[k+1]).
 * All reads are checked before anything changes; when the round fails afterwards (the device or the scorer), the reads and
 * the mapper are put back as they were (a failed round can be repeated). */
int rawdtw_mapper_round(rawdtw_mapper *m, uint32_t n_reads, const uint32_t *read_ids, const uint64_t *event_off,
                        const float *events, const uint64_t *hit_off, const rawdtw_seed_hit_t *hits);
/* (With device_chain and one read group a page-locked `events` array -- rawdtw_host_alloc -- goes to the device as it is, without a
 * copy into the mapper's own staging.) */
int rawdtw_mapper_read_state(const rawdtw_mapper *m, uint32_t read_id, int *finished, uint32_t *chunks_done);
int rawdtw_mapper_finish(rawdtw_mapper *m);
/* --dtw-output-cigar at the reference's default fill.  Off (the default): rawdtw_mapper_finish of a global + banded mapper with flag
 * 0x4 fails with RAWDTW_ERR_UNSUPPORTED as the reference asserts (rmap.cpp:223-225).  On: it takes every mapped read's best chain
 * through rawdtw_banded_traceback_steps ("banded traceback" above) -- the job rawdtw_chain_build_jobs(..., cigar = 0) builds, radius
 * max(1, (int)(n * frac)); from the host's events or, under "signal_cigar", from the arena -- and writes alns:f: from that cost and
 * aln:s: with the global mode's quirk as the full-matrix branch does; a job without a path gives an empty aln:s:.  Sparse and
 * full-matrix mappers are untouched by it.  A setter, not a context option: the option table stays as recorded. */
int rawdtw_mapper_set_banded_cigar(rawdtw_mapper *m, int on);
/* aln:s: made on the device ("aln text" above).  Off (the default): rawdtw_mapper_finish is what it was.  On: where the finish takes
 * the full-matrix traceback (global + full, and sparse; from the host's events or, under "signal_cigar", from the arena) it builds one
 * rec a job -- a sparse part mode 1 with its part's start anchor, a global chain mode 0 with the chain's start anchor --, calls
 * rawdtw_traceback_batch_text / _arena_text with rawdtw_aln_text_bound bytes of room and hands every read its stretch of the text;
 * alns:f: comes from the costs as before.  The tags are byte for byte those of the setter off.  The banded finish
 * (rawdtw_mapper_set_banded_cigar) and the local finish keep the host formatter whatever this says. */
int rawdtw_mapper_set_device_text(rawdtw_mapper *m, int on);
/* *len = the line's length; RAWDTW_ERR_RANGE when buf (cap bytes) is too small for it and its terminator.  With flag 0x20 a
 * mapped line ends in anchors:s: (rmap.cpp:745-747).  A read sequence-until dropped has no line: *len = 0, "". */
int rawdtw_mapper_paf(const rawdtw_mapper *m, uint32_t read_id, char *buf, uint32_t cap, uint32_t *len);
/* ---- sequence-until in the mapper (flag 0x1; the reference's deterministic behaviour, that of one pipeline thread).  The
 * caller closes its mini-batches in input order, every read of a batch finished; the mapper takes each read's record from its
 * final chains (mapped = is_mapped_with_high_confidence, ref_id = chains[0]'s sequence, fragment_length = end - start + 1;
 * unmapped: 0, 0) and feeds them to its own rawdtw_su.  When the test passes at read k of a batch (su_stop = k + 1):
 *   - reads k' < su_stop keep their lines; mapped reads k' >= su_stop get the rmap.cpp:965 form (gated at :960) -- name,
 *     read_length, nine '*', mapq, every tag of the mapped line; unmapped reads keep theirs;
 *   - every read added but not in a closed batch is finished at once (no further rounds) and has no line, as is every read
 *     added afterwards (chunks_done 0): the reference's pipeline ends at step 0 of the next mini-batch (rmap.cpp:885).
 * Slot ids are reused after release_read: the batch's order is the caller's read_ids, never the ids. ---- */
/* the parameters (NULL: the defaults), before the first batch is closed; turns sequence-until on */
int rawdtw_mapper_set_sequence_until(rawdtw_mapper *m, const rawdtw_su_opt_t *opt);
/* close one mini-batch: records, rawdtw_su_feed, rawdtw_mapper_su_apply.  An unknown, released, unfinished or already closed
 * read, or sequence-until off: RAWDTW_ERR_INVALID and nothing changes. */
int rawdtw_mapper_su_batch(rawdtw_mapper *m, uint32_t n, const uint32_t *read_ids, uint32_t *stop);
/* The split form, for a host with the reads of a mini-batch on several ranks: each rank's records, all-gathered and replayed in
 * read order on every rank (rawalign_amd.shard.sequence_until_round), decide the stop, which each rank then applies to its own
 * block of the batch.  batch_records changes nothing.  su_apply closes the block with the decision: first_gated =
 * RAWDTW_SU_NO_STOP, or the stop fired and the block's reads at positions >= first_gated are gated -- 0: the whole block (the
 * stop fell in a block before it), n: none of it (the stop fell at or after its last read), and the run stops all the same.
 * su_batch is batch_records + rawdtw_su_feed + su_apply(stop ? stop : RAWDTW_SU_NO_STOP). */
#define RAWDTW_SU_NO_STOP (~(uint32_t)0)
int rawdtw_mapper_batch_records(const rawdtw_mapper *m, uint32_t n, const uint32_t *read_ids, uint8_t *mapped, uint32_t *ref_id,
                                uint32_t *fragment_length);
int rawdtw_mapper_su_apply(rawdtw_mapper *m, uint32_t n, const uint32_t *read_ids, uint32_t first_gated);
/* *stopped: the stop has fired; *n_mapped_at_stop: the mapped reads of closed batches before the gate -- with su_batch the
 * number the reference's "[M::...] Sequence Until is activated ... %d mapped reads" prints (with su_apply, this rank's share) */
int rawdtw_mapper_su_state(const rawdtw_mapper *m, int *stopped, uint32_t *n_mapped_at_stop);
/* the lines --dtw-log-scores writes to stderr (rmap.cpp:308-312), in order */
int rawdtw_mapper_log(const rawdtw_mapper *m, const char **text);
int rawdtw_mapper_stats(const rawdtw_mapper *m, uint64_t *rounds, uint64_t *parts_scored, uint64_t *parts_reused);
/* where a round's time went, accumulated over the mapper's rounds, in milliseconds of host wall time: 0 the per-read host
 * phase (events, re-seeding, sort, chaining, evaluation order, carry matching), 1 laying the round's arrays out, 2 the
 * submissions (enqueue only), 3 waiting for the device in fetch, 4 the round's end per read (primary chains, MAPQ, stop
 * rule); 5 bytes handed to the device for anchor lists, 6 for events, 7 for everything else (offsets, bases, carry records).
 * With device_chain: 0 = the events and the seed lists (the checks and the round's set-up count here too), 1 = the round's
 * chains per read out of the arrays the device wrote, 2 = the submissions and the wait for the device's sort + DP, 5 = 0 (no
 * anchor list goes up), 7 includes the seed lists. */
int rawdtw_mapper_timing(const rawdtw_mapper *m, double out[8]);
/* Harness hook: score a round's chains with `fn` instead of on the device -- for timing or checking the SAME control flow
 * with another DTW implementation (bench.py's cpu_baseline, the CPU-only tests).  fn receives the round's chains read by
 * read, each read's chains in evaluation order (rmap.cpp:512), and must write score[c] / keep[c] for every chain exactly as
 * the DTW block of gen_chains would (rmap.cpp:515-524); a non-zero return fails the round.  The product's own path never
 * sets one. */
typedef int (*rawdtw_scorer_fn)(void *user, uint64_t n_reads, const uint64_t *chain_off, const uint64_t *anchor_off,
                                const rawdtw_anchor_t *anchors, const uint32_t *chain_seq, const int32_t *chain_strand,
                                const float *const *read_events, const uint32_t *read_n_events, float *score, uint8_t *keep);
int rawdtw_mapper_set_scorer(rawdtw_mapper *m, rawdtw_scorer_fn fn, void *user);
const char *rawdtw_mapper_last_error(const rawdtw_mapper *m);
int rawdtw_mapper_destroy(rawdtw_mapper *m);

/* ---- seeding: a chunk's events to seed hits -- ri_sketch (src/rsketch.c:276-284) followed by ri_idx_get
 * (src/rawindex.cpp:256-273), as gen_chains calls them (src/rmap.cpp:364-391) -- bit for bit and in the reference's order.
 *   sketch, w == 0  rsketch.c:223-274  event i is skipped when i > 0 && fabs(ev[i] - ev[last kept]) < 0.3F (an fp32 subtraction,
 *                                      an ordered compare: a NaN is kept, and so is the event after it) or ev[i] ==
 *                                      RI_MASK_SIGNAL; a kept event's code is its sign and top exponent bit followed by lq
 *                                      bits from bit 32 - q down; the last e codes, (lq + 2) bits each, are hashed with hash64
 *                                      under the 32-bit mask (rsketch.c:6-15); from the e-th kept event on, every kept event
 *                                      emits (hash, i), i = the position of the LAST event of the e-mer
 *   sketch, w > 0   rsketch.c:146-221  the minimizer sketch: no RI_MASK_SIGNAL test, the position is the e-mer's first event,
 *                                      and of each window of w e-mers the smallest hash is emitted (ties and the first window
 *                                      as rsketch.c:193-219 has them).  On the host; on the device under "seed_minimizer" (below).
 *   lookup          rmap.cpp:371-391   per sketch element in order, per position y of its hash in the index's order:
 *                                      ref_seq = y >> 32, strand = y & 1, target_position = (y >> 1) & 0x7fffffff,
 *                                      query_position = i (inside the chunk; the mapper adds the chunk's start)
 * There is no occurrence cap (rmap.cpp:368 is commented out).  Refused with RAWDTW_ERR_INVALID: e outside 2..9 (rsketch.c:278
 * asserts), w >= 256 (rsketch.c:154), q == 0 or q > 32, lq > 30 and (lq + 2) * e >= 64 (the reference's shifts are undefined
 * there).  A chunk with fewer than e kept events, an empty one included, has no hits. ---- */
typedef struct {
    uint32_t w, e, n, q, lq, k; /* ri_idx_t's, the order of the .ind header (rawindex.cpp:279) */
} rawdtw_seed_pars_t;
typedef struct rawdtw_seed_index rawdtw_seed_index;
/* the index of ri_idx_add / ri_idx_sort (rawindex.cpp:91-97, 194-246) from signal arrays: both strands of every sequence are
 * sketched, forward with strand bit 1 and reverse with strand bit 0 (rawindex.cpp:141-147); a hash's positions
 * id << 32 | pos << 1 | strand are kept in ascending order (radix_sort_64, rawindex.cpp:233).  `threads` sketches sequences in
 * parallel; the result never depends on it. */
int rawdtw_seed_index_build(uint32_t n_seq, const float *const *fwd, const float *const *rev, const uint32_t *len,
                            const rawdtw_seed_pars_t *pars, int threads, rawdtw_seed_index **out);
/* the same from the hash buckets of a .ind file (rawindex.cpp:297-312, 354-374): 2^14 buckets (ri_idx_load always uses b = 14),
 * each u32 n, n x u64 positions, u32 size, size x (u64 key, u64 val); hash = (key >> 1) << 14 | bucket; key & 1: val is the one
 * position, else val = start << 32 | count into the bucket's positions.  A short file, a list outside its bucket, a hash above
 * 32 bits or one listed twice: RAWDTW_ERR_INVALID. */
int rawdtw_seed_index_load(const rawdtw_index *idx, rawdtw_seed_index **out);
/* ri_idx_get: *pos (valid while the index lives) and *n, 0 for a hash the index does not hold */
int rawdtw_seed_index_get(const rawdtw_seed_index *six, uint64_t hash, const uint64_t **pos, uint32_t *n);
int rawdtw_seed_index_info(const rawdtw_seed_index *six, uint32_t *n_seq, uint64_t *n_keys, uint64_t *n_positions,
                           uint64_t *table_bytes, rawdtw_seed_pars_t *pars);
/* every hash the index holds, in table order (tests, and the writer of a .ind file's buckets); hashes has room for n_keys */
int rawdtw_seed_index_keys(const rawdtw_seed_index *six, uint32_t *hashes);
int rawdtw_seed_index_destroy(rawdtw_seed_index *six);
/* ri_sketch for one chunk: hash_out and pos_out have room for n entries */
int rawdtw_seed_sketch(const rawdtw_seed_pars_t *pars, const float *events, uint32_t n, uint32_t *hash_out, uint32_t *pos_out,
                       uint32_t *n_out);
/* host, many chunks (chunk k = events[event_off[k] .. event_off[k+1]), which may be empty) on `threads` threads, a thread whole
 * chunks: chunk k's hits are hits[hit_off[k] .. hit_off[k+1]).  A total above hits_cap: RAWDTW_ERR_RANGE with hit_off filled and
 * no hit written. */
int rawdtw_seed_hits_host(const rawdtw_seed_index *six, uint32_t n_chunks, const uint64_t *event_off, const float *events,
                          uint64_t *hit_off /* n_chunks+1 */, rawdtw_seed_hit_t *hits, uint64_t hits_cap, int threads);
/* device.  _upload puts the index's table into the context's device memory (it replaces an earlier one and is freed with the
 * context; the index may be destroyed afterwards; an index is known by a serial number of its own, never by its address, and
 * uploading the one that is there already does nothing).  _begin / _end are the two halves, as rawdtw_detect_begin / _end: one seeding
 * at a time a context, with its own grow-only workspace; _begin checks everything (nothing is enqueued when it refuses) and
 * returns, the arrays must stay valid until _end; page-locked hit_off / hits (rawdtw_host_alloc) the device writes itself, others
 * are copied in _end (through a device array of hits_cap entries: keep hits_cap near the need).  A total above hits_cap:
 * RAWDTW_ERR_RANGE from _end with hit_off filled; the device checks the total before it writes a single hit.  An index with
 * w > 0 is RAWDTW_ERR_UNSUPPORTED from _begin (seed such chunks with rawdtw_seed_hits_host) unless "seed_minimizer" is on; no
 * table on the context is RAWDTW_ERR_INVALID.  No w == 0 input is declined for its size or its repeats.
 *   rawdtw_set_option(ctx, "seed_minimizer", V)  0 (the default): as above.  1: a w > 0 table on this context is seeded on the device
 *        (a further launch between the filter and the probe runs the reference's window over every chunk, rsketch.c:193-219; 32
 *        bytes of workspace an event instead of 24) by rawdtw_seed_begin / _end, rawdtw_seed_resident_begin / _end / _fetch, and by
 *        rawdtw_mapper_round_seeded / _seeded_resident of a mapper on this context: the same hits as rawdtw_seed_hits_host, in
 *        its order.  It never changes what a w == 0 table does.  rawdtw_get_option reads it back.  A chunk whose sketch had more
 *        elements than the chunk has events (an e-mer can be emitted twice; not seen on any input) is RAWDTW_ERR_UNSUPPORTED from
 *        _end with no hit written and hit_off not to be used: seed that round with rawdtw_seed_hits_host. */
int rawdtw_seed_index_upload(rawdtw_ctx *ctx, const rawdtw_seed_index *six);
int rawdtw_seed_begin(rawdtw_ctx *ctx, uint32_t n_chunks, const uint64_t *event_off, const float *events,
                      uint64_t *hit_off /* n_chunks+1 */, rawdtw_seed_hit_t *hits, uint64_t hits_cap);
int rawdtw_seed_end(rawdtw_ctx *ctx, float *kernel_ms /* may be NULL: the launches' device time */);
/* rawdtw_mapper_round with the seeding in front of it: the round's hits come from `six` instead of from the caller (the lines
 * of gen_chains a host would otherwise keep, rmap.cpp:364-391), then the unchanged rawdtw_mapper_round runs on them.  A mapper
 * with a context seeds on the device (the table of `six` is uploaded at the first round and whenever the context holds another index's; the
 * whole round is seeded on the mapper's own context, whichever group a read belongs to, so a second group needs no table) into
 * a page-locked buffer of its own; a mapper without one (a scorer's), and an index with
 * w > 0 unless the context's "seed_minimizer" option is on, seed on the host with opt.threads.  `six` must hold as many sequences as the mapper (RAWDTW_ERR_INVALID).  A failed
 * seeding changes nothing in the mapper. */
int rawdtw_mapper_round_seeded(rawdtw_mapper *m, const rawdtw_seed_index *six, uint32_t n_reads, const uint32_t *read_ids,
                               const uint64_t *event_off, const float *events);

/* ---- a chunk round whose seed hits stay on the device.  rawdtw_mapper_round_seeded brings every hit home (16 bytes) and sends it
 * up again as a seed (12 bytes), although the chaining reads its seeds on the device; the entries below leave the hits where the
 * seeding found them.
 *   rawdtw_seed_resident_begin / _end  rawdtw_seed_begin / _end on events that are in the context's event arena already (after the
 *       round's rawdtw_events_append: nothing goes up twice): chunk k is the arena's ev_len[k] events from ev_start[k].  Only
 *       hit_off (n_chunks + 1 entries, 8 bytes a chunk) comes home; the hits stay in the seeding's workspace until the context's
 *       next seeding of either kind, or its next rawdtw_seed_index_upload of another index.  The rules are rawdtw_seed_begin's:
 *       refused before anything is enqueued, one seeding a context at a time (of either kind; a resident one is ended by
 *       rawdtw_seed_resident_end only), w > 0 RAWDTW_ERR_UNSUPPORTED unless "seed_minimizer" is on, no table RAWDTW_ERR_INVALID, a chunk outside the arena
 *       RAWDTW_ERR_RANGE, 64-bit counts.
 *   rawdtw_seed_resident_fetch  the ended resident seeding's hits into hits[0 .. hit_off[n_chunks]), in rawdtw_seed_begin's order
 *       (page-locked: written by the device itself); RAWDTW_ERR_RANGE when hits_cap is below the total.  For fall-backs and tests.
 *   rawdtw_chain_round_begin_resident  rawdtw_chain_round_begin without a seed list from the host: read r's seeds are its previous
 *       chains' anchors prev_seeds[prev_off[r] .. prev_off[r+1]) (host, small) followed by chunk r's hits of the ended resident
 *       seeding as {ref_seq * 2 + strand, target_position, query_position + chunk_start[r]} (rmap.cpp:385-391), written on the device
 *       into seed_off[r] ..; a read with sits_out[r] != 0 (its chunk is below min_events, rmap.cpp:569-572) gets nothing and must
 *       have an empty stretch and no previous seeds.  RAWDTW_ERR_INVALID: no ended resident seeding, n_reads other than its
 *       chunks, or a seed_off stretch that is not previous + hits.  Caps, RAWDTW_ERR_UNSUPPORTED and rawdtw_chain_round_end as for
 *       rawdtw_chain_round_begin -- with "chain_long_seeds" at N a read of more than 2 048 and at most N seeds is chained on the device
 *       here too, from the seeds the device laid down, and only a read above N declines the round; the arrays must stay valid until _end.
 *   rawdtw_mapper_round_seeded_resident  rawdtw_mapper_round_seeded through the three above: append the events, seed from the
 *       arena, size the round by hit_off, chain, and from there the unchanged round.  Only for a mapper that chains on the
 *       device (device_chain, a context, no scorer; with or without a DTW stage) with one read group and a w == 0 index (or a w > 0 one
 *       with "seed_minimizer" on on that context): anything else is
 *       RAWDTW_ERR_UNSUPPORTED with nothing changed (use rawdtw_mapper_round_seeded).  A round the device chaining declines (its
 *       caps) fetches the hits once and is chained on the host: the same lines.  A failed round leaves the mapper as it was.
 *   rawdtw_mapper_resident_stats  rounds that stayed resident, rounds that fell back, bytes of hits fetched to the host (16 a hit
 *       of the fall-back rounds), bytes of seeds sent up (12 a previous anchor of the resident rounds).  Any pointer may be NULL. ---- */
int rawdtw_seed_resident_begin(rawdtw_ctx *ctx, uint32_t n_chunks, const uint64_t *ev_start, const uint32_t *ev_len,
                               uint64_t *hit_off /* n_chunks+1 */);
int rawdtw_seed_resident_end(rawdtw_ctx *ctx, float *kernel_ms /* may be NULL */);
int rawdtw_seed_resident_fetch(rawdtw_ctx *ctx, rawdtw_seed_hit_t *hits, uint64_t hits_cap);
int rawdtw_chain_round_begin_resident(rawdtw_ctx *ctx, const rawdtw_chain_opt_t *opt, uint64_t n_reads, const uint64_t *seed_off,
                                      const uint64_t *prev_off, const rawdtw_seed_t *prev_seeds, const uint32_t *chunk_start,
                                      const uint8_t *sits_out, const uint32_t *read_base, uint32_t n_keys, const uint64_t *key_base,
                                      uint64_t *chain_off, uint64_t *anchor_off, rawdtw_chain_rec_t *recs, uint64_t chains_cap,
                                      rawdtw_anchor_t *anchors);
int rawdtw_mapper_round_seeded_resident(rawdtw_mapper *m, const rawdtw_seed_index *six, uint32_t n_reads, const uint32_t *read_ids,
                                        const uint64_t *event_off, const float *events);
int rawdtw_mapper_resident_stats(const rawdtw_mapper *m, uint64_t *resident_rounds, uint64_t *fallback_rounds,
                                 uint64_t *hit_bytes_to_host, uint64_t *seed_bytes_to_device);

/* ---- a chunk round from signal: the events never leave the device.  A caller of rawdtw_mapper_round_seeded_resident still brings every
 * event home from the detection and sends it up again; the entries below run detection, seeding and chaining one behind the other on the
 * context's stream, and what comes home is 4 bytes a chunk (its event count) and the hit offsets.
 *   rawdtw_detect_resident_begin / rawdtw_detect_raw_resident_begin  rawdtw_detect_begin / rawdtw_detect_raw_begin with the events'
 *       destination in the context's event arena (the library's own after rawdtw_events_reserve, or the caller's after
 *       rawdtw_set_events_device): chunk k's normalised events go to the arena at dst_start[k] .., at most room[k] of them.  The write is
 *       all or nothing and decided on the device before a single event is written: when any chunk has more events than its room, or the
 *       total is above events_cap, nothing is written anywhere and _end returns RAWDTW_ERR_RANGE (its message says which).  Refused before
 *       anything is enqueued: RAWDTW_ERR_INVALID for a null argument, no arena on the context, a detection of any kind already begun, and
 *       the plain entries' rules on offsets and window lengths -- except that an EMPTY window is allowed in both (ev_len 0, nothing
 *       written; so is an all-outlier raw window); RAWDTW_ERR_RANGE for dst_start[k] + room[k] beyond the arena.  One detection at a time
 *       a context, of any of the four kinds.
 *   rawdtw_detect_resident_end  waits for the detection's own work and fills ev_len (n_chunks counts), *total and, when s_len is not NULL,
 *       the samples a chunk kept (the window's length for the pA entry); also when it returns RAWDTW_ERR_RANGE.  No event comes home.  The
 *       dense offsets and the counts stay in the detection's workspace.  rawdtw_detect_end does not end a resident detection, nor this a
 *       plain one (RAWDTW_ERR_INVALID, the detection stays begun).
 *   rawdtw_seed_detected_begin  valid while a resident detection is begun and not ended on the context: rawdtw_seed_resident_begin on
 *       that detection's chunks, enqueued directly behind it with no host step between -- the offsets and the places are the detection's,
 *       on the device; the workspace is sized by the detection's events_cap (24 bytes an event, 32 with w > 0), for no count has come home.
 *       The rules are rawdtw_seed_resident_begin's.  rawdtw_seed_resident_end ends it (in either order with rawdtw_detect_resident_end):
 *       RAWDTW_ERR_RANGE when the detection declined -- every launch of the seeding then did nothing, and hit_off is not to be used --,
 *       RAWDTW_ERR_UNSUPPORTED for the minimizer overflow as before; rawdtw_seed_resident_fetch and rawdtw_chain_round_begin_resident
 *       work on the retained hits unchanged.
 *   rawdtw_mapper_round_signal_resident / rawdtw_mapper_round_raw_resident  one chunk round from the signal itself: window k (pA samples
 *       sig[sig_off[k] .. sig_off[k+1]), or int16 samples raw[raw_off[k] .. raw_off[k+1]) with channel chan[k], cut with
 *       rawdtw_signal_chunk_table) is read read_ids[k]'s next chunk; ev_opt NULL = the defaults.  The chunk's events are detected into the
 *       read's slot behind its committed events, seeded there, and the round goes on as rawdtw_mapper_round_seeded_resident's from the hit
 *       counts on (a round the device chaining declines fetches the hits -- not the events -- and is chained on the host: same lines).
 *       One upload (the samples), one launch sequence and one wait in front of the chaining.  Preconditions: those of
 *       rawdtw_mapper_round_seeded_resident, and nothing may read the host's copy of a read's events later -- no --dtw-output-cigar
 *       (flag 0x4; rawdtw_mapper_finish uploads that copy -- unless "signal_cigar" below is on) and no external scorer, neither then nor afterwards (rawdtw_mapper_set_scorer is
 *       refused once such a round has run); a mapper with no DTW stage is served.  Anything else: RAWDTW_ERR_UNSUPPORTED with nothing
 *       changed (rawdtw_detect_raw_begin + rawdtw_mapper_round_seeded_resident map the round).  events_cap is the mapper's guess -- what
 *       the seeding's workspace holds already, or a quarter of the round's samples + 1 024 --, and a round with more events runs once more
 *       with the total the device reported.  A chunk that does not fit its read's slot: RAWDTW_ERR_RANGE, "a read outgrew its slot in the
 *       event arena".  A failed round leaves reads and mapper as they were; what the device wrote above a read's committed events is
 *       scratch and overwritten by the next attempt.
 *   rawdtw_set_option(ctx, "signal_events_cap", N)  N > 0: the first try's events_cap of the mapper's rounds from signal on this context
 *       (tests of the retry); 0, the default: the guess.  rawdtw_get_option reads it back.
 *   rawdtw_set_option(ctx, "signal_cigar", 0 | 1)  opt-in, default 0 (any other value: RAWDTW_ERR_INVALID); read once a round, and read
 *       back by rawdtw_get_option.  1: the two rounds from signal no longer refuse a mapper for flag 0x4 (--dtw-output-cigar) alone --
 *       every other refusal stays, an external scorer set later included.  Once such a round is committed, rawdtw_mapper_finish takes
 *       EVERY mapped read's events from its slot of the arena (a context mapper's rounds of every kind put them there): the jobs are built
 *       over the slot's base and go to rawdtw_traceback_arena_steps; the arena is not replaced, no event is uploaded and
 *       event_bytes_crossed stays what it was.  On any other mapper, whatever the option says, rawdtw_mapper_finish is unchanged.  The
 *       one thing it cannot serve: a read that got events in a round of a mapper without a DTW stage chained on the host (those never
 *       reach the arena) -- RAWDTW_ERR_UNSUPPORTED from rawdtw_mapper_finish, nothing changed.
 *   rawdtw_mapper_read_events  read read_id's committed events: from its slot of the arena through rawdtw_events_fetch on a mapper with a
 *       context, from the host's copy otherwise (also after a rawdtw_mapper_finish that uploaded the host's copies over the arena, and for
 *       a read with events from a round that ran nothing on the device).  *n is always written with their number (0 for a read with no round yet);
 *       cap < *n: RAWDTW_ERR_RANGE, out untouched.  out may be NULL when cap is 0.
 *   rawdtw_mapper_signal_stats  rounds from signal that were committed, how many of them ran twice, bytes of samples sent up (both tries
 *       of a retried round), and the bytes of events that crossed PCIe in either direction over all of the mapper's rounds (what
 *       rawdtw_mapper_timing's slot 6 counts: 0 for a mapper that only ran rounds from signal).  Any pointer may be NULL. ---- */
int rawdtw_detect_resident_begin(rawdtw_ctx *ctx, const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *sig_off,
                                 const float *sig, const uint64_t *dst_start /* n_chunks */, const uint32_t *room /* n_chunks */,
                                 uint64_t events_cap);
int rawdtw_detect_raw_resident_begin(rawdtw_ctx *ctx, const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *raw_off,
                                     const int16_t *raw, const rawdtw_channel_t *chan /* n_chunks */,
                                     const uint64_t *dst_start /* n_chunks */, const uint32_t *room /* n_chunks */, uint64_t events_cap);
int rawdtw_detect_resident_end(rawdtw_ctx *ctx, uint32_t *s_len /* n_chunks, may be NULL */, uint32_t *ev_len /* n_chunks */,
                               uint64_t *total, float *kernel_ms /* may be NULL */);
int rawdtw_seed_detected_begin(rawdtw_ctx *ctx, uint64_t *hit_off /* n_chunks+1 */);
int rawdtw_mapper_round_signal_resident(rawdtw_mapper *m, const rawdtw_seed_index *six, const rawdtw_event_opt_t *ev_opt,
                                        uint32_t n_reads, const uint32_t *read_ids, const uint64_t *sig_off, const float *sig);
int rawdtw_mapper_round_raw_resident(rawdtw_mapper *m, const rawdtw_seed_index *six, const rawdtw_event_opt_t *ev_opt, uint32_t n_reads,
                                     const uint32_t *read_ids, const uint64_t *raw_off, const int16_t *raw,
                                     const rawdtw_channel_t *chan /* n_reads */);
int rawdtw_mapper_signal_stats(const rawdtw_mapper *m, uint64_t *rounds, uint64_t *retried_rounds, uint64_t *sample_bytes_to_device,
                               uint64_t *event_bytes_crossed);
int rawdtw_mapper_read_events(rawdtw_mapper *m, uint32_t read_id, float *out, uint32_t cap, uint32_t *n);

/* ---- a round's end for all its reads at once: gen_primary_chains (rmap.cpp:90-128, comparator rmap.h:41-45), comp_mapq (65-88) and
 * is_mapped_with_high_confidence (594-665) -- the three steps between a batch's score / keep and "this read is finished".
 * Read r's candidates are its chains in evaluation order, [chain_off[r], chain_off[r+1]); recs[c].key = sequence * 2 + strand;
 * score[c] / keep[c] are rawdtw_batch_fetch's (score[c] is the chain's alignment_score whatever the flags; keep may be NULL without
 * evaluate_chains).  Chain c takes part when !opt->evaluate_chains || keep[c] (rmap.cpp:525).
 *   out[r].n_primary            the read's primary chains
 *   primary[chain_off[r] + k]   k < n_primary: the index within the read of the k-th primary chain, best first; RAWDTW_NO_PRIMARY behind them
 *   out[r].mapq                 comp_mapq's value for the first primary chain
 *   out[r].flags                bit 0: mapped with high confidence; bit 1: declined (device forms only; the other outputs are void)
 * A read with no chain taking part reads {0, 0, 0}.
 *   rawdtw_round_end_host        the batched restatement over rawdtw_gen_primary_chains and rawdtw_is_mapped_with_high_confidence.  Never
 *        declines: the fall-back for declined reads (a read at a time: n_reads = 1, chain_off + r, out + r, the other arrays as they are)
 *        and what the device forms are tested against, bit for bit.
 *   rawdtw_round_end             the host arrays go up, one launch (a wave a read, a lane a candidate), the results come home.
 *   rawdtw_batch_round_end_begin enqueued on the batch's stream behind its last run: reads the batch's score, keep and chain offsets where
 *        they lie in device memory.  `recs`: a host array (copied up) or, with recs_on_device, a device array of the batch's n_chains
 *        records that stays as it is until _fetch (rawdtw_chain_round_recs gives the chaining workspace's).  One round end at a time a context.
 *   rawdtw_batch_round_end_fetch waits and copies out[n_reads] and primary[n_chains] home.  A batch the device-planned path declined is
 *        scored again through the job list first (as rawdtw_batch_fetch does) and its round end runs again on those scores.
 *   rawdtw_chain_round_recs      the device address of the context's ended chaining round's recs (valid until its next chaining round).
 * A read is declined -- the caller runs rawdtw_round_end_host on it alone; a declined read never declines the round -- when
 *   - more than 64 of its chains take part;
 *   - two chains taking part are equal on all seven keys (std::sort's choice between them is not the comparator's, and it decides
 *     whose anchors survive);
 *   - a chaining or alignment score of a chain taking part is NaN;
 *   - a quotient that is evaluated -- comp_mapq's s1 / s0, the stop rule's s0 / s1 -- is not finite, or comp_mapq's product
 *     40 * (1 - s1 / s0) is not in [-2^31, 2^31) (the host's conversion to int there is x86's, the device's saturates).
 * The arithmetic is fp32 with IEEE division, no contraction, denormals kept; the stop rule's mean is a serial sum in primary order.
 *   rawdtw_set_option(ctx, "device_round_end", 1)  on the context a mapper was created with: its rounds that are chained on the device
 *        and run the DTW enqueue the round end behind rawdtw_batch_submit_device and take primary, mapq and the stop rule's answer
 *        from it; reads that sat the round out and declined reads end on the host as before.  0 (the default): no such call is made.
 *        Lines and logs are the same either way.  rawdtw_get_option reads it back.
 *   rawdtw_get_option(ctx, "round_end_kernel_us")  read-only: the launch of the context's most recently FETCHED round end between its
 *        HIP events, in microseconds; 0 before any.  (What scripts/round_end_probe.py reports as the kernel's time.)
 * n_reads == 0: rawdtw_round_end_host and rawdtw_round_end return RAWDTW_OK and do nothing; a batch without reads has no round end
 * (rawdtw_batch_round_end_begin: RAWDTW_ERR_INVALID).  A batch destroyed between _begin and _fetch takes its round end with it: the
 * launch is waited for, its results are dropped, and the context is free for the next round end.
 *   rawdtw_mapper_round_end_stats  committed rounds that used it, the reads it ended, the reads it declined.  Any pointer may be NULL. ---- */
typedef struct { uint32_t n_primary, mapq, flags; } rawdtw_round_out_t;
#define RAWDTW_ROUND_HIGH 1u
#define RAWDTW_ROUND_DECLINED 2u
#define RAWDTW_NO_PRIMARY 0xffffffffu
int rawdtw_round_end_host(const rawdtw_select_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off, const rawdtw_chain_rec_t *recs,
                          const float *score, const uint8_t *keep, rawdtw_round_out_t *out, uint32_t *primary);
int rawdtw_round_end(rawdtw_ctx *ctx, const rawdtw_select_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off,
                     const rawdtw_chain_rec_t *recs, const float *score, const uint8_t *keep, rawdtw_round_out_t *out, uint32_t *primary);
int rawdtw_batch_round_end_begin(rawdtw_ctx *ctx, rawdtw_batch *batch, const rawdtw_select_opt_t *opt, const rawdtw_chain_rec_t *recs,
                                 int recs_on_device);
int rawdtw_batch_round_end_fetch(rawdtw_ctx *ctx, rawdtw_batch *batch, rawdtw_round_out_t *out, uint32_t *primary);
int rawdtw_chain_round_recs(rawdtw_ctx *ctx, const rawdtw_chain_rec_t **d_recs);
int rawdtw_mapper_round_end_stats(const rawdtw_mapper *m, uint64_t *rounds, uint64_t *reads_device, uint64_t *reads_declined);

/* ---- the kept chains: a round's primary chains stay on the device as the next round's previous seeds.  gen_chains re-seeds a round with
 * the anchors of the chains the read kept from the round before (rmap.cpp:344-357); a round that ends on the device has them in the
 * chaining workspace and knows which are primary, so they need not come up from the host again (12 bytes each).
 * THE STORE, one a context: n_slots x 2 halves of N rawdtw_seed_t each and one uint32_t count a half.  A store address is slot * 2 + half.
 * Two halves a slot, so that a round writes the half a read is NOT seeded from and a failed round leaves the other as it was.
 *   rawdtw_chain_keep_reserve     grow-only: at least n_slots slots of at least seeds_per_half (1 .. 2^20) seeds.  A store that grows loses
 *        its contents (every half reads RAWDTW_NOT_KEPT again); RAWDTW_ERR_OOM with nothing changed when the allocation fails; freed with
 *        the context.
 * WHAT IS KEPT for read r (its primary chains p = 0 .. out[r].n_primary - 1, best first; chain c = chain_off[r] + primary[chain_off[r] + p]):
 * the chains one after the other, each chain's anchors in the order they lie, as {recs[c].key, target_position, query_position} -- the
 * list the mapper builds from a read's chains for the next round.  Nothing is kept and the count reads RAWDTW_NOT_KEPT for a read the
 * round end declined (RAWDTW_ROUND_DECLINED), a read whose total is above the cap (N), and a read with dst[r] == RAWDTW_NO_KEEP; such a
 * half's seeds are left as they are.  A read without a primary chain keeps a count of 0.
 *   rawdtw_round_keep_host        the host restatement, what the device forms are tested against byte for byte: kept_count[n_reads],
 *        seed_off_out[n_reads + 1] and the kept reads' seeds, dense, in seeds_out (room for every anchor of the round; NULL: counts and
 *        offsets only).  RAWDTW_ERR_INVALID for a null argument, offsets that descend, or a primary index outside its read.
 *   rawdtw_round_keep             the host arrays go up, one launch (a wave a read), kept_count[n_reads] comes home; read r's seeds go to
 *        the store's half dst[r].  For tests on constructed rounds.  RAWDTW_ERR_INVALID as the host form, and for no store, a dst outside
 *        it, the same address twice, or a chain whose anchor_off stretch is not its n_anchors.
 *   rawdtw_batch_round_end_keep   enqueued on the context's stream behind a begun rawdtw_batch_round_end_begin of a batch from
 *        rawdtw_batch_submit_device whose records are the context's ended chaining round's (rawdtw_chain_round_recs): reads out, primary,
 *        recs, anchor_off and anchors where they lie.  RAWDTW_ERR_INVALID before anything is enqueued: no round end begun for this batch,
 *        no ended chaining round, no store, a dst outside the store, the same address twice.
 *   rawdtw_batch_round_keep_fetch after rawdtw_batch_round_end_fetch: kept_count[n_reads] (4 bytes a read).  When the round end ran again
 *        at its fetch (a batch the device-planned path declined), the keep launch runs again behind it first.  The context keeps a host
 *        mirror of every half's count, updated here; a half is RAWDTW_NOT_KEPT in the mirror from the keep's enqueue until this call.
 *   rawdtw_chain_kept_fetch       for tests: the half's count into *n (RAWDTW_NOT_KEPT included) and its first `cap` seeds (cap <= N)
 *        into `seeds`, whatever the count says.
 *   rawdtw_chain_round_begin_resident_kept  rawdtw_chain_round_begin_resident with a source per read: prev_src[r] == RAWDTW_PREV_HOST takes
 *        the read's prev_off stretch of prev_seeds as before; a store address takes the half's seeds -- the read's prev_off stretch must
 *        be empty and its seed_off stretch the mirror's count of that half plus its chunk's hits.  RAWDTW_ERR_INVALID before anything is
 *        enqueued: an address outside the store, a half whose mirror count is RAWDTW_NOT_KEPT (or that was never written), a read that
 *        sits out and has a source, a wrong stretch.  The keep launch of round N and this round's writer launch are on the context's
 *        stream, in that order.
 *   rawdtw_get_option(ctx, "round_keep_kernel_us")  read-only: the context's most recently fetched keep launch between its HIP events.
 *   rawdtw_set_option(ctx, "resident_chains", N)  on the context a mapper was created with, N = 1 .. 2^20 seeds a read: a resident round
 *        (rawdtw_mapper_round_seeded_resident, _signal_resident, _raw_resident) whose end is enqueued on the device ("device_round_end")
 *        keeps every read's primary chains in the store (reserved for the mapper's max_reads slots at the first such round; a failed
 *        reserve fails the round) and the next such round takes the read's previous seeds from there.  The host's copy of the chains
 *        stays as it is: fall-backs, rawdtw_mapper_finish and the lines read it, and lines, logs and counters are the same either way
 *        -- except rawdtw_mapper_resident_stats' seed_bytes_to_device, which counts what is actually sent up.  A read is seeded from the
 *        host again after anything else changed its chains: a round chained or ended on the host, a read the round end declined or
 *        whose anchors are more than N, rawdtw_mapper_round and rawdtw_mapper_round_seeded.  A read that sits a round out keeps its
 *        half; a failed round changes nothing.  Should a read's kept count ever differ from its chains on the host, the round fails with
 *        RAWDTW_ERR_DEVICE.  0 (the default): no such call is made.  The option is read once a round.  The store's slots are the
 *        mapper's read slots: one mapper a context uses it at a time.
 *   rawdtw_mapper_kept_stats  over committed rounds that used the store: reads with at least one previous seed that took them from the
 *        device / from the host, those seeds, and reads whose chains a keep launch did not keep.  Any pointer may be NULL.
 *   rawdtw_set_option(ctx, "chain_decline_reads", 1)  on the context a mapper was created with (its second group's context takes it over): a
 *        device-chained round -- plain, resident or from signal -- no longer goes to the host whole because the chaining cannot take one
 *        read.  The reads rawdtw_chain_round_declined names are chained by the host's own code on the mapper's threads (a resident round
 *        fetches their seeds alone, rawdtw_chain_round_declined_seeds, not the round's hits), appended (rawdtw_chain_round_append), and the
 *        DTW, the round end and the keep run on one batch.  Lines, logs and rounds are those of the mapper that chains on the host.  Such a
 *        round is no fall-back: rawdtw_mapper_resident_stats' fallback_rounds and hit_bytes_to_host do not move.  A declined read is not
 *        kept in the store of "resident_chains" (reads_not_kept counts it) and is seeded from the host in the round after; every other
 *        read keeps its half.  The option is read once a round and group.
 *   rawdtw_mapper_decline_stats  over committed rounds in which the chaining declined at least one read alone: those rounds; the reads declined
 *        for their seeds (reason bit 1) and for their chains (bits 2, 4); the other reads that took part in those rounds, counted for each read
 *        group that declined one of its own (the device chained them where a fall-back would have chained them on the host); and the bytes of declined reads' seeds brought home in resident
 *        rounds.  Any pointer may be NULL. ---- */
#define RAWDTW_NOT_KEPT 0xffffffffu
#define RAWDTW_NO_KEEP 0xffffffffu
#define RAWDTW_PREV_HOST 0xffffffffu
int rawdtw_chain_keep_reserve(rawdtw_ctx *ctx, uint64_t n_slots, uint64_t seeds_per_half);
int rawdtw_mapper_decline_stats(const rawdtw_mapper *m, uint64_t *rounds_with_declines, uint64_t *reads_declined_seeds,
                                uint64_t *reads_declined_chains, uint64_t *reads_chained_device, uint64_t *seed_bytes_to_host);
int rawdtw_mapper_kept_stats(const rawdtw_mapper *m, uint64_t *reads_from_device, uint64_t *reads_from_host, uint64_t *seeds_from_device,
                             uint64_t *seeds_from_host, uint64_t *reads_not_kept);
int rawdtw_round_keep_host(uint64_t n_reads, const uint64_t *chain_off, const rawdtw_chain_rec_t *recs, const uint64_t *anchor_off,
                           const rawdtw_anchor_t *anchors, const rawdtw_round_out_t *out, const uint32_t *primary, uint32_t cap,
                           uint32_t *kept_count, uint64_t *seed_off_out, rawdtw_seed_t *seeds_out);
int rawdtw_round_keep(rawdtw_ctx *ctx, uint64_t n_reads, const uint64_t *chain_off, const rawdtw_chain_rec_t *recs,
                      const uint64_t *anchor_off, const rawdtw_anchor_t *anchors, const rawdtw_round_out_t *out, const uint32_t *primary,
                      const uint32_t *dst, uint32_t *kept_count);
int rawdtw_batch_round_end_keep(rawdtw_ctx *ctx, rawdtw_batch *batch, const uint32_t *dst);
int rawdtw_batch_round_keep_fetch(rawdtw_ctx *ctx, rawdtw_batch *batch, uint32_t *kept_count);
int rawdtw_chain_kept_fetch(rawdtw_ctx *ctx, uint32_t addr, rawdtw_seed_t *seeds, uint32_t cap, uint32_t *n);
int rawdtw_chain_round_begin_resident_kept(rawdtw_ctx *ctx, const rawdtw_chain_opt_t *opt, uint64_t n_reads, const uint64_t *seed_off,
                                           const uint64_t *prev_off, const rawdtw_seed_t *prev_seeds, const uint32_t *prev_src,
                                           const uint32_t *chunk_start, const uint8_t *sits_out, const uint32_t *read_base,
                                           uint32_t n_keys, const uint64_t *key_base, uint64_t *chain_off, uint64_t *anchor_off,
                                           rawdtw_chain_rec_t *recs, uint64_t chains_cap, rawdtw_anchor_t *anchors);

/* ---- the reference from bases: ri_seq_to_sig (src/rsig.cpp:7-41) as rawindex.cpp:132-149 calls it, bit for bit.
 * The forward array of a sequence is strand 1 (the bases from the last to the first, each as 3 ^ code), the reverse array strand 0.
 * Codes are seq_nt4_table's (rutils.c:5-16): ACGTacgt, any other byte shifts 00 into the k-mer on either strand.  A strand has
 * s_len = len - k + 1 values (0 for len < k): the model's level of each k-mer, normalised by the mean and the standard deviation of
 * the strand's levels, whose sums are sequential double additions in emission order.  `contracted` 0: one rounding an operation;
 * 1: std_dev = sqrt(fma(-mean, mean, sum2 / j)), what an -O3 build of the reference for an FMA host computes (the only operation of the
 * function a compiler can fuse with an effect).  A strand of equal levels is NaN throughout (0 / 0); a NaN's sign and payload are not
 * part of the contract.
 *   rawdtw_pore_model_load   PoreModel::Load (pore_model.cpp:50-84) as main.cpp:349-351 uses it: lines that start with '#' or "kmer" are
 *        skipped (blank ones too), *k is the first k-mer's length, a row's slot is GenerateSeedFromSequence's (N -> A, lower case
 *        accepted), level_mean its second column; slots never named are 0.  RAWDTW_ERR_INVALID for an unreadable file, one without a
 *        k-mer, a k-mer of another length or k > 12; RAWDTW_ERR_RANGE with *k set when cap < 4^k floats (level_mean NULL, cap 0: ask k).
 *   rawdtw_seq_to_sig_host   one strand on the host: out has room for len - k + 1 floats.  The device's comparator; needs no GPU.
 *   rawdtw_seq_sums_restated the two sums alone, as both paths advance them: 64 values a step, each step one exact integer reduction
 *        where that equals the 64 roundings (every addend in [0, 2^(p+1)) for the sum's binade p, no rounding tie, no binade left),
 *        else 64 additions in order.  fast / slow count the steps of sum [0] and of sum2 [1]; either may be NULL.  For tests.
 *   rawdtw_reference_from_bases   what rawdtw_upload_reference does, from bases: the same arena layout, sequence table and
 *        rawdtw_reference_offset answers, the arena counted and shared as any other.  pore_vals has 4^k floats.  The bases cross as they
 *        are, a byte each; the codes are taken on the device.  A sequence shorter than k has length 0 on both strands.
 *        RAWDTW_ERR_INVALID for k outside 1 .. 12, a len of 2^31 or more and null arguments.  A failed call leaves the context's
 *        previous reference in place.
 *   rawdtw_reference_fetch   one strand of the context's reference (however it got there) comes home; RAWDTW_ERR_RANGE when cap is
 *        below its length, RAWDTW_ERR_INVALID for a sequence the context's table does not have.
 *   rawdtw_reference_build_stats   of the context's most recent rawdtw_reference_from_bases: the steps over all strands that went fast
 *        and slow, for sum [0] and sum2 [1], and the device time of the sums' and of the write's launch.  Any pointer may be NULL.
 *   rawdtw_seed_index_build_device   rawdtw_seed_index_build from the arrays the context's reference holds (rawdtw_upload_reference,
 *        rawdtw_index_upload or rawdtw_reference_from_bases), built on the device: the same keys in the same order, the same
 *        rawdtw_seed_index_get answers and rawdtw_seed_index_info numbers.  w > 0: RAWDTW_ERR_UNSUPPORTED and nothing changed (build on
 *        the host); no reference with a sequence table on the context, or bad pars: RAWDTW_ERR_INVALID.
 *   rawdtw_seed_index_build_stats   milliseconds of the context's most recent device build: filter, emit, sort (device time), the
 *        entries' way home and the table's build (host time).  After a w > 0 build the emit slot is the sum of the three selection launches.
 *   rawdtw_seed_index_build_device_min   rawdtw_seed_index_build_device's contract for w in 0 .. 255.  w = 0 runs that function's path
 *        unchanged.  w > 0: ri_sketch_min's windows (rsketch.c:146-221) over whole strands, as a count, a scan and a write of every
 *        e-mer's step on its own (rawdtw_seed_min.h) -- the table equals rawdtw_seed_index_build's from the same arrays: keys, key order,
 *        rawdtw_seed_index_get answers, rawdtw_seed_index_info numbers.  The entry arrays are sized by the scan's total (more entries than
 *        e-mers is legal).  RAWDTW_ERR_INVALID for bad pars (w >= 256, e < 2) or no reference with a sequence table, RAWDTW_ERR_OOM,
 *        RAWDTW_ERR_INTERNAL when the write launch's element count is not the scan's total; a failed call changes nothing.
 *        rawdtw_seed_index_build_device itself still refuses w > 0.
 *   rawdtw_seed_sketch_windowed   the host restatement of that parallel form for one strand or chunk: the kept events, every e-mer's hash,
 *        then the shared step for every e-mer independently.  Equal to rawdtw_seed_sketch, element for element (w = 0: ri_sketch_reg).
 *        *n is the true count; with cap too small RAWDTW_ERR_RANGE, *n still set and the first cap elements written.  Needs no GPU.  For tests.
 *   rawdtw_seed_index_build_min_stats   of the context's most recent w > 0 build: the e-mers over all strands, the entries emitted, and
 *        the device time in ms of the hash, count + scan and write launches.  Any pointer may be NULL. ---- */
int rawdtw_pore_model_load(const char *path, uint32_t *k, float *level_mean, uint64_t cap);
int rawdtw_seq_to_sig_host(const char *bases, uint32_t len, const float *pore_vals, uint32_t k, int strand, int contracted, float *out,
                           uint32_t *s_len);
int rawdtw_seq_sums_restated(const float *values, uint64_t n, double *sum, double *sum2, uint64_t fast[2], uint64_t slow[2]);
int rawdtw_reference_from_bases(rawdtw_ctx *ctx, uint32_t n_seq, const char *const *bases, const uint64_t *len, const float *pore_vals,
                                uint32_t k, int contracted);
int rawdtw_reference_fetch(rawdtw_ctx *ctx, uint32_t seq, int strand, float *out, uint64_t cap);
int rawdtw_reference_build_stats(const rawdtw_ctx *ctx, uint64_t fast_steps[2], uint64_t slow_steps[2], float kernel_ms[2]);
int rawdtw_seed_index_build_device(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out);
int rawdtw_seed_index_build_stats(const rawdtw_ctx *ctx, float phase_ms[5]);
int rawdtw_seed_index_build_device_min(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out);
int rawdtw_seed_sketch_windowed(const rawdtw_seed_pars_t *pars, const float *events, uint32_t len, uint32_t *hash, uint32_t *pos, uint32_t cap,
                                uint32_t *n);
int rawdtw_seed_index_build_min_stats(const rawdtw_ctx *ctx, uint64_t *emers, uint64_t *entries, float select_ms[3]);

/* ---- The seed index built and kept on the device (rawdtw_seed_build.hip, rawdtw_seed_tile.h): from the context's reference to a table
 * the seeding kernels read, without the entries, the slots or the lists crossing the link.
 *   rawdtw_seed_index_build_resident   rawdtw_seed_index_build_device_min's checks and refusals, w in 0 .. 255.  The kept events come
 *        from three launches with no chain over events (a tile of `tile` events a workgroup: every element's next kept element and its
 *        chain's last; a wave a strand, one step a tile: the tile's entry against the carried value; a tile again: the chain written
 *        out), then the unchanged emit or selection launches and the two sorts; the table's slots and lists are built from the sorted
 *        entries on the device, byte for byte what fill_table makes (keys inserted by rank with an atomic minimum a slot), and installed
 *        as the context's seed table under a fresh serial behind the last check.  A failed call leaves the context's table, and an ended
 *        resident seeding, as they were.  RAWDTW_ERR_INVALID while a seeding is begun on the context, as rawdtw_seed_index_upload.
 *        *out carries the header alone (rawdtw_seed_index_info answers as for a host-built index) and no host copy.
 *   rawdtw_seed_index_is_resident   1 while the index has no host copy, else 0 (NULL: 0).
 *        Such an index: rawdtw_seed_index_upload on the context that built it is the same-serial no-op, so every seeding and mapper
 *        entry that uploads works unchanged there.  What needs the host copy -- rawdtw_seed_index_get, _keys, rawdtw_seed_hits_host, the
 *        mapper's host seeding, rawdtw_seed_index_upload to another context -- returns RAWDTW_ERR_UNSUPPORTED: call
 *        rawdtw_seed_index_fetch first.  Once the context's table has been replaced, _upload there and _fetch return RAWDTW_ERR_INVALID.
 *        rawdtw_seed_index_destroy frees the handle only: the context owns the table.
 *   rawdtw_seed_index_fetch   the slots and lists come home into the handle: from then on an ordinary index with the same serial.  An
 *        index that has its host copy: RAWDTW_OK and nothing done.
 *   rawdtw_seed_index_from_entries   the table of n entries (hash[i], y[i]) sorted by (hash, y), through fill_table on the host;
 *        RAWDTW_ERR_INVALID for entries out of order.  Needs no GPU.
 *   rawdtw_seed_table_from_entries   the same entries through the device's table launches alone: a resident index on ctx.
 *        Both let chosen hashes meet in the slots.  For tests.
 *   rawdtw_seed_index_build_resident_stats   of the context's most recent resident build or rawdtw_seed_table_from_entries: the tile
 *        size, the tiles, kept events, entries and keys, the keys that do not lie in their home slot (counted on the finished table),
 *        and device milliseconds of the per-tile pass, the chain, the mark, emit or selection, the sorts and the table launches. ---- */
typedef struct {
    uint32_t tile, log2_slots;
    uint64_t tiles, kept, entries, keys, displaced;
    float next_ms, chain_ms, mark_ms, emit_ms, sort_ms, table_ms;
} rawdtw_seed_resident_stats_t;
int rawdtw_seed_index_build_resident(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out);
int rawdtw_seed_index_is_resident(const rawdtw_seed_index *six);
int rawdtw_seed_index_fetch(rawdtw_ctx *ctx, rawdtw_seed_index *six);
int rawdtw_seed_index_from_entries(const rawdtw_seed_pars_t *pars, uint32_t n_seq, uint64_t n, const uint32_t *hash, const uint64_t *y,
                                   rawdtw_seed_index **out);
int rawdtw_seed_table_from_entries(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, uint32_t n_seq, uint64_t n, const uint32_t *hash,
                                   const uint64_t *y, rawdtw_seed_index **out);
int rawdtw_seed_index_build_resident_stats(const rawdtw_ctx *ctx, rawdtw_seed_resident_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif /* RAWDTW_H */
