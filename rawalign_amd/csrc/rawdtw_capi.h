// rawdtw_capi.h -- what the translation units behind the C ABI (include/rawdtw.h) share: the records behind the opaque
// handles, small helpers, and the planner's entry points.  Internal: nothing here is part of the ABI.
//   rawdtw_capi.cpp       contexts, options (their table: rawdtw_options.h), arenas, pinned memory, incremental event upload
//   rawdtw_planner.cpp    the host planner of the job-list path, its launch sequences, rawdtw_plan_*, rawdtw_score_batch
//   rawdtw_batch.cpp      candidate batches: the stream path's set-up (sync-free, planned on the device), the job-list form,
//                         run / fetch / diagnostics, chunk rounds (a batch's launches by name and count: rawdtw_launches.h)
//   rawdtw_plan_check.cpp the readers of a device-planned batch's plan behind those diagnostics (no HIP: rawdtw_plan_check.h)
//   rawdtw_traceback.cpp  rawdtw_traceback_batch*, the single-call drop-ins
//   rawdtw_tb_driver.cpp  the one sub-batch driver of the three tracebacks (full matrix, banded, semiglobal)
//   rawdtw_semiglobal.cpp subsequence DTW: rawdtw_semiglobal_*, its drop-ins (kernels: rawdtw_semiglobal_kernels.hip)
//   rawdtw_index.cpp      the .ind reader
// There is NO CPU fallback in any of them: every scoring entry point runs the HIP kernels or returns an error status.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "rawdtw_internal.h"
#include "rawdtw_keep_layout.h"
#include "rawdtw_options.h"

using namespace rawdtw;

// Array of trivially-copyable records whose resize leaves the elements uninitialised: the planner's
// large outputs are written once, in parallel, and a value-initialising resize would first sweep them
// on one thread (page faults included).
template <typename T> struct RawVec {
    T *p = nullptr;
    size_t n = 0;
    RawVec() = default;
    RawVec(const RawVec &) = delete;
    RawVec &operator=(const RawVec &) = delete;
    ~RawVec() { free(p); }
    void resize(size_t count)
    {
        free(p);
        p = count ? static_cast<T *>(malloc(count * sizeof(T))) : nullptr;
        if (count && !p) { n = 0; throw std::bad_alloc(); }
        n = count;
    }
    size_t size() const { return n; }
    T *data() { return p; }
    const T *data() const { return p; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
    const T *begin() const { return p; }
    const T *end() const { return p + n; }
};

// one pooled workspace of the stream path: a device block and a pinned host block (rawdtw_batch_create carves them up)
struct StreamWs {
    char *d = nullptr; size_t d_bytes = 0;
    char *h = nullptr; size_t h_bytes = 0;
};

// a reference arena the library allocated, alive while any context uses it
struct RefHold {
    float *d = nullptr;
    std::atomic<int> refs{1};
};

// what a traceback call leaves for its timing getter: device time of its fill and walk launches, direction bytes written, path
// elements handed to the caller (rawdtw_tb_driver.cpp)
struct TbTiming {
    float fill_ms = 0.f, walk_ms = 0.f;
    uint64_t dir_written = 0, path_elems = 0;
};

struct rawdtw_ctx : rawdtw::Options { // (every option is a field of Options: rawdtw_options.h)
    int device = 0;
    hipStream_t stream = nullptr;
    // side streams: independent launches of one batch run concurrently (fork/join around the main stream)
    static constexpr int kSide = 3;
    hipStream_t side[kSide] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[kSide] = {nullptr, nullptr, nullptr};
    hipStream_t wide = nullptr;                 // sync-free batches: the side list's launch runs here, beside the tiles' launch
    hipEvent_t ev_wide_fork = nullptr, ev_wide_join = nullptr;
    int n_side = 0; // side streams used to fork the launches of one batch (RAWDTW_SIDE_STREAMS, 0..kSide). 0: the
                    // launches of a batch run in sequence on its one stream and overlap comes from several batches in
                    // flight on several contexts (swept: best throughput and cleaner per-kernel timings)
    std::vector<StreamWs> ws_free;     // workspaces of destroyed batches, reused by the next ones (no hipMalloc in the steady state)
    uint32_t stream_lds = 0, stream_blocks = 0; // persistent grid of k_stream at the current tile size
    int stream_threads_cached = 0;
    int stream_bpc_cached = -1;
    std::vector<uint64_t> job_off_scratch;
    void *d_append = nullptr;          // rawdtw_events_append staging, grow-only
    size_t append_bytes = 0;
    void *d_fetch = nullptr;           // rawdtw_events_fetch: the segment tables and, for an `out` the device cannot write, the staging; grow-only
    size_t fetch_bytes = 0;
    uint8_t *d_tb_dir = nullptr; // traceback direction workspace, grow-only (hipFree of 600 MB per call costs 1 ms)
    uint64_t tb_dir_bytes = 0;
    void *d_tb_paths = nullptr;  // traceback path buffers, two slots (rawdtw_tb_layout.h), grow-only
    size_t tb_paths_bytes = 0;
    void *h_pinned = nullptr;  // pinned landing zone of the traceback's paths, two slots, grow-only
    size_t pinned_bytes = 0;
    hipStream_t tb_copy = nullptr;                      // traceback: the paths' way home, beside the next sub-batch's kernels
    TbTiming tb, band_tb, semi; // the most recent full-matrix, banded and semiglobal traceback call (semi: any semiglobal call)
    // the aln text (rawdtw_aln_text.hip): a traceback's text form keeps its records, totals, offsets and the text itself here, two slots, grow-only;
    // the text goes home on a stream of its own (tb_copy already holds the next sub-batch's copies when a sub-batch's total is known)
    void *d_tb_text = nullptr;
    size_t tb_text_bytes = 0;
    hipStream_t tb_text = nullptr;
    float aln_count_ms = 0.f, aln_write_ms = 0.f;      // device time of the most recent text call's launches (rawdtw_aln_text_timing)
    uint64_t aln_text_bytes = 0;
    uint64_t tb_sub_batches = 0;  // "tb_sub_batches" (read-only): sub-batches of the most recent traceback call, known before its first plan is built
    // reference arena.  An arena the library allocated (rawdtw_upload_reference, rawdtw_index_upload) is held through a
    // counted RefHold, shared by every context that adopted it with rawdtw_share_reference: it is freed when the last of
    // them lets go, so the owner may upload another reference or be destroyed while sharers still run on the old one.
    float *d_ref = nullptr;
    uint64_t n_ref = 0;
    struct RefHold *ref_hold = nullptr; // null: no arena, or the caller's own device memory (rawdtw_set_reference_device)
    // plans and batches created on this context and not destroyed yet: rawdtw_destroy detaches them (frees their device
    // memory, clears their back pointer), after which rawdtw_plan_destroy / rawdtw_batch_destroy only delete the host record
    std::vector<rawdtw_plan *> live_plans;
    std::vector<rawdtw_batch *> live_batches;
    std::vector<uint64_t> ref_off; // 2*n_seq entries: [seq*2 + 0] = forward (strand 1), [seq*2 + 1] = reverse
    std::vector<uint32_t> ref_len;
    // the most recent rawdtw_reference_from_bases (rawdtw_refsig.hip): steps of sum [0] and sum2 [1], the sums' and the write's launch
    bool refsig_built = false;
    uint64_t refsig_fast[2] = {0, 0}, refsig_slow[2] = {0, 0};
    float refsig_ms[2] = {0.f, 0.f};
    // the most recent rawdtw_seed_index_build_device (rawdtw_seed_build.hip): filter, emit, sort, entries home, fill_table
    float seed_build_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    // the most recent w > 0 build of rawdtw_seed_index_build_device_min: e-mers over all strands, entries emitted, and the device time
    // of the hash, count + scan and write launches (their sum is seed_build_ms's emit slot)
    uint64_t seed_min_emers = 0, seed_min_entries = 0;
    float seed_min_ms[3] = {0.f, 0.f, 0.f};
    // the most recent rawdtw_seed_index_build_resident / rawdtw_seed_table_from_entries (rawdtw_seed_index_build_resident_stats)
    rawdtw_seed_resident_stats_t seed_resident{};
    // event arena
    float *d_ev = nullptr;
    uint64_t n_ev = 0, cap_ev = 0;
    bool own_ev = false;
    struct rawdtw_chain_ws *chain_ws = nullptr; // rawdtw_chain_round's device block (rawdtw_chain.hip), grow-only
    struct rawdtw_detect_ws *detect_ws = nullptr; // rawdtw_detect_begin's device block (rawdtw_events.hip), grow-only
    struct rawdtw_seed_ws *seed_ws = nullptr;     // rawdtw_seed_index_upload's table and rawdtw_seed_begin's device block (rawdtw_seed.hip), grow-only
    struct rawdtw_round_end_ws *round_end_ws = nullptr; // rawdtw_round_end's device block (rawdtw_round_end.hip), grow-only
    struct rawdtw_keep_ws *keep_ws = nullptr;           // the store of kept chains and its launch's block (rawdtw_keep.hip), grow-only
    uint32_t chain_max_seeds = 0; // tests: RAWDTW_CHAIN_MAX_SEEDS lowers rawdtw_chain_round's cap on seeds a read, so that small rounds take the declined path (0: no)
    bool border_local = false;      // rawdtw_set_border_local: border_constraint 2 is accepted by the batch entry points and rawdtw_mapper_create
    // rawdtw_set_semiglobal_window: columns a window of the semiglobal traceback (0: off, the n x m directions), the most recent traceback
    // call's windows (rawdtw_semiglobal_window_stats) and the two words the window kernel counts into (allocated at the first windowed call)
    uint32_t semi_window = 0;
    uint64_t semi_win_jobs = 0, semi_win_windows = 0, semi_win_max = 0, semi_win_ckpt_bytes = 0;
    unsigned long long *d_semi_win_stats = nullptr;
    bool local_jobs_device = true;  // a local batch from device arrays builds its job records on the device (k_local_jobs); tests: RAWDTW_LOCAL_JOBS=host
    std::string err;
};

struct rawdtw_plan {
    rawdtw_ctx *ctx = nullptr;
    uint64_t n_jobs = 0;
    RawVec<uint32_t> order;        // plan position -> job index
    std::vector<Launch> launches;
    std::vector<uint32_t> run_order; // launch indices, heaviest first
    std::vector<int32_t> launch_rpl;
    DevJob *d_jobs = nullptr;      // records of the jobs NOT handled by the tile kernel (plan order, after the tile jobs)
    uint64_t n_tile_jobs = 0;      // plan positions [0, n_tile_jobs) are tile-kernel jobs, in job order
    TileDesc *d_tiles = nullptr;
    TileSpan *d_spans = nullptr;
    TileJob *d_tjobs = nullptr;
    unsigned long long *d_masks = nullptr; // band bitmasks of the micro-path shapes
    uint64_t n_tiles = 0, n_tiles_hi = 0;   // d_tiles = [bulk tiles][wide-band tiles]
    uint32_t tile_lds_floats = 0, tile_hi_lds_floats = 0;
    FullAux *d_aux = nullptr;      // indexed like d_jobs (only meaningful for full-matrix jobs)
    float *d_cost = nullptr;
    uint32_t *d_end_j = nullptr;   // semiglobal launches (a local batch's plan): the last row's first minimum, job order
    uint64_t need_ev = 0, need_ref = 0; // ... and how far its windows reach into the arenas: checked again at every run (the arenas are the context's current ones)
    float *d_bnd = nullptr;
    uint8_t *d_dir = nullptr;
    uint64_t bnd_floats = 0, dir_bytes = 0;
    RawVec<DevJob> h_jobs;         // plan order (kept for traceback + info)
    std::vector<FullAux> h_aux;    // of the non-tile jobs: index = plan position - n_tile_jobs
    rawdtw_plan_info_t info{};
    bool cells_counted = false;
    int plan_threads_used = 1;
    bool dir_borrowed = false; // d_dir is the context's workspace, not the plan's
};

struct rawdtw_index {
    std::string path;
    uint32_t pars[8] = {0};
    std::vector<std::string> names;
    std::vector<uint32_t> lens;
    std::vector<uint64_t> fwd_pos; // file offset of each sequence's forward array (reverse follows it)
    uint64_t bucket_pos = 0;       // file offset of the first hash bucket (rawdtw_seed_index_load reads from there)
};

// What a caller hands to rawdtw_batch_create / rawdtw_batch_submit*: its arrays stay valid until fetch (a declined batch is redone from
// them through the job list), and the two properties of this one batch that are no setting of the context.
struct BatchIn {
    const uint64_t *chain_off = nullptr, *anchor_off = nullptr;
    const rawdtw_anchor_t *anchors = nullptr;
    const uint64_t *ref_base = nullptr;
    const uint32_t *read_base = nullptr;
    // compact hand-over (rawdtw_batch_submit_compact): the lists in packed form instead of `anchors`
    bool compact = false;
    const rawdtw_anchor_t *heads = nullptr, *unit_abs = nullptr;
    const uint16_t *steps = nullptr;
    const rawdtw_wide_step_t *wide = nullptr;
    uint64_t n_wide = 0;
    // chunk rounds (rawdtw_batch_submit_carry): the batch of the round before, the per-chain carry records and the round's SHORT
    // lists (new entries + junction); anchor_off / anchors stay the FULL lists' (anchors: the fallback's, may be null)
    const rawdtw_batch *prev = nullptr;
    const rawdtw_carry_t *carry = nullptr;
    const uint64_t *new_off = nullptr;
    const rawdtw_anchor_t *new_anchors = nullptr;
    bool resident = false; // anchors / ref_base / read_base (a round: new_anchors) are DEVICE pointers, used in place ("resident_arrays", rawdtw_batch_submit_device)
    bool submit = false;   // create and first run are one call: the side list's launch may go out between the planning launches
};

struct rawdtw_batch {
    rawdtw_ctx *ctx = nullptr;
    rawdtw_plan *plan = nullptr;   // job-list path
    rawdtw_align_opt_t opt{};
    uint64_t n_reads = 0, n_chains = 0;
    // filled the first time somebody asks, also through a const handle (the diagnostics): the job count of a sync-free batch (batch_count_jobs),
    // its counters (stream_counters; `dirty` goes with the wait) and its statistics (stream_stats_home)
    mutable uint64_t n_jobs = 0;
    mutable bool jobs_counted = false, cnt_valid = false, stats_home = false, cells_counted = false;
    mutable bool dirty = false;          // work enqueued since the last host synchronisation
    ChainDesc *d_chains = nullptr;
    uint64_t *d_chain_off = nullptr;
    uint32_t *d_fold_order = nullptr; // chain ids, longest chain first
    bool fold_fused = false;          // sync-free batch: fold and select are one launch (k_fold_select), no fold order was built
    float *d_full = nullptr, *d_gate = nullptr, *d_score = nullptr;
    uint8_t *d_keep = nullptr;
    bool own_chain_arrays = false;  // the arrays above are hipMalloc'd (job-list path) rather than carved from `ws`
    std::vector<hipEvent_t> ev; // event pairs of the runs enqueued since the last collect
    uint32_t ev_runs = 0;
    // stream path
    bool stream = false;
    StreamWs ws;
    StreamArgs sa{};
    uint32_t stream_lds = 0;
    int stream_threads = 256;
    unsigned long long *h_cnt = nullptr; // pinned landing zone of the counter block ...
    float *h_score = nullptr;            // ... and, behind it at the device block's offsets, of the scores and the keep flags: counters, scores
    uint8_t *h_keep = nullptr;           // and flags lie one behind the other in the workspace and come home in ONE copy (rawdtw_batch_fetch:
    size_t res_bytes = 0;                // every operation on a batch's stream is a step of its latency through the pipeline: three copies -> one, + 2 %)
    uint32_t stream_runs = 0;                // DTW launches issued for this batch (the tile queue needs a reset from the second on)
    size_t ws_bytes = 0;
    hipEvent_t ev_plan[4] = {nullptr, nullptr, nullptr, nullptr}; // ("time_plan") around scan + side list order, the side list's launch, the pass planning
    bool wide_out = false;            // the side list's launch for the next run went out with the planning launches
    BatchIn in;                          // what the caller handed over (in.prev: read at create only)
    bool in_carried = false;             // a chunk round: the device works on the short lists
    uint64_t parts_carried = 0;          // (summed from the carry records at create)
    // host copies of in.anchors / in.ref_base / in.read_base, made only if the job list is needed: of resident arrays, or the compact lists unpacked
    std::vector<rawdtw_anchor_t> host_anchors;
    std::vector<uint64_t> host_ref_base;
    std::vector<uint32_t> host_read_base;
    // a batch from device arrays that is no device-planned one (rawdtw_batch_hand_over_stats): job records k_local_jobs wrote, and what the
    // hand-over moved over the link -- offsets up and records home, or all anchors and bases home
    uint64_t local_records = 0, link_up = 0, link_home = 0;
};

namespace rawdtw {
namespace capi {


// the next `count` elements of a 256-byte aligned block
template <typename T> T *carve(char *&p, uint64_t count)
{
    T *q = reinterpret_cast<T *>(p);
    p += (count * sizeof(T) + 255) & ~(size_t)255;
    return q;
}
// (the same on an address, for a layout that is first laid from 0 to learn its size)
template <typename T> T *carve(uintptr_t &p, uint64_t count)
{
    T *q = reinterpret_cast<T *>(p);
    p += (count * sizeof(T) + 255) & ~(size_t)255;
    return q;
}

inline int fail(rawdtw_ctx *ctx, int status, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    return status;
}

inline int hip_fail(rawdtw_ctx *ctx, hipError_t e, const char *what)
{
    int st = (e == hipErrorOutOfMemory) ? RAWDTW_ERR_OOM : RAWDTW_ERR_DEVICE;
    return fail(ctx, st, std::string(what) + ": " + hipGetErrorString(e));
}

// The grow-only blocks of a begin / end workspace (rawdtw_seed.hip, rawdtw_events.hip): a device block, a page-locked host block in
// 8-byte words, the event pair around the launches and the event behind what comes home.
struct WsBlocks {
    void *dev = nullptr;
    size_t dev_bytes = 0;
    uint64_t *pin = nullptr;
    size_t pin_bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr;
};
// both blocks grown to at least need / pin_need bytes (a quarter more when they grow; contents are not kept), the events created on first use
int blocks_reserve(rawdtw_ctx *ctx, WsBlocks &w, size_t need, size_t pin_need, const char *dev_oom);
void blocks_release(WsBlocks &w);
// the device address of a page-locked host array of `bytes` bytes, or null: null itself, pageable memory, or an allocation that does
// not extend that far (the array is then copied by the caller's _end)
void *device_view(void *p, size_t bytes);

void chain_ws_free(rawdtw_ctx *ctx); // rawdtw_chain.hip
void detect_ws_free(rawdtw_ctx *ctx); // rawdtw_events.hip
void seed_ws_free(rawdtw_ctx *ctx);   // rawdtw_seed.hip
// The context's seed table for rawdtw_seed_build.hip's resident builds (rawdtw_seed.hip owns it).  installable: RAWDTW_OK, or what
// rawdtw_seed_index_upload would refuse (a seeding begun and not ended).  install: a finished table in device memory takes the place of
// the context's (the stream is idle; the blocks are the context's from here on).  view: the table's blocks while the context's table is
// the index `serial`; false: it has been replaced.
int seed_table_installable(rawdtw_ctx *ctx);
void seed_table_install(rawdtw_ctx *ctx, void *d_slots, uint64_t *d_list, uint32_t log2_slots, const rawdtw_seed_pars_t &pars, uint64_t serial);
bool seed_table_view(const rawdtw_ctx *ctx, uint64_t serial, const void **d_slots, const uint64_t **d_list);
void round_end_ws_free(rawdtw_ctx *ctx); // rawdtw_round_end.hip
void round_end_forget(rawdtw_ctx *ctx, const rawdtw_batch *b); // (rawdtw_batch.cpp's batch_detach)
int64_t round_end_kernel_us(const rawdtw_ctx *ctx); // the most recent fetched round end's launch, from its event pair ("round_end_kernel_us", read-only)
// The context's round end as rawdtw_keep.hip reads it: begun and not fetched (`pending`) or the most recently fetched one; out and primary
// where its launch left them in the round end's workspace, valid until the context's next round end.  `serial` counts the launches: a
// round end that ran again at its fetch has another.
struct RoundEndView {
    bool pending = false;
    const rawdtw_batch *batch = nullptr;
    uint64_t n_reads = 0, n_chains = 0, serial = 0;
    const rawdtw_round_out_t *d_out = nullptr;
    const uint32_t *d_primary = nullptr;
    const rawdtw_chain_rec_t *d_recs = nullptr;
};
bool round_end_view(const rawdtw_ctx *ctx, RoundEndView *v); // rawdtw_round_end.hip; false: the context has had no round end
// the context's ended chaining round's records, anchor offsets and anchors in its workspace (rawdtw_chain.hip); false: there is none
struct ChainKeptView { const rawdtw_chain_rec_t *d_recs = nullptr; const uint64_t *d_aoff = nullptr; const rawdtw_anchor_t *d_anch = nullptr; };
bool chain_kept_view(const rawdtw_ctx *ctx, ChainKeptView *v);
// the store of kept chains (rawdtw_keep.hip): its block, its layout and the host mirror of the halves' counts; false: there is none
struct KeepStoreView { const char *store = nullptr; keep::Layout L; const uint32_t *mirror = nullptr; };
bool keep_store_view(const rawdtw_ctx *ctx, KeepStoreView *v);
void keep_ws_free(rawdtw_ctx *ctx);
void keep_forget(rawdtw_ctx *ctx, const rawdtw_batch *b); // (rawdtw_batch.cpp's batch_detach)
int64_t round_keep_kernel_us(const rawdtw_ctx *ctx); // the most recent fetched keep launch, from its event pair ("round_keep_kernel_us", read-only)
// A resident detection begun on the context and not ended (rawdtw_events.hip), as rawdtw_seed_detected_begin reads it: everything the
// seeding needs is in the detection's workspace on the device.  `enqueued` false: no launch went out (no chunk, or no sample).
struct DetectView {
    bool enqueued = false;
    uint32_t n = 0;                  // chunks
    uint64_t cap = 0;                // the detection's events_cap: the total of events is at most this, or the flag is set
    uint64_t n_samples = 0;          // the samples that went up (a chunk never has more events than samples)
    const uint64_t *d_eoff = nullptr; // n + 1 dense event offsets
    const uint64_t *d_dst = nullptr;  // per chunk: where its events start in the context's event arena
    const uint64_t *d_flag = nullptr; // [0] != 0: the detection declined (a chunk over its room, or the total over the cap) and wrote nothing
};
bool detect_resident_view(const rawdtw_ctx *ctx, DetectView *v);
// the context's ended resident seeding (rawdtw_seed.hip) as rawdtw_chain_round_begin_resident uses it: its hit offsets on the host
// (null: there is none), and the launch that lays reads' previous anchors and hits down as the chaining's seed list, on the context's stream
const uint64_t *seed_resident_hit_off(const rawdtw_ctx *ctx, uint64_t *n_chunks);
// (d_prev_src null: every read's previous anchors come from d_prev; else per read RAWDTW_PREV_HOST or a half of the store of kept chains)
void seed_resident_write_chain(rawdtw_ctx *ctx, rawdtw_seed_t *d_seeds, const uint64_t *d_seed_off, const uint64_t *d_prev_off, const rawdtw_seed_t *d_prev,
                               const uint32_t *d_chunk_start, const uint8_t *d_sits_out, const uint32_t *d_prev_src);

#define HIP_TRY(ctx, expr)                                                                            \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return hip_fail((ctx), e_, #expr);                                      \
    } while (0)

// exact size of the band's cell set (same walk as the kernels; host side, for reporting)
inline uint64_t banded_cells(uint32_t n, uint32_t m, int R)
{
    const uint32_t N = n > m ? n : m, M = n > m ? m : n;
    const int P = R + ((R % 2 == 0) ? 1 : 0), S = R + ((R % 2 == 1) ? 1 : 0);
    uint64_t cells = 1;
    int row = 0;
    uint32_t rem = 0;
    for (uint32_t col = 1; col < N; col++) {
        rem += M;
        const bool adv = rem >= N;
        if (adv) { rem -= N; row++; }
        for (int pass = adv ? 0 : 1; pass < 2; pass++) {
            const int len = pass == 0 ? S : P;
            const int si = pass == 0 ? (int)col + S / 2 - 1 : (int)col + P / 2;
            const int sj = pass == 0 ? row - S / 2 : row - P / 2;
            int lo = 0, hi = len;
            lo = std::max(lo, si - (int)N + 1);
            lo = std::max(lo, -sj);
            hi = std::min(hi, si + 1);
            hi = std::min(hi, (int)M - sj);
            if (hi > lo) cells += (uint64_t)(hi - lo);
        }
    }
    return cells;
}

// bitmask of the band's cell set for a shape whose longer side is <= 8: bit 8*j + i  <=>  cell
// (i over the longer sequence, j over the shorter) is evaluated (same walk as banded_cells)
inline uint64_t band_mask8(uint32_t N, uint32_t M, int R)
{
    const int P = R + ((R % 2 == 0) ? 1 : 0), S = R + ((R % 2 == 1) ? 1 : 0);
    uint64_t mask = 1; // (0,0)
    int row = 0;
    uint32_t rem = 0;
    for (uint32_t col = 1; col < N; col++) {
        rem += M;
        const bool adv = rem >= N;
        if (adv) { rem -= N; row++; }
        for (int pass = adv ? 0 : 1; pass < 2; pass++) {
            const int len = pass == 0 ? S : P;
            const int si = pass == 0 ? (int)col + S / 2 - 1 : (int)col + P / 2;
            const int sj = pass == 0 ? row - S / 2 : row - P / 2;
            int lo = 0, hi = len;
            lo = std::max(lo, si - (int)N + 1);
            lo = std::max(lo, -sj);
            hi = std::min(hi, si + 1);
            hi = std::min(hi, (int)M - sj);
            for (int o = lo; o < hi; o++) mask |= 1ull << (8 * (sj + o) + (si - o));
        }
    }
    return mask;
}

inline int full_rpl(uint32_t ny)
{
    return ny <= 64 ? 1 : ny <= 128 ? 2 : ny <= 256 ? 4 : 8;
}

inline uint64_t dir_bytes_for(uint32_t n, uint32_t m, int rpl)
{
    const uint32_t NX = n > m ? n : m, NY = n > m ? m : n;
    const uint64_t strips = (NY + 64ull * rpl - 1) / (64ull * rpl);
    const uint64_t spb = rpl == 8 ? 8 : 16; // steps per 16-byte block (k_full_wave)
    return strips * (((uint64_t)NX + 63 + spb - 1) / spb) * 64 * 16;
}

// let go of the context's reference arena (the allocation dies with its last user)
inline void drop_reference(rawdtw_ctx *ctx)
{
    if (RefHold *h = ctx->ref_hold) {
        if (h->refs.fetch_sub(1) == 1) { if (h->d) (void)hipFree(h->d); delete h; }
    }
    ctx->ref_hold = nullptr; ctx->d_ref = nullptr; ctx->n_ref = 0;
}

template <typename T> void unregister(std::vector<T *> &v, T *x)
{
    for (size_t i = 0; i < v.size(); i++)
        if (v[i] == x) { v[i] = v.back(); v.pop_back(); return; }
}

template <typename T> int dev_alloc(rawdtw_ctx *ctx, T **p, uint64_t count)
{
    *p = nullptr;
    if (count == 0) return RAWDTW_OK;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(p), count * sizeof(T)));
    return RAWDTW_OK;
}

// ---- what the call-scoped units (rawdtw_semiglobal.cpp, rawdtw_band_tb.cpp) share ----
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// a device block that goes when the call ends (behind the context's stream); `what` names the unit in the failure's message
struct DevBlock {
    rawdtw_ctx *ctx; const char *what; char *p = nullptr;
    DevBlock(rawdtw_ctx *c, const char *w) : ctx(c), what(w) {}
    DevBlock(const DevBlock &) = delete;
    DevBlock &operator=(const DevBlock &) = delete;
    ~DevBlock() { if (p) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(p); } }
    int reserve(size_t bytes)
    {
        if (hipMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(bytes, 256)) != hipSuccess) {
            p = nullptr; (void)hipGetLastError();
            return fail(ctx, RAWDTW_ERR_OOM, std::string(what) + " workspace allocation failed");
        }
        return RAWDTW_OK;
    }
};
// the events around a call's fill and walk launches
struct EventPair {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    EventPair() = default;
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
// b goes to a private reference arena for the duration of a single call (the hold on the context's own arena stays)
struct PrivateRef {
    rawdtw_ctx *ctx; float *saved; uint64_t saved_n; float *d_b = nullptr;
    explicit PrivateRef(rawdtw_ctx *c) : ctx(c), saved(c->d_ref), saved_n(c->n_ref) {}
    PrivateRef(const PrivateRef &) = delete;
    PrivateRef &operator=(const PrivateRef &) = delete;
    int put(const float *b, uint32_t m)
    {
        int st = dev_alloc(ctx, &d_b, ((uint64_t)m + 3) & ~3ull);
        if (st != RAWDTW_OK) return st;
        hipError_t e = hipMemcpyAsync(d_b, b, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "operand upload");
        ctx->d_ref = d_b; ctx->n_ref = m;
        return RAWDTW_OK;
    }
    ~PrivateRef()
    {
        ctx->d_ref = saved; ctx->n_ref = saved_n;
        if (d_b) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(d_b); }
    }
};
// the context's direction workspace, grow-only (one traceback at a time per context)
inline int ensure_tb_dir(rawdtw_ctx *ctx, uint64_t need)
{
    if (ctx->tb_dir_bytes >= need) return RAWDTW_OK;
    if (ctx->d_tb_dir) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ctx->d_tb_dir); }
    ctx->d_tb_dir = nullptr; ctx->tb_dir_bytes = 0;
    const uint64_t want = need + need / 8;
    if (int st = dev_alloc(ctx, &ctx->d_tb_dir, want)) return st;
    ctx->tb_dir_bytes = want;
    return RAWDTW_OK;
}
// "tb_workspace_mb" (the option goes before the variable RAWDTW_TB_WORKSPACE_MB) in bytes
inline uint64_t tb_budget_bytes(const rawdtw_ctx *ctx)
{
    if (ctx->tb_workspace_mb) return ctx->tb_workspace_mb << 20;
    if (const char *e = getenv("RAWDTW_TB_WORKSPACE_MB")) return std::max<uint64_t>(1, strtoull(e, nullptr, 10)) << 20;
    return 16ull << 30;
}

inline int ensure_events_capacity(rawdtw_ctx *ctx, uint64_t n)
{
    if (ctx->own_ev && ctx->cap_ev >= n) return RAWDTW_OK;
    if (ctx->own_ev && ctx->d_ev) (void)hipFree(ctx->d_ev);
    ctx->d_ev = nullptr;
    ctx->own_ev = true;
    uint64_t cap = std::max<uint64_t>(n + (n >> 2), 1024);
    cap = (cap + 63) & ~63ull;
    int st = dev_alloc(ctx, &ctx->d_ev, cap);
    if (st != RAWDTW_OK) { ctx->cap_ev = 0; return st; }
    ctx->cap_ev = cap;
    return RAWDTW_OK;
}

// ---- the planner's entry points (rawdtw_planner.cpp) ----
struct PlanCfg;
// run fn(t) for t in [0, T) on T threads (the caller's thread takes t = 0)
template <typename F> void parallel_for(int T, F fn)
{
    if (T <= 1) { fn(0); return; }
    std::vector<std::thread> th;
    th.reserve(T - 1);
    for (int t = 1; t < T; t++) th.emplace_back([&fn, t] { fn(t); });
    fn(0);
    for (auto &x : th) x.join();
}
int build_plan(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, bool traceback, rawdtw_plan **out);
uint64_t count_cells(const rawdtw_plan *pl, uint64_t p0, uint64_t p1);
MergeSel merge_of(const rawdtw_ctx *ctx, const rawdtw_plan *pl); // (merge_select, rawdtw_launches.h, under the context's settings)
int run_all_launches(rawdtw_ctx *ctx, rawdtw_plan *pl, hipEvent_t *ev);
void plan_release_device(rawdtw_plan *plan);
// ---- rawdtw_semiglobal.cpp ----
// A plan whose launches are semiglobal fills (kKindSemiWave), one class a launch: what a local batch owns in the planner's place.  Records,
// aux and boundary rows on the device, costs in job order; run_all_launches runs it against the context's current arenas.
int build_semi_plan(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, rawdtw_plan **out);
// ---- rawdtw_local.hip ----
// k_local_jobs: chain c's job record of a local batch from anchors[anchor_off[c + 1] - 1], anchors[anchor_off[c]], ref_base[c], read_base[c]
// (all device arrays), written in chain order; an empty chain gets n = m = 0
hipError_t launch_local_jobs(const uint64_t *anchor_off, const rawdtw_anchor_t *anchors, const uint64_t *ref_base, const uint32_t *read_base,
                             uint64_t n_chains, rawdtw_job_t *jobs_out, hipStream_t s);
// the tile records as downloaded from the device against the job list (rawdtw_batch_verify_plan): "" or what is wrong
std::string verify_uploaded_tiles(const rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const rawdtw_plan *pl, const TileDesc *tiles,
                                  size_t n_tiles, const TileSpan *spans, size_t n_spans, const TileJob *tjobs, size_t n_tjobs, std::vector<uint8_t> &seen);
// ---- rawdtw_batch.cpp ----
// a batch whose (deferred) planning failed has neither form left: every entry point but destroy refuses it
inline bool batch_dead(const rawdtw_batch *b) { return !b->stream && !b->plan; }
void batch_detach(rawdtw_ctx *ctx, rawdtw_batch *b);
// the batch's results as they will stand: a device-planned batch's counters home (a wait for its stream), and a batch that path declined
// scored again through the job list (*redone: its device arrays are others now)
int batch_settle(rawdtw_ctx *ctx, rawdtw_batch *b, bool *redone);

} // namespace capi
} // namespace rawdtw
