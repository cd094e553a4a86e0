// rawdtw_batch.cpp -- candidate batches behind rawdtw_batch_* (include/rawdtw.h): the DTW block of gen_chains
// (src/rmap.cpp:509-530) for every read of a mini-batch in one submission.  The stream path's set-up (sparse + banded
// batches: everything enqueued, planned on the device -- kernels in rawdtw_runs.hip), the job-list form for the other
// modes and for what the stream path declines, run / fetch / diagnostics, and chunk rounds (rawdtw_batch_submit_carry).
// Host code only.
#include "rawdtw_capi.h"
#include "rawdtw_plan_check.h"
#include "rawdtw_stream_layout.h"

using namespace rawdtw;
using namespace rawdtw::capi;

static_assert(stream::kCounterBytes == kStreamCounters * 8 && stream::kChainDescBytes == sizeof(ChainDesc), "the two sizes rawdtw_stream_layout.h names");

// a region of a workspace block as a pointer
template <typename T> static T *at(char *block, const ws::Region &r) { return reinterpret_cast<T *>(block + r.at); }

extern "C" {

// ---- whole-batch form ----------------------------------------------------------------------------
// Two implementations behind rawdtw_batch_*:
//   stream  (sparse + banded batches, the default): rawdtw_stream.hip -- rawdtw_batch_create only enqueues copies and
//           planning kernels on the context's stream, no host synchronisation, no allocation in the steady state
//           (workspaces are pooled per context); every count stays on the device.
//   job list (everything else, and the rare batch the stream path declines): the jobs are built on the host and go
//           through plan_host / build_plan like any rawdtw_plan.
namespace {

// LDS image of a device-planned batch's tiles, in floats.  With four workgroups a CU (stream_blocks_per_cu) a SIMD keeps
// 128 registers free beside the DTW launch's waves -- room for a wave of the next batches' planning kernels or of the
// batch before's fold -- and the LDS that a fifth workgroup would take goes into larger tiles (fewer tiles, fuller sorted
// waves).  Measured on the bench pipeline (4 batches in flight): 5 x 4800 floats 425 GCUPS, 4 x 7200 453, 3 x 6400 450;
// later, with k_pre's chain table in LDS (2 KB a workgroup): 4 x 7200 508, 4 x 7000 524, 4 x 6800 523, 4 x 6000 511 -- the planning
// kernels of the batches behind need LDS beside the four resident workgroups.
static uint32_t stream_tile_floats(const rawdtw_ctx *ctx) { return (ctx->tile_lds_set ? ctx->tile_lds_floats : kStreamTileFloats) & ~3u; } // (16-byte multiples: the records and the sort table sit behind the image)

bool stream_eligible(const rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_anchors)
{
    // (the job-list path takes batches below "device_plan_min_jobs" anchors: a chain of n anchors has n - 1 jobs)
    if (!ctx->device_plan || n_anchors < ctx->device_plan_min_jobs || n_anchors == 0 || n_anchors >= (1ull << 31)) return false;
    if (opt->border_constraint != 1 || opt->fill_method == 0) return false; // sparse + banded only
    if (ctx->lane_max_radius < 0 || ctx->sort_n || ctx->sort_r1_n || ctx->sort_r3 || ctx->lane_hi || !ctx->merge_small) return false;
    if (ctx->tile_threads != 256 || ctx->debug_skip_kinds) return false;
    const uint32_t worst_part = 2u * ctx->lane_max_n + 16u; // image floats of the largest tile-class part alone
    return stream_tile_floats(ctx) >= 2u * worst_part && stream_tile_floats(ctx) <= 16384u;
}

int ws_acquire(rawdtw_ctx *ctx, size_t dev_bytes, size_t host_bytes, StreamWs *out)
{
    int best = -1;
    for (size_t i = 0; i < ctx->ws_free.size(); i++) {
        const StreamWs &w = ctx->ws_free[i];
        if (w.d_bytes >= dev_bytes && w.h_bytes >= host_bytes && (best < 0 || w.d_bytes < ctx->ws_free[best].d_bytes)) best = (int)i;
    }
    if (best >= 0) {
        *out = ctx->ws_free[best];
        ctx->ws_free.erase(ctx->ws_free.begin() + best);
        return RAWDTW_OK;
    }
    // nothing fits: drop the smallest pooled workspace when the pool is full, then allocate with head room
    if (ctx->ws_free.size() >= 8) {
        size_t smallest = 0;
        for (size_t i = 1; i < ctx->ws_free.size(); i++) if (ctx->ws_free[i].d_bytes < ctx->ws_free[smallest].d_bytes) smallest = i;
        (void)hipFree(ctx->ws_free[smallest].d); (void)hipHostFree(ctx->ws_free[smallest].h);
        ctx->ws_free.erase(ctx->ws_free.begin() + smallest);
    }
    StreamWs w;
    w.d_bytes = dev_bytes + dev_bytes / 4; w.h_bytes = host_bytes + host_bytes / 4;
    if (hipMalloc(reinterpret_cast<void **>(&w.d), w.d_bytes) != hipSuccess) return fail(ctx, RAWDTW_ERR_OOM, "batch workspace allocation failed");
    if (hipHostMalloc(reinterpret_cast<void **>(&w.h), w.h_bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipFree(w.d);
        return fail(ctx, RAWDTW_ERR_OOM, "pinned batch staging allocation failed");
    }
    *out = w;
    return RAWDTW_OK;
}

void ws_release(rawdtw_ctx *ctx, StreamWs &w)
{
    if (w.d) ctx->ws_free.push_back(w);
    w = StreamWs{};
}

bool stream_declined(const rawdtw_batch *b);

// the side list's launch on the context's second stream: behind everything enqueued on the main stream so far; the main
// stream joins it (ev_wide_join) before the fold
static hipError_t stream_wide_fork(rawdtw_ctx *ctx, const StreamArgs &a)
{
    if (!ctx->wide_beside) return stream_wide(a, ctx->wide_blocks, ctx->stream); // (in line: nothing to join)
    hipError_t he = hipEventRecord(ctx->ev_wide_fork, ctx->stream);
    if (he == hipSuccess) he = hipStreamWaitEvent(ctx->wide, ctx->ev_wide_fork, 0);
    if (he == hipSuccess) he = stream_wide(a, ctx->wide_blocks, ctx->wide);
    if (he == hipSuccess) he = hipEventRecord(ctx->ev_wide_join, ctx->wide);
    return he;
}

// the stream path: everything rawdtw_batch_create does for a sparse + banded batch -- O(1) host work: a workspace from the
// pool, five copies and three launches enqueued
int batch_create_stream(rawdtw_ctx *ctx, rawdtw_batch *b)
{
    const BatchIn &in = b->in;
    // (a chunk round: the device's lists are the SHORT ones -- new entries + junction -- and `na` their length; the full lists only
    // give the fold its offsets)
    const rawdtw_batch *prev = in.prev;
    const bool round = prev != nullptr; // (rawdtw_batch_submit_carry checked that it can serve: rawdtw_batch_can_carry)
    const bool compact = in.compact;
    const uint64_t nc = b->n_chains, nr = b->n_reads, n_full = in.anchor_off[nc], na = round ? in.new_off[nc] : n_full;
    const uint32_t lds_floats = stream_tile_floats(ctx);
    // where everything lies: rawdtw_stream_layout.h
    const stream::Layout L = stream::layout({nr, nc, na, n_full, compact ? stream::Kind::compact : round ? stream::Kind::round : stream::Kind::plain,
                                             in.n_wide, ctx->pass_pool});
    int st = ws_acquire(ctx, L.need, L.pin_need, &b->ws);
    if (st != RAWDTW_OK) return st;
    char *const d = b->ws.d, *const h = b->ws.h;
    StreamArgs &a = b->sa;
    a = StreamArgs{};
    a.n_anchors = na; a.n_chains = nc; a.n_reads = nr; a.n_ev = ctx->n_ev; a.n_ref = ctx->n_ref;
    a.frac = b->opt.band_radius_frac;
    // tiles take radius <= stream_tile_radius; the radii between that and lane_max_radius (none by default) go to the side
    // list's lane classes
    a.lane_max_radius = std::min(ctx->lane_max_radius, ctx->stream_tile_radius); a.side_lane_radius = ctx->lane_max_radius;
    a.lane_max_n = ctx->lane_max_n;
    // (a batch that runs out of slots is redone through the job list)
    a.tile_anchors = kStreamTile; a.n_tiles = L.n_tiles; a.n_slots = L.n_slots; a.others_cap = L.others_cap;
    a.lds_floats = lds_floats;
    a.debug = ctx->stream_debug;
    a.ev = ctx->d_ev; a.ref = ctx->d_ref;
    a.cnt = at<unsigned long long>(d, L.cnt);
    b->d_score = at<float>(d, L.score); b->d_keep = at<uint8_t>(d, L.keep); b->res_bytes = L.res_bytes; // (right behind the counters: one copy brings all three home)
    b->d_chain_off = at<uint64_t>(d, L.chain_off);
    a.tlist = at<uint2>(d, L.tlist); a.todo = at<uint4>(d, L.todo); a.recs = at<uint2>(d, L.recs); a.runtab = at<uint4>(d, L.runtab);
    a.tile_stats = at<unsigned long long>(d, L.tile_stats);
    a.omix = at<DevJob>(d, L.omix); a.ojobs = at<DevJob>(d, L.ojobs); a.ocls = at<uint8_t>(d, L.ocls);
    b->d_chains = at<ChainDesc>(d, L.chains); b->d_fold_order = at<uint32_t>(d, L.fold_order);
    b->d_full = at<float>(d, L.full); b->d_gate = at<float>(d, L.gate);
    a.out = at<float>(d, L.out);
    a.anchor_off = at<uint64_t>(d, L.anchor_off);
    // ("resident_arrays": the three big arrays are device pointers, used in place; their regions stay unused)
    const rawdtw_anchor_t *const lists = round ? in.new_anchors : in.anchors; // (a round: only its NEW anchors, and the junctions, cross the bus)
    a.anchors = in.resident ? lists : at<rawdtw_anchor_t>(d, L.anchors);
    a.ref_base = in.resident ? in.ref_base : at<uint64_t>(d, L.ref_base);
    a.read_base = in.resident ? in.read_base : at<uint32_t>(d, L.read_base);
    if (compact) { // the packed lists; k_scan decodes them into the anchors' region
        a.heads = at<rawdtw_anchor_t>(d, L.heads); a.unit_abs = at<rawdtw_anchor_t>(d, L.unit_abs);
        a.steps = at<uint16_t>(d, L.steps); a.wide = at<rawdtw_wide_step_t>(d, L.wide); a.n_wide = in.n_wide;
        a.anchors_w = at<rawdtw_anchor_t>(d, L.anchors);
    }
    a.full_off = a.anchor_off; a.n_full = n_full; a.out_full = a.out; // (no predecessor: the lists are the full ones)
    if (round) { // (the previous batch's cost array is read by this batch's k_gather: stream order keeps it alive that long)
        a.carry = at<rawdtw_carry_t>(d, L.carry); a.full_off = at<uint64_t>(d, L.full_off); a.out_full = at<float>(d, L.out_full);
        a.prev_out_full = prev->sa.out_full; a.prev_n_full = prev->sa.n_full;
        a.prev_cnt = prev->sa.cnt; a.prev_others_cap = prev->sa.others_cap;
    }
    b->h_cnt = at<unsigned long long>(h, L.p_cnt); b->h_score = at<float>(h, L.p_score); b->h_keep = at<uint8_t>(h, L.p_keep); // (same offsets as on the device)
    unsigned long long *h_init = b->h_cnt; // the counters' initial values travel from the pinned block
    for (int i = 0; i < kStreamCounters; i++) h_init[i] = 0;
    h_init[kCntBad] = h_init[kCntOverflow] = ~0ull;
    hipStream_t s = ctx->stream;
    if (ctx->time_plan) for (hipEvent_t &pe : b->ev_plan) if (!pe) HIP_TRY(ctx, hipEventCreate(&pe));
    HIP_TRY(ctx, hipMemcpyAsync(d + L.cnt.at, h_init, stream::kCounterBytes, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d + L.anchor_off.at, round ? in.new_off : in.anchor_off, (nc + 1) * 8, hipMemcpyHostToDevice, s));
    if (compact) {
        HIP_TRY(ctx, hipMemcpyAsync(d + L.heads.at, in.heads, nc * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d + L.unit_abs.at, in.unit_abs, L.n_units * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d + L.steps.at, in.steps, na * 2, hipMemcpyHostToDevice, s));
        if (in.n_wide) HIP_TRY(ctx, hipMemcpyAsync(d + L.wide.at, in.wide, in.n_wide * sizeof(rawdtw_wide_step_t), hipMemcpyHostToDevice, s));
    } else if (round) {
        HIP_TRY(ctx, hipMemcpyAsync(d + L.carry.at, in.carry, nc * sizeof(rawdtw_carry_t), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d + L.full_off.at, in.anchor_off, (nc + 1) * 8, hipMemcpyHostToDevice, s));
    }
    if (!in.resident) { // what the three kinds share (a compact batch's anchors are decoded on the device)
        if (!compact && na) HIP_TRY(ctx, hipMemcpyAsync(d + L.anchors.at, lists, na * sizeof(rawdtw_anchor_t), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d + L.ref_base.at, in.ref_base, nc * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d + L.read_base.at, in.read_base, nc * 4, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(ctx, hipMemcpyAsync(d + L.chain_off.at, in.chain_off, (nr + 1) * 8, hipMemcpyHostToDevice, s));
    b->fold_fused = ctx->fold_mode == 4; // (no fold order then: the one-workgroup sort stays off the scan's critical path)
    if (ctx->time_plan) HIP_TRY(ctx, hipEventRecord(b->ev_plan[0], s)); // ("time_plan": the planning LAUNCHES, behind the hand-over's copies)
    hipError_t e = stream_plan(a, b->d_chains, b->fold_fused ? nullptr : b->d_fold_order, s);
    // The side list's launch goes out here, between the scan and the pass planning, for the batch's first run (a batch that
    // runs again launches it again in front of the tiles' launch): measured, the fresh-batch pipeline runs 6 % faster with
    // the wide bands' long tail in front of the planning launch than behind it.
    if (e == hipSuccess && ctx->time_plan) e = hipEventRecord(b->ev_plan[1], s);
    b->wide_out = false;
    // (only inside rawdtw_batch_submit*: between a separate create and run the caller may upload new events, and a run reads
    // the arenas as they are then)
    if (e == hipSuccess && !(ctx->stream_debug & 4u) && ctx->wide_order == 0 && (in.submit || ctx->wide_at_create)) { e = stream_wide_fork(ctx, a); b->wide_out = e == hipSuccess; }
    if (e == hipSuccess && ctx->time_plan) e = hipEventRecord(b->ev_plan[2], s);
    if (e == hipSuccess) e = stream_plan_passes(a, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "batch planning launches");
    if (ctx->time_plan) HIP_TRY(ctx, hipEventRecord(b->ev_plan[3], s));
    // the persistent grid: what the device holds at this LDS size
    if (ctx->stream_lds != lds_floats || ctx->stream_threads_cached != ctx->stream_threads || ctx->stream_bpc_cached != ctx->stream_blocks_per_cu) {
        hipDeviceProp_t prop;
        HIP_TRY(ctx, hipGetDeviceProperties(&prop, ctx->device));
        const int per_cu = stream_blocks_per_cu(lds_floats, ctx->stream_threads);
        if (per_cu <= 0) return fail(ctx, RAWDTW_ERR_DEVICE, "occupancy query failed for the batch kernel");
        const int use = ctx->stream_blocks_per_cu > 0 ? std::min(per_cu, ctx->stream_blocks_per_cu) : per_cu;
        ctx->stream_blocks = (uint32_t)(use * prop.multiProcessorCount);
        ctx->stream_bpc_cached = ctx->stream_blocks_per_cu;
        ctx->stream_lds = lds_floats;
        ctx->stream_threads_cached = ctx->stream_threads;
    }
    b->stream = true;
    b->stream_lds = lds_floats;
    b->stream_threads = ctx->stream_threads;
    b->n_jobs = 0; b->jobs_counted = false;
    b->cnt_valid = false; b->stats_home = false;
    b->dirty = true;
    b->ws_bytes = L.need;
    return RAWDTW_OK;
}

// DTW jobs of a sync-free batch (align_chain issues n_anchors - 1 per chain, rmap.cpp:248): counted from the caller's
// chain offsets the first time somebody asks -- rawdtw_batch_create itself does not walk the chains
void batch_count_jobs(const rawdtw_batch *b)
{
    if (b->jobs_counted || !b->stream) return;
    uint64_t n = 0;
    for (uint64_t c = 0; c < b->n_chains; c++) {
        const uint64_t k = b->in.anchor_off[c + 1] - b->in.anchor_off[c];
        n += k ? k - 1 : 0;
    }
    b->n_jobs = n;
    b->jobs_counted = true;
}

// the two base arrays from the caller's device memory into the batch's host copies: the last of a resident hand-over to come home
static int bases_home(rawdtw_ctx *ctx, rawdtw_batch *b)
{
    const uint64_t nc = b->n_chains;
    try { b->host_ref_base.resize(nc + 1); b->host_read_base.resize(nc + 1); } // (+ 1: non-null arrays for a round without chains)
    catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    if (nc) HIP_TRY(ctx, hipMemcpy(b->host_ref_base.data(), b->in.ref_base, nc * 8, hipMemcpyDeviceToHost));
    if (nc) HIP_TRY(ctx, hipMemcpy(b->host_read_base.data(), b->in.read_base, nc * 4, hipMemcpyDeviceToHost));
    b->link_home += nc * 12;
    b->in.ref_base = b->host_ref_base.data(); b->in.read_base = b->host_read_base.data();
    b->in.resident = false;
    return RAWDTW_OK;
}

// what the job-list path reads on the host: the compact lists unpacked, device-resident arrays brought home
int materialise_host_arrays(rawdtw_ctx *ctx, rawdtw_batch *b)
{
    BatchIn &in = b->in;
    const uint64_t nc = b->n_chains, na = in.anchor_off[nc];
    if (in.compact) { // the job list is built from plain anchors
        try { b->host_anchors.resize(na); } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
        if (rawdtw_anchors_unpack(nc, in.anchor_off, in.heads, in.unit_abs, in.steps, in.wide, in.n_wide, b->host_anchors.data()) != RAWDTW_OK)
            return fail(ctx, RAWDTW_ERR_INVALID, "malformed compact anchor lists");
        in.anchors = b->host_anchors.data();
        in.compact = false;
        return RAWDTW_OK;
    }
    if (b->in_carried) { // a chunk round: the device only has the short lists; the full ones are the caller's, for exactly this
        if (!in.anchors) return fail(ctx, RAWDTW_ERR_UNSUPPORTED, "a carried round the device-planned path declined, and no full anchor lists to redo it from: submit the round whole");
        b->in_carried = false;
        return in.resident ? bases_home(ctx, b) : RAWDTW_OK; // (the bases are the caller's device arrays)
    }
    if (!in.resident) return RAWDTW_OK;
    try { b->host_anchors.resize(na + 1); } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    if (na) HIP_TRY(ctx, hipMemcpy(b->host_anchors.data(), in.anchors, na * sizeof(rawdtw_anchor_t), hipMemcpyDeviceToHost));
    b->link_home += na * sizeof(rawdtw_anchor_t);
    const int st = bases_home(ctx, b);
    if (st == RAWDTW_OK) in.anchors = b->host_anchors.data();
    return st;
}

int batch_finish_joblist(rawdtw_ctx *ctx, rawdtw_batch *b, const rawdtw_job_t *jobs, uint64_t n_jobs, const std::vector<ChainDesc> &desc);

// the job-list path: jobs built on the host (chain ranges spread over the planner's threads), plan_host, chain records
int batch_create_joblist(rawdtw_ctx *ctx, rawdtw_batch *b, const std::vector<uint64_t> &job_off, uint64_t n_jobs)
{
    const BatchIn &in = b->in; // (its arrays are on the host: materialise_host_arrays)
    const uint64_t n_chains = b->n_chains;
    const rawdtw_align_opt_t *opt = &b->opt;
    // chain descriptors: from the anchors alone.  The parts' read regions telescope (consecutive parts share their
    // anchor event), so sum(n) = (last.q - first.q) + parts in the reference's uint32 arithmetic (rmap.cpp:236,292).
    std::vector<ChainDesc> desc(n_chains);
    for (uint64_t c = 0; c < n_chains; c++) {
        const uint64_t a0 = in.anchor_off[c], a1 = in.anchor_off[c + 1];
        ChainDesc &d = desc[c];
        d.job_first = job_off[c];
        d.n_jobs = (uint32_t)(job_off[c + 1] - job_off[c]);
        d.descending = 0;
        if (a1 == a0) { d.span = 0; d.num_aligned = 0; continue; }
        const rawdtw_anchor_t &first = in.anchors[a1 - 1], &last = in.anchors[a0];
        d.span = last.query_position - first.query_position + 1; // rmap.cpp:202,245
        d.num_aligned = opt->border_constraint != 1 ? d.span : (last.query_position - first.query_position) + d.n_jobs; // (global and local: n)
    }
    RawVec<rawdtw_job_t> jobs;
    try { jobs.resize(n_jobs); } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    int T = ctx->plan_threads;
    if (T <= 0) {
        const unsigned hc = std::thread::hardware_concurrency();
        T = (int)std::min<uint64_t>(std::min<unsigned>(hc ? hc : 1, 16), n_jobs / 32768 + 1);
    }
    T = std::max(1, std::min(T, 64));
    std::vector<int> status(T, RAWDTW_OK);
    parallel_for(T, [&](int t) {
        // split by jobs, not chains: chain lengths are skewed
        const uint64_t j_lo = n_jobs * (uint64_t)t / T, j_hi = n_jobs * (uint64_t)(t + 1) / T;
        const uint64_t c_lo = std::lower_bound(job_off.begin(), job_off.begin() + n_chains, j_lo) - job_off.begin();
        const uint64_t c_hi = t + 1 == T ? n_chains
                                         : std::lower_bound(job_off.begin(), job_off.begin() + n_chains, j_hi) - job_off.begin();
        for (uint64_t c = c_lo; c < c_hi; c++) {
            const uint64_t a0 = in.anchor_off[c], a1 = in.anchor_off[c + 1];
            const uint32_t nj = (uint32_t)(job_off[c + 1] - job_off[c]);
            if (!nj) continue;
            int s2 = rawdtw_chain_build_jobs(opt, in.anchors + a0, (uint32_t)(a1 - a0), in.ref_base[c], in.read_base[c], 0,
                                             jobs.data() + job_off[c]);
            if (s2 != RAWDTW_OK) { status[t] = s2; return; }
        }
    });
    for (int t = 0; t < T; t++) if (status[t] != RAWDTW_OK) return fail(ctx, status[t], "job building failed");
    return batch_finish_joblist(ctx, b, jobs.data(), n_jobs, desc);
}

// the second half of the job-list form: the plan -- the planner's, or for a local batch the semiglobal launches (build_semi_plan) --, the
// chain records and the fold order on the device
int batch_finish_joblist(rawdtw_ctx *ctx, rawdtw_batch *b, const rawdtw_job_t *jobs, uint64_t n_jobs, const std::vector<ChainDesc> &desc)
{
    const uint64_t n_chains = b->n_chains, n_reads = b->n_reads;
    int st = b->opt.border_constraint == 2 ? build_semi_plan(ctx, jobs, n_jobs, &b->plan) : build_plan(ctx, jobs, n_jobs, false, &b->plan);
    if (st != RAWDTW_OK) return st;
    b->n_jobs = n_jobs;
    st = dev_alloc(ctx, &b->d_chains, n_chains);
    if (st == RAWDTW_OK) st = dev_alloc(ctx, &b->d_chain_off, n_reads + 1);
    if (st == RAWDTW_OK) st = dev_alloc(ctx, &b->d_fold_order, n_chains);
    if (st == RAWDTW_OK) st = dev_alloc(ctx, &b->d_full, n_chains);
    if (st == RAWDTW_OK) st = dev_alloc(ctx, &b->d_gate, n_chains);
    if (st == RAWDTW_OK) st = dev_alloc(ctx, &b->d_score, n_chains);
    if (st == RAWDTW_OK) st = dev_alloc(ctx, &b->d_keep, n_chains);
    if (st != RAWDTW_OK) return st;
    b->own_chain_arrays = true;
    hipError_t e = hipSuccess;
    // fold order: longest chain first (stable counting sort on the part count)
    std::vector<uint32_t> fold_order(n_chains);
    {
        constexpr uint32_t kB = 65536;
        std::vector<uint64_t> start(kB + 1, 0);
        auto bucket = [&](uint64_t c) { return kB - 1 - std::min<uint32_t>(desc[c].n_jobs, kB - 1); };
        for (uint64_t c = 0; c < n_chains; c++) start[bucket(c) + 1]++;
        for (uint32_t q = 0; q < kB; q++) start[q + 1] += start[q];
        for (uint64_t c = 0; c < n_chains; c++) fold_order[start[bucket(c)]++] = (uint32_t)c;
    }
    if (n_chains) e = hipMemcpyAsync(b->d_chains, desc.data(), n_chains * sizeof(ChainDesc), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && n_chains)
        e = hipMemcpyAsync(b->d_fold_order, fold_order.data(), n_chains * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_chain_off, b->in.chain_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream); // (the staging vectors above die with this scope)
    if (e != hipSuccess) return hip_fail(ctx, e, "uploading chain descriptors");
    return RAWDTW_OK;
}

// A local batch whose anchor arrays are on the device (rawdtw_batch_submit_device, "resident_arrays"): k_local_jobs (rawdtw_local.hip)
// writes a record a chain from the chain's two end anchors and its bases; the offsets go up (8 bytes a chain), the records come home
// (32 bytes a chain) and the host plans the launches' classes from them.  No anchor crosses the link.
int batch_create_local_device(rawdtw_ctx *ctx, rawdtw_batch *b)
{
    const BatchIn &in = b->in;
    const uint64_t n_chains = b->n_chains;
    std::vector<rawdtw_job_t> recs;
    std::vector<ChainDesc> desc;
    try { recs.resize(n_chains); desc.resize(n_chains); } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    if (n_chains) {
        DevBlock blk(ctx, "local batch"); // (freed behind the stream when this scope ends)
        const int st = blk.reserve(al256((n_chains + 1) * 8) + n_chains * sizeof(rawdtw_job_t));
        if (st != RAWDTW_OK) return st;
        char *p = blk.p;
        uint64_t *d_off = carve<uint64_t>(p, n_chains + 1);
        rawdtw_job_t *d_recs = carve<rawdtw_job_t>(p, n_chains);
        HIP_TRY(ctx, hipMemcpyAsync(d_off, in.anchor_off, (n_chains + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        const hipError_t e = launch_local_jobs(d_off, in.anchors, in.ref_base, in.read_base, n_chains, d_recs, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "local job records launch");
        HIP_TRY(ctx, hipMemcpyAsync(recs.data(), d_recs, n_chains * sizeof(rawdtw_job_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        b->local_records = n_chains; b->link_up += (n_chains + 1) * 8; b->link_home += n_chains * sizeof(rawdtw_job_t);
    }
    uint64_t n_jobs = 0; // an empty chain has no job: the records are compacted in place, chain order kept
    for (uint64_t c = 0; c < n_chains; c++) {
        const bool empty = in.anchor_off[c + 1] == in.anchor_off[c];
        desc[c] = ChainDesc{n_jobs, empty ? 0u : 1u, empty ? 0u : recs[c].n, empty ? 0u : recs[c].n, 0u}; // span = num_aligned = n
        if (!empty) recs[n_jobs++] = recs[c];
    }
    return batch_finish_joblist(ctx, b, recs.data(), n_jobs, desc);
}

// forget the device pointers: into the workspace, or at the job-list form's own arrays (handed back or freed by the caller)
void batch_forget_arrays(rawdtw_batch *b)
{
    b->d_chains = nullptr; b->d_chain_off = nullptr; b->d_fold_order = nullptr;
    b->d_full = b->d_gate = b->d_score = nullptr; b->d_keep = nullptr;
}

void batch_release_device(rawdtw_batch *b)
{
    if (b->plan) { rawdtw_plan_destroy(b->plan); b->plan = nullptr; }
    if (b->own_chain_arrays) {
        if (b->d_chains) (void)hipFree(b->d_chains);
        if (b->d_chain_off) (void)hipFree(b->d_chain_off);
        if (b->d_fold_order) (void)hipFree(b->d_fold_order);
        if (b->d_full) (void)hipFree(b->d_full);
        if (b->d_gate) (void)hipFree(b->d_gate);
        if (b->d_score) (void)hipFree(b->d_score);
        if (b->d_keep) (void)hipFree(b->d_keep);
    }
    batch_forget_arrays(b);
    b->own_chain_arrays = false;
}

// The counters of a stream batch, read once (after its planning kernels have run).
int stream_counters(rawdtw_ctx *ctx, const rawdtw_batch *b)
{
    if (b->cnt_valid) return RAWDTW_OK;
    HIP_TRY(ctx, hipMemcpyAsync(b->h_cnt, b->sa.cnt, stream::kCounterBytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    b->cnt_valid = true;
    b->dirty = false;
    return RAWDTW_OK;
}

// does the stream path's result stand?  (no invalid job, nothing over a capacity, no band it does not take)
bool stream_declined(const rawdtw_batch *b)
{
    const unsigned long long *c = b->h_cnt;
    return c[kCntBad] != ~0ull || c[kCntOverflow] != ~0ull || c[kCntUnsupported] != 0 || c[kCntOthers] > b->sa.others_cap;
}

// The statistics the device sums on request -- tile jobs, tile bytes, side-list bytes; with_cells: the cell count in front of them --
// in h_cnt: what is missing is summed and brought home, once a batch (the planning launches wrote what is summed; runs do not change it).
int stream_stats_home(rawdtw_ctx *ctx, const rawdtw_batch *b, bool with_cells)
{
    if (b->cells_counted || (b->stats_home && !with_cells)) return RAWDTW_OK;
    const int first = with_cells ? kCntCells : kCntTileJobs;
    static_assert(kCntTileJobs == kCntCells + 1 && kCntOtherBytes == kCntCells + 3, "the four reporting counters lie one behind the other");
    if (with_cells) HIP_TRY(ctx, stream_count_cells(b->sa, b->sa.cnt + kCntCells, ctx->stream));
    if (!b->stats_home) HIP_TRY(ctx, stream_sum_stats(b->sa, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&b->h_cnt[first], b->sa.cnt + first, (kCntOtherBytes + 1 - first) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    b->stats_home = true;
    b->cells_counted = with_cells;
    return RAWDTW_OK;
}

// what the job-list form starts from: the caller's arrays on the host and the chains' job offsets
int joblist_count(rawdtw_ctx *ctx, rawdtw_batch *b, std::vector<uint64_t> &job_off, uint64_t *n_jobs)
{
    const int st = materialise_host_arrays(ctx, b);
    if (st != RAWDTW_OK) return st;
    job_off.resize(b->n_chains + 1);
    if (rawdtw_batch_build_jobs(&b->opt, b->n_chains, b->in.anchor_off, b->in.anchors, b->in.ref_base, b->in.read_base, job_off.data(), nullptr, 0, n_jobs) != RAWDTW_OK)
        return fail(ctx, RAWDTW_ERR_INVALID, "job counting failed");
    return RAWDTW_OK;
}

// Redo a stream batch through the job-list path (which also words the error of an invalid batch).
int stream_fallback(rawdtw_ctx *ctx, rawdtw_batch *b)
{
    std::vector<uint64_t> job_off;
    uint64_t n_jobs = 0;
    int st = joblist_count(ctx, b, job_off, &n_jobs);
    if (st != RAWDTW_OK) return st;
    b->stream = false; b->jobs_counted = true; // (batch_create_joblist sets n_jobs)
    // (event pairs of timed runs enqueued so far were laid out for the declined form's launches: rawdtw_batch_collect walks them by
    // the launch count of the form the batch has, so they go with the form they timed)
    for (auto &e : b->ev) if (e) (void)hipEventDestroy(e);
    b->ev.clear(); b->ev_runs = 0;
    ws_release(ctx, b->ws);
    b->h_cnt = nullptr; b->h_score = nullptr; b->h_keep = nullptr; b->res_bytes = 0; // (they lay in the workspace)
    batch_forget_arrays(b);
    st = batch_create_joblist(ctx, b, job_off, n_jobs);
    if (st != RAWDTW_OK) { batch_release_device(b); return st; }
    return rawdtw_batch_run(ctx, b);
}

} // namespace

// the guard of the entry points that take a context and a batch: the batch is this context's and has a form left (batch_dead)
static bool batch_ok(const rawdtw_ctx *ctx, const rawdtw_batch *batch) { return ctx && batch && batch->ctx == ctx && !batch_dead(batch); }
static int batch_check(rawdtw_ctx *ctx, const rawdtw_batch *batch)
{
    return batch_ok(ctx, batch) ? RAWDTW_OK : fail(ctx, RAWDTW_ERR_INVALID, "batch does not belong to this context");
}

// The context's own handle of a batch that came in through a const pointer (rawdtw_batch_info redoes a declined batch: more than a cache).
static rawdtw_batch *batch_owned(const rawdtw_batch *batch)
{
    for (rawdtw_batch *b : batch->ctx->live_batches) if (b == batch) return b;
    return nullptr;
}

static int batch_create_any(rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_reads, const BatchIn &in, rawdtw_batch **out)
{
    if (!out) return RAWDTW_ERR_INVALID;
    *out = nullptr;
    if (!ctx || !opt || !in.chain_off || !in.anchor_off || (!in.anchors && !in.compact && !in.prev && n_reads) || !in.ref_base || !in.read_base)
        return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (in.compact && (!in.heads || !in.unit_abs || !in.steps || (!in.wide && in.n_wide)))
        return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    // (2, local: only on a context that opted in -- rawdtw_set_border_local; off, the refusal, its status and its wording stay)
    if (opt->border_constraint != 0 && opt->border_constraint != 1 && !(opt->border_constraint == 2 && ctx->border_local))
        return fail(ctx, RAWDTW_ERR_INVALID, "invalid border constraint (rmap.cpp:301-304)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t n_chains = in.chain_off[n_reads];
    int st = RAWDTW_OK;
    rawdtw_batch *b = new (std::nothrow) rawdtw_batch;
    if (!b) return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    b->ctx = ctx; b->opt = *opt; b->n_reads = n_reads; b->n_chains = n_chains;
    ctx->live_batches.push_back(b);
    b->in = in;
    if (in.prev) {
        b->in_carried = true;
        for (uint64_t c = 0; c < n_chains; c++) b->parts_carried += in.carry[c].parts;
    }
    if (stream_eligible(ctx, opt, in.anchor_off[n_chains]))
        st = batch_create_stream(ctx, b);
    else if (opt->border_constraint == 2 && b->in.resident && !b->in.compact && ctx->local_jobs_device)
        st = batch_create_local_device(ctx, b); // (two anchors a chain are all a local batch needs: they are read where they lie)
    else {
        uint64_t n_jobs = 0;
        st = joblist_count(ctx, b, ctx->job_off_scratch, &n_jobs); // (a context is not re-entrant)
        if (st == RAWDTW_OK) st = batch_create_joblist(ctx, b, ctx->job_off_scratch, n_jobs);
    }
    b->in.prev = nullptr; // (read at create only)
    if (st != RAWDTW_OK) { rawdtw_batch_destroy(b); return st; }
    *out = b;
    return RAWDTW_OK;
}

// the five arrays every hand-over has, under the context's "resident_arrays"
static BatchIn batch_in(const rawdtw_ctx *ctx, const uint64_t *chain_off, const uint64_t *anchor_off, const rawdtw_anchor_t *anchors,
                        const uint64_t *ref_base, const uint32_t *read_base)
{
    BatchIn in;
    in.chain_off = chain_off; in.anchor_off = anchor_off; in.anchors = anchors; in.ref_base = ref_base; in.read_base = read_base;
    in.resident = ctx && ctx->resident_arrays;
    return in;
}

int rawdtw_batch_create(rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off,
                        const uint64_t *anchor_off, const rawdtw_anchor_t *anchors, const uint64_t *ref_base,
                        const uint32_t *read_base, rawdtw_batch **out)
{
    return batch_create_any(ctx, opt, n_reads, batch_in(ctx, chain_off, anchor_off, anchors, ref_base, read_base), out);
}

static int batch_enqueue_one(rawdtw_ctx *ctx, rawdtw_batch *batch, hipEvent_t *e, uint32_t nl);

// rawdtw_batch_submit*: create and the first run in one call; no batch is left behind a failure
static int batch_submit_any(rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_reads, BatchIn in, rawdtw_batch **out)
{
    in.submit = true;
    int st = batch_create_any(ctx, opt, n_reads, in, out);
    if (st != RAWDTW_OK) return st;
    st = batch_enqueue_one(ctx, *out, nullptr, 0);
    if (st != RAWDTW_OK) { rawdtw_batch_destroy(*out); *out = nullptr; }
    return st;
}

int rawdtw_batch_submit(rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off,
                        const uint64_t *anchor_off, const rawdtw_anchor_t *anchors, const uint64_t *ref_base,
                        const uint32_t *read_base, rawdtw_batch **out)
{
    return batch_submit_any(ctx, opt, n_reads, batch_in(ctx, chain_off, anchor_off, anchors, ref_base, read_base), out);
}

int rawdtw_batch_submit_device(rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off,
                               const uint64_t *anchor_off, const rawdtw_anchor_t *d_anchors, const uint64_t *d_ref_base,
                               const uint32_t *d_read_base, rawdtw_batch **out)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    BatchIn in = batch_in(ctx, chain_off, anchor_off, d_anchors, d_ref_base, d_read_base);
    in.resident = true; // (the option's meaning, for this one batch: a batch keeps the form it was created under)
    return batch_submit_any(ctx, opt, n_reads, in, out);
}

int rawdtw_batch_submit_compact(rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off,
                                const uint64_t *anchor_off, const rawdtw_anchor_t *heads, const rawdtw_anchor_t *unit_abs,
                                const uint16_t *steps, const rawdtw_wide_step_t *wide, uint64_t n_wide, const uint64_t *ref_base,
                                const uint32_t *read_base, rawdtw_batch **out)
{
    BatchIn in = batch_in(ctx, chain_off, anchor_off, nullptr, ref_base, read_base);
    in.compact = true; in.heads = heads; in.unit_abs = unit_abs; in.steps = steps; in.wide = wide; in.n_wide = n_wide;
    in.resident = false; // (the packed lists are host arrays: k_scan decodes them on the device)
    return batch_submit_any(ctx, opt, n_reads, in, out);
}

// can `prev` serve as the previous batch of a chunk round with options `opt`?  (include/rawdtw.h)
int rawdtw_batch_can_carry(const rawdtw_ctx *ctx, const rawdtw_batch *prev, const rawdtw_align_opt_t *opt)
{
    if (!ctx || !prev || !opt || prev->ctx != ctx || !prev->stream || prev->stream_runs == 0) return 0;
    if (prev->cnt_valid && stream_declined(prev)) return 0;
    // (a part's radius, and with it its cost, follows from these; the fold's options may differ)
    if (prev->opt.border_constraint != opt->border_constraint || prev->opt.fill_method != opt->fill_method ||
        memcmp(&prev->opt.band_radius_frac, &opt->band_radius_frac, sizeof(float)) != 0)
        return 0;
    return 1; // (the kernel-selection options only decide which body scores a part: costs do not depend on them)
}

int rawdtw_batch_submit_carry(rawdtw_ctx *ctx, const rawdtw_align_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off,
                              const uint64_t *anchor_off, const rawdtw_anchor_t *anchors, const uint64_t *new_off, const rawdtw_anchor_t *new_anchors,
                              const uint64_t *ref_base, const uint32_t *read_base, const rawdtw_batch *prev, const rawdtw_carry_t *carry, rawdtw_batch **out)
{
    if (out) *out = nullptr;
    if (!ctx || !opt || !out || !chain_off || !anchor_off || !new_off || !carry || !prev) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    const uint64_t nc = chain_off[n_reads];
    if (!rawdtw_batch_can_carry(ctx, prev, opt) || !stream_eligible(ctx, opt, new_off[nc]))
        return fail(ctx, RAWDTW_ERR_UNSUPPORTED, "the previous batch cannot serve this round (another context or options, never run, or not on the device-planned path): submit the round whole");
    if (new_off[nc] > anchor_off[nc] || (!new_anchors && new_off[nc])) return fail(ctx, RAWDTW_ERR_INVALID, "more new anchors than anchors");
    BatchIn in = batch_in(ctx, chain_off, anchor_off, anchors, ref_base, read_base);
    in.prev = prev; in.carry = carry; in.new_off = new_off; in.new_anchors = new_anchors;
    return batch_submit_any(ctx, opt, n_reads, in, out);
}

int rawdtw_batch_round_stats(rawdtw_ctx *ctx, rawdtw_batch *batch, uint64_t *parts_scored, uint64_t *parts_reused)
{
    if (const int bad = batch_check(ctx, batch)) return bad;
    batch_count_jobs(batch);
    uint64_t reused = 0;
    if (batch->stream) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const int st = stream_counters(ctx, batch);
        if (st != RAWDTW_OK) return st;
        if (!stream_declined(batch)) reused = batch->parts_carried;
    }
    if (parts_reused) *parts_reused = reused;
    if (parts_scored) *parts_scored = batch->n_jobs - reused;
    return RAWDTW_OK;
}

// A device-planned batch's plan on the host, downloaded once (its counters are home: stream_counters): the work list's entries
// in use -- both stretches --, all job records, the copy-order slots in use, the side list.  A work list longer than the slots
// leaves the arrays empty (StreamPlanView::fits_slots: the readers say so).
struct StreamPlanHost {
    StreamPlanView v;
    std::vector<PassEntry> todo;
    std::vector<JobRec> recs;
    std::vector<CopyOrder> runtab;
    std::vector<DevJob> side;
};
static_assert(sizeof(PassEntry) == sizeof(uint4) && sizeof(JobRec) == sizeof(uint2) && sizeof(CopyOrder) == sizeof(uint4), "the host's records are the device's words");
static int stream_plan_download(rawdtw_ctx *ctx, const rawdtw_batch *batch, StreamPlanHost &h)
{
    const StreamArgs &a = batch->sa;
    const unsigned long long *cnt = batch->h_cnt;
    StreamPlanView &v = h.v;
    v.n_anchors = a.n_anchors; v.n_chains = batch->n_chains;
    v.n_tiles = a.n_tiles; v.n_slots = a.n_slots; v.lds_floats = a.lds_floats; v.lane_max_n = a.lane_max_n; v.lane_max_radius = a.lane_max_radius;
    v.n_first = cnt[kCntTodo]; v.n_pool = cnt[kCntPool]; v.n_other = cnt[kCntOthers]; v.n_reused = cnt[kCntReused];
    v.anchor_off = batch->in.anchor_off;
    if (!v.fits_slots()) return RAWDTW_OK;
    constexpr size_t kRT = stream::kSlotOrders;
    h.todo.resize(v.n_todo()); h.runtab.resize(v.n_todo() * kRT);
    h.recs.resize((size_t)a.n_tiles * kStreamRecStride); h.side.resize(v.n_other);
    if (v.n_first) {
        HIP_TRY(ctx, hipMemcpy(h.todo.data(), a.todo, v.n_first * sizeof(uint4), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(h.runtab.data(), a.runtab, v.n_first * kRT * sizeof(uint4), hipMemcpyDeviceToHost));
    }
    if (v.n_pool) {
        HIP_TRY(ctx, hipMemcpy(h.todo.data() + v.n_first, a.todo + a.n_tiles, v.n_pool * sizeof(uint4), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(h.runtab.data() + v.n_first * kRT, a.runtab + (size_t)a.n_tiles * kRT, v.n_pool * kRT * sizeof(uint4), hipMemcpyDeviceToHost));
    }
    if (!h.recs.empty()) HIP_TRY(ctx, hipMemcpy(h.recs.data(), a.recs, h.recs.size() * sizeof(uint2), hipMemcpyDeviceToHost));
    if (v.n_other) HIP_TRY(ctx, hipMemcpy(h.side.data(), a.ojobs, v.n_other * sizeof(DevJob), hipMemcpyDeviceToHost));
    v.todo = h.todo.data(); v.recs = h.recs.data(); v.runtab = h.runtab.data(); v.side = h.side.data();
    return RAWDTW_OK;
}

int rawdtw_batch_verify_plan(rawdtw_ctx *ctx, const rawdtw_batch *batch, const rawdtw_job_t *jobs, uint64_t n_jobs,
                             int *device_planned, char *message, uint32_t message_cap)
{
    auto say = [&](const std::string &m) { if (message && message_cap) snprintf(message, message_cap, "%s", m.c_str()); };
    say("");
    if (!batch_ok(ctx, batch) || (n_jobs && !jobs)) return RAWDTW_ERR_INVALID;
    if (device_planned) *device_planned = batch->stream ? 1 : 0;
    batch_count_jobs(batch);
    if (n_jobs != batch->n_jobs) { say("job count differs from the batch's"); return RAWDTW_ERR_INVALID; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    auto S = [](uint64_t v) { return std::to_string(v); };
    std::string e;
    if (batch->stream) {
        // what the scan and k_plan left behind for the DTW launch, against the job list the host builds from the same chains
        // (check_stream_plan); then the statistics, which the device sums
        int st = stream_counters(ctx, batch);
        if (st != RAWDTW_OK) return st;
        if (stream_declined(batch)) {
            if (device_planned) *device_planned = 0;
            say("the stream path declined this batch (it is redone through the job list at fetch)");
            return RAWDTW_OK;
        }
        StreamPlanHost h;
        st = stream_plan_download(ctx, batch, h);
        if (st != RAWDTW_OK) return st;
        StreamPlanStats want;
        e = check_stream_plan(h.v, jobs, n_jobs, &want);
        if (e.empty()) {
            st = stream_stats_home(ctx, batch, false);
            if (st != RAWDTW_OK) return st;
            const unsigned long long *c = batch->h_cnt;
            if (c[kCntTileJobs] != want.tile_jobs || c[kCntTileBytes] != want.tile_bytes || c[kCntOtherBytes] != want.other_bytes) e = "tile statistics";
        }
        say(e);
        return e.empty() ? RAWDTW_OK : RAWDTW_ERR_DEVICE + 100;
    }
    const rawdtw_plan *pl = batch->plan;
    // the tile records as the kernels will read them
    const size_t n_tiles = pl->n_tiles + pl->n_tiles_hi;
    std::vector<TileDesc> tiles(n_tiles);
    std::vector<TileJob> tjobs(pl->n_tile_jobs);
    if (n_tiles) HIP_TRY(ctx, hipMemcpy(tiles.data(), pl->d_tiles, n_tiles * sizeof(TileDesc), hipMemcpyDeviceToHost));
    if (pl->n_tile_jobs) HIP_TRY(ctx, hipMemcpy(tjobs.data(), pl->d_tjobs, pl->n_tile_jobs * sizeof(TileJob), hipMemcpyDeviceToHost));
    size_t n_spans = 0;
    for (const TileDesc &t : tiles) n_spans = std::max<size_t>(n_spans, (size_t)t.span_first + (t.n_spans & 0x7fffffffu));
    std::vector<TileSpan> spans(n_spans);
    if (n_spans) HIP_TRY(ctx, hipMemcpy(spans.data(), pl->d_spans, n_spans * sizeof(TileSpan), hipMemcpyDeviceToHost));
    std::vector<uint8_t> tseen;
    e = verify_uploaded_tiles(ctx, jobs, n_jobs, pl, tiles.data(), n_tiles, spans.data(), n_spans, tjobs.data(), tjobs.size(), tseen);
    // every job has exactly one home: a tile record or a record of another class
    std::vector<uint8_t> oseen(n_jobs, 0);
    if (e.empty()) {
        const uint64_t n_other = n_jobs - pl->n_tile_jobs;
        for (uint64_t q = 0; q < n_other && e.empty(); q++) {
            const DevJob &d = pl->h_jobs[pl->n_tile_jobs + q];
            const uint32_t k = d.aux;
            if (k >= n_jobs || oseen[k] || tseen[k]) e = "job " + S(k) + " planned twice";
            else if (d.n != jobs[k].n || d.m != jobs[k].m || d.ref_off != jobs[k].ref_off || d.read_off != jobs[k].read_off ||
                     ((d.flags & kFlagExcludeLast) != 0) != (jobs[k].exclude_last != 0))
                e = "record of job " + S(k) + " differs from the job";
            else oseen[k] = 1;
        }
        for (uint64_t k = 0; k < n_jobs && e.empty(); k++)
            if (!tseen[k] && !oseen[k]) e = "job " + S(k) + " is in no launch";
    }
    say(e);
    return e.empty() ? RAWDTW_OK : RAWDTW_ERR_DEVICE + 100;
}

int rawdtw_batch_chunk_profile(rawdtw_ctx *ctx, rawdtw_batch *batch, int flat_map, uint64_t *out, uint32_t cap, uint32_t *n_out)
{
    if (!batch_ok(ctx, batch) || !n_out) return fail(ctx, RAWDTW_ERR_INVALID, "bad arguments to batch_chunk_profile");
    *n_out = 0;
    if (!batch->stream) return RAWDTW_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int st = stream_counters(ctx, batch);
    if (st != RAWDTW_OK) return st;
    if (stream_declined(batch)) return RAWDTW_OK;
    StreamPlanHost h;
    const int sd = stream_plan_download(ctx, batch, h);
    if (sd != RAWDTW_OK) return sd;
    if (!h.v.fits_slots()) return fail(ctx, RAWDTW_ERR_DEVICE, "work list longer than the slots");
    uint64_t w[21];
    if (!stream_chunk_profile(h.v, flat_map != 0, w)) return fail(ctx, RAWDTW_ERR_DEVICE, "work list entry out of range");
    *n_out = 21;
    for (uint32_t i = 0; i < 21 && i < cap && out; i++) out[i] = w[i];
    return RAWDTW_OK;
}

int rawdtw_batch_info(const rawdtw_batch *batch, rawdtw_plan_info_t *info, uint64_t *n_chains)
{
    if (!batch || batch_dead(batch)) return RAWDTW_ERR_INVALID;
    if (n_chains) *n_chains = batch->n_chains;
    if (!info) return RAWDTW_OK;
    if (!batch->stream) return rawdtw_plan_info(batch->plan, info);
    rawdtw_ctx *ctx = batch->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int st = stream_counters(ctx, batch);
    if (st != RAWDTW_OK) return st;
    if (stream_declined(batch)) { // what the job-list path will run
        st = stream_fallback(ctx, batch_owned(batch));
        if (st != RAWDTW_OK) return st;
        return rawdtw_plan_info(batch->plan, info);
    }
    st = stream_stats_home(ctx, batch, true);
    if (st != RAWDTW_OK) return st;
    batch_count_jobs(batch);
    const unsigned long long *c = batch->h_cnt;
    rawdtw_plan_info_t I{};
    I.n_jobs = batch->n_jobs;
    I.cells = c[kCntCells];
    I.algorithmic_bytes = c[kCntTileBytes] + c[kCntOtherBytes];
    unsigned long long side_lane = 0; // the side list's lane-per-job classes count with the tiles' jobs: same body, same class rule
    for (uint32_t q = kClsL0; q < kClsL0 + kClsLCount; q++) side_lane += c[kCntCls0 + q]; // (the 8-slot lane classes stay with the wide bands)
    I.n_lane_jobs = c[kCntTileJobs] + side_lane;
    I.n_wave_band_jobs = c[kCntOthers] - side_lane;
    I.n_full_jobs = 0;
    I.workspace_bytes = batch->ws_bytes;
    I.n_launches = 1;
    *info = I;
    return RAWDTW_OK;
}

// the chain fold (kKindChainFold) or the read select (kKindReadSelect) of a batch enqueued
static int batch_tail(rawdtw_ctx *ctx, rawdtw_batch *b, LaunchKind kind)
{
    hipError_t e;
    const int which = kind == kKindChainFold ? 0 : 1;
    if (ctx->debug_skip_kinds & (1u << kind)) return RAWDTW_OK;
    if (ctx->debug_skip_tail & (1u << which)) return RAWDTW_OK;
    const float *job_cost = b->stream ? b->sa.out_full : b->plan->d_cost;
    if (b->stream && b->fold_fused) {
        if (which == 1) return RAWDTW_OK; // (done by the launch before)
        StreamArgs f = b->sa; // (the fold walks the FULL lists: a chunk round's costs were gathered into out_full)
        f.anchor_off = b->sa.full_off; f.out = b->sa.out_full; f.n_anchors = b->sa.n_full;
        e = stream_gather(b->sa, b->d_chains, ctx->stream);
        if (e == hipSuccess) e = stream_fold_select(f, b->d_chains, b->d_chain_off, b->n_reads, b->opt.match_bonus, b->opt.fused_score, b->opt.min_score, b->d_full,
                               b->d_gate, b->d_score, b->d_keep, ctx->stream);
    } else if (which == 0)
        e = launch_chain_fold(std::min(ctx->fold_mode, 3), b->d_chains, b->d_fold_order, b->n_chains, job_cost, b->opt.match_bonus, b->opt.fused_score,
                              b->d_full, b->d_gate, ctx->fold_long_parts, ctx->stream);
    else
        e = launch_read_select(b->d_chain_off, b->n_reads, b->d_full, b->d_gate, b->opt.min_score, b->d_score,
                               b->d_keep, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, which == 0 ? "chain fold launch" : "read select launch");
    return RAWDTW_OK;
}

// The batch's reported launches (rawdtw_launches.h) under the form it has and the context's settings now: what is timed, collected and
// reported reads this and nothing else.  (An untimed run needs no table.)
static std::vector<BatchLaunch> batch_table(const rawdtw_batch *b)
{
    return b->stream ? batch_launches(b->stream_lds, nullptr, MergeSel{}) : batch_launches(0, &b->plan->launches, merge_of(b->ctx, b->plan));
}

// One run of the batch enqueued.  `e`, when given, holds the run's event pairs: pair i of the `nl` entries of the batch's table.
static int batch_enqueue_one(rawdtw_ctx *ctx, rawdtw_batch *batch, hipEvent_t *e, uint32_t nl)
{
    auto mark = [&](uint32_t i, int stop) { return !e || hipEventRecord(e[event_slot(0, i, nl) + stop], ctx->stream) == hipSuccess; };
    batch->dirty = true;
    if (batch->stream) {
        // The arenas may have been re-uploaded, grown or swapped since the batch was planned (rawdtw_upload_events,
        // rawdtw_events_reserve, rawdtw_upload_reference ... free and reallocate them): the launch reads the context's
        // CURRENT arrays, and the windows -- checked against the sizes at planning time -- must still lie inside them.
        if (ctx->n_ev < batch->sa.n_ev || ctx->n_ref < batch->sa.n_ref)
            return fail(ctx, RAWDTW_ERR_INVALID, "an arena shrank after the batch was created: create the batch again");
        batch->sa.ev = ctx->d_ev; batch->sa.ref = ctx->d_ref;
        // entry 0: the side list (k_wide) -- in line, or (option "wide_beside") forked onto the context's second stream and
        // joined before the fold; entry 1: the tiles' passes (k_runs)
        const bool wide = !(ctx->stream_debug & 4u);
        const bool wide_now = wide && !batch->wide_out; // (the first run's went out with the planning launches)
        batch->wide_out = false;
        if (!mark(0, 0)) return RAWDTW_ERR_DEVICE;
        if (wide_now && ctx->wide_order != 2) {
            const hipError_t he = stream_wide_fork(ctx, batch->sa);
            if (he != hipSuccess) return hip_fail(ctx, he, "side list launch");
        }
        if (!mark(0, 1) || !mark(1, 0)) return RAWDTW_ERR_DEVICE;
        hipError_t he = stream_run(batch->sa, ctx->stream_blocks, batch->stream_lds, batch->stream_threads, batch->stream_runs++ > 0, ctx->stream);
        if (he != hipSuccess) return hip_fail(ctx, he, "batch kernel launch");
        if (!mark(1, 1)) return RAWDTW_ERR_DEVICE;
        if (wide_now && ctx->wide_order == 2) { // (timing experiments: the side list behind the tiles -- and behind entry 1's stop: in no bracket)
            he = stream_wide_fork(ctx, batch->sa);
            if (he != hipSuccess) return hip_fail(ctx, he, "side list launch");
        }
        if (wide && ctx->wide_beside && hipStreamWaitEvent(ctx->stream, ctx->ev_wide_join, 0) != hipSuccess) return RAWDTW_ERR_DEVICE;
    } else if (const int st = run_all_launches(ctx, batch->plan, e)) return st; // (pair i around the plan's launch i: the table keeps the plan's order)
    auto tail = [&](uint32_t i, LaunchKind kind) {
        if (!mark(i, 0)) return (int)RAWDTW_ERR_DEVICE;
        const int st = batch_tail(ctx, batch, kind);
        return st == RAWDTW_OK && !mark(i, 1) ? (int)RAWDTW_ERR_DEVICE : st;
    };
    if (const int st = tail(nl - 2, kKindChainFold)) return st; // the table's last two entries
    return tail(nl - 1, kKindReadSelect);
}

int rawdtw_batch_run(rawdtw_ctx *ctx, rawdtw_batch *batch)
{
    if (const int bad = batch_check(ctx, batch)) return bad;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return batch_enqueue_one(ctx, batch, nullptr, 0);
}

int rawdtw_batch_run_timed(rawdtw_ctx *ctx, rawdtw_batch *batch, float *launch_ms, uint32_t *launch_kind, uint32_t cap,
                           uint32_t *n_launches)
{
    if (launch_ms) return rawdtw_batch_run_reps(ctx, batch, 1, launch_ms, launch_kind, cap, n_launches);
    if (const int bad = batch_check(ctx, batch)) return bad;
    std::vector<float> unread(batch_table(batch).size()); // (a timed run all the same: its collect names the kinds)
    return rawdtw_batch_run_reps(ctx, batch, 1, unread.data(), launch_kind, cap, n_launches);
}

int rawdtw_batch_enqueue(rawdtw_ctx *ctx, rawdtw_batch *batch, int timed)
{
    if (const int bad = batch_check(ctx, batch)) return bad;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!timed) return batch_enqueue_one(ctx, batch, nullptr, 0);
    const uint32_t nl = (uint32_t)batch_table(batch).size();
    const size_t base = event_slot(batch->ev_runs, 0, nl);
    batch->ev.resize(event_slot(batch->ev_runs + 1, 0, nl), nullptr);
    for (size_t k = base; k < batch->ev.size(); k++) if (!batch->ev[k]) HIP_TRY(ctx, hipEventCreate(&batch->ev[k]));
    batch->ev_runs++;
    return batch_enqueue_one(ctx, batch, &batch->ev[base], nl);
}

int rawdtw_batch_collect(rawdtw_ctx *ctx, rawdtw_batch *batch, float *launch_ms, uint32_t *launch_kind, uint32_t cap,
                         uint32_t *n_launches, uint32_t *n_runs)
{
    if (n_launches) *n_launches = 0;
    if (n_runs) *n_runs = 0;
    // (a batch whose redo through the job list failed at fetch has no launches left to report: refused like everywhere else)
    if (const int bad = batch_check(ctx, batch)) return bad;
    const std::vector<BatchLaunch> t = batch_table(batch);
    const uint32_t nl = (uint32_t)t.size();
    if (n_launches) *n_launches = nl;
    if (n_runs) *n_runs = batch->ev_runs;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    batch->dirty = false;
    int st = RAWDTW_OK;
    for (uint32_t i = 0; i < nl && i < cap; i++) {
        double acc = 0;
        for (uint32_t r = 0; r < batch->ev_runs; r++) {
            float ms = 0.f;
            const size_t b = event_slot(r, i, nl);
            if (hipEventElapsedTime(&ms, batch->ev[b], batch->ev[b + 1]) != hipSuccess) st = RAWDTW_ERR_DEVICE;
            acc += ms;
        }
        if (launch_ms) launch_ms[i] = batch->ev_runs ? (float)(acc / batch->ev_runs) : 0.f;
        if (launch_kind) launch_kind[i] = t[i].word();
    }
    for (auto &e : batch->ev) if (e) (void)hipEventDestroy(e);
    batch->ev.clear();
    batch->ev_runs = 0;
    if (st != RAWDTW_OK && ctx->err.empty()) ctx->err = "collect failed";
    return st;
}

int rawdtw_batch_run_reps(rawdtw_ctx *ctx, rawdtw_batch *batch, uint32_t reps, float *launch_ms, uint32_t *launch_kind,
                          uint32_t cap, uint32_t *n_launches)
{
    if (const int bad = batch_check(ctx, batch)) return bad;
    if (n_launches) *n_launches = (uint32_t)batch_table(batch).size();
    int st = RAWDTW_OK;
    for (uint32_t r = 0; r < reps && st == RAWDTW_OK; r++) st = rawdtw_batch_enqueue(ctx, batch, launch_ms != nullptr);
    if (launch_ms) {
        int st2 = rawdtw_batch_collect(ctx, batch, launch_ms, launch_kind, cap, nullptr, nullptr);
        if (st == RAWDTW_OK) st = st2;
    } else {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess && st == RAWDTW_OK) st = RAWDTW_ERR_DEVICE;
        batch->dirty = false;
    }
    return st;
}

int rawdtw_batch_launch_stats(const rawdtw_batch *batch, uint32_t i, uint32_t *kind, int32_t *param, uint64_t *n_jobs,
                              uint64_t *algorithmic_bytes, uint64_t *cells)
{
    if (!batch || batch_dead(batch)) return RAWDTW_ERR_INVALID;
    std::vector<BatchLaunch> t = batch_table(batch);
    if (i >= t.size()) return RAWDTW_ERR_INVALID;
    const bool tail = i + 2 >= t.size(); // fold or select
    rawdtw_plan_info_t I{};
    if (batch->stream && !tail) { // the device's statistics (every job, byte and cell is counted in exactly one of the two launches)
        int st = cells ? rawdtw_batch_info(batch, &I, nullptr) : stream_counters(batch->ctx, batch);
        if (st == RAWDTW_OK && !cells) st = stream_stats_home(batch->ctx, batch, false);
        if (st != RAWDTW_OK) return st;
        if (!batch->stream) { // (rawdtw_batch_info has moved the batch to the job-list path)
            t = batch_table(batch);
            if (i + 2 >= t.size()) return RAWDTW_ERR_INVALID;
        }
    }
    const BatchLaunch &E = t[i];
    uint64_t bytes = 0, cl = 0, nj = 0;
    if (tail) {
        const bool fold = E.kind == kKindChainFold;
        batch_count_jobs(batch);
        nj = fold ? batch->n_chains : batch->n_reads;
        // fold: one 4-byte cost per job + a 24-byte descriptor and two 4-byte results per chain;
        // select: 8 bytes read and 5 written per chain
        bytes = fold ? batch->n_jobs * 4 + batch->n_chains * 32 : batch->n_chains * 13 + batch->n_reads * 8;
    } else if (batch->stream) {
        const unsigned long long *c = batch->h_cnt;
        batch_count_jobs(batch);
        const uint64_t n_side = std::min<uint64_t>(c[kCntOthers], batch->sa.others_cap);
        uint64_t side_cells = 0;
        if (cells && n_side) {
            std::vector<DevJob> side(n_side);
            if (hipMemcpy(side.data(), batch->sa.ojobs, n_side * sizeof(DevJob), hipMemcpyDeviceToHost) != hipSuccess) return RAWDTW_ERR_DEVICE;
            for (const DevJob &d : side) side_cells += banded_cells(d.n, d.m, d.R);
        }
        const bool wide = i == 0; // (entry 0 is the side list's launch)
        nj = wide ? n_side : batch->n_jobs - std::min<uint64_t>(n_side, batch->n_jobs);
        bytes = wide ? c[kCntOtherBytes] : c[kCntTileBytes];
        cl = wide ? side_cells : I.cells - std::min<uint64_t>(side_cells, I.cells);
    } else {
        const rawdtw_plan *pl = batch->plan;
        auto add = [&](const Launch &X) {
            for (uint64_t p = X.first; p < X.first + X.count; p++) {
                const DevJob &d = pl->h_jobs[p];
                bytes += 4ull * ((uint64_t)d.n + d.m) + 4 + 32;
            }
            if (cells) cl += count_cells(pl, X.first, X.first + X.count);
            nj += X.count;
        };
        // the merged launch reports the classes it carries; a carried launch nothing of its own
        if (E.kind == kKindBandMerged) { for (const BatchLaunch &X : t) if (X.carried || X.plan == E.plan) add(pl->launches[X.plan]); }
        else if (!E.carried) add(pl->launches[E.plan]);
    }
    if (kind) *kind = E.kind;
    if (param) *param = E.param;
    if (n_jobs) *n_jobs = nj;
    if (algorithmic_bytes) *algorithmic_bytes = bytes;
    if (cells) *cells = cl;
    return RAWDTW_OK;
}

int rawdtw_batch_fetch(rawdtw_ctx *ctx, rawdtw_batch *batch, float *score, uint8_t *keep, float *job_cost)
{
    if (const int bad = batch_check(ctx, batch)) return bad;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int attempt = 0; attempt < 2; attempt++) {
        const float *d_cost = batch->stream ? batch->sa.out_full : batch->plan->d_cost;
        // a sync-free batch: counters, scores and keep flags in one copy into the batch's pinned block, and from there into the
        // caller's arrays (200 KB of host copying against two more operations on the stream)
        const bool block = batch->stream && batch->n_chains && (score || keep);
        if (block) HIP_TRY(ctx, hipMemcpyAsync(batch->h_cnt, batch->sa.cnt, batch->res_bytes, hipMemcpyDeviceToHost, ctx->stream));
        else if (batch->n_chains) {
            if (score) HIP_TRY(ctx, hipMemcpyAsync(score, batch->d_score, batch->n_chains * 4, hipMemcpyDeviceToHost, ctx->stream));
            if (keep) HIP_TRY(ctx, hipMemcpyAsync(keep, batch->d_keep, batch->n_chains, hipMemcpyDeviceToHost, ctx->stream));
        }
        // (a sync-free batch keeps one cost per ANCHOR: the part that ends there; they are put into job order below)
        std::vector<float> per_anchor;
        if (job_cost && batch->stream && batch->sa.n_full) {
            try { per_anchor.resize(batch->sa.n_full); } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
            HIP_TRY(ctx, hipMemcpyAsync(per_anchor.data(), d_cost, batch->sa.n_full * 4, hipMemcpyDeviceToHost, ctx->stream));
        } else if (job_cost && !batch->stream && batch->n_jobs)
            HIP_TRY(ctx, hipMemcpyAsync(job_cost, d_cost, batch->n_jobs * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (batch->stream && !batch->cnt_valid && !block)
            HIP_TRY(ctx, hipMemcpyAsync(batch->h_cnt, batch->sa.cnt, stream::kCounterBytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        batch->dirty = false;
        if (!batch->stream) return RAWDTW_OK;
        batch->cnt_valid = true;
        if (!stream_declined(batch)) {
            if (block) {
                if (score) memcpy(score, batch->h_score, batch->n_chains * 4);
                if (keep) memcpy(keep, batch->h_keep, batch->n_chains);
            }
            if (job_cost) { // chain c's part p (rmap.cpp:248-293) ends at anchor a1 - 2 - p
                const uint64_t *aoff = batch->in.anchor_off;
                uint64_t k = 0;
                for (uint64_t c = 0; c < batch->n_chains; c++) {
                    const uint64_t a0 = aoff[c], a1 = aoff[c + 1];
                    for (uint64_t pidx = 0; a1 > a0 && pidx + 1 < a1 - a0; pidx++) job_cost[k++] = per_anchor[a1 - 2 - pidx];
                }
            }
            return RAWDTW_OK;
        }
        int st = stream_fallback(ctx, batch); // invalid anchors (the job-list path words the error) or a shape it does not take
        if (st != RAWDTW_OK) return st;
    }
    return RAWDTW_OK;
}

int rawdtw_batch_hand_over_stats(const rawdtw_batch *batch, uint64_t *records_on_device, uint64_t *bytes_to_device, uint64_t *bytes_to_host)
{
    if (!batch) return RAWDTW_ERR_INVALID;
    if (records_on_device) *records_on_device = batch->local_records;
    if (bytes_to_device) *bytes_to_device = batch->link_up;
    if (bytes_to_host) *bytes_to_host = batch->link_home;
    return RAWDTW_OK;
}

int rawdtw_batch_plan_ms(rawdtw_ctx *ctx, rawdtw_batch *batch, float *ms)
{
    if (!ctx || !batch || batch->ctx != ctx || !ms) return fail(ctx, RAWDTW_ERR_INVALID, "bad arguments to batch_plan_ms");
    *ms = 0.0f;
    if (!batch->stream || !batch->ev_plan[0] || !batch->ev_plan[3]) return RAWDTW_OK;
    HIP_TRY(ctx, hipEventSynchronize(batch->ev_plan[3]));
    float scan = 0.f, plan = 0.f; // (the side list's launch between them is DTW work: rawdtw_batch_wide_ms)
    HIP_TRY(ctx, hipEventElapsedTime(&scan, batch->ev_plan[0], batch->ev_plan[1]));
    HIP_TRY(ctx, hipEventElapsedTime(&plan, batch->ev_plan[2], batch->ev_plan[3]));
    *ms = scan + plan;
    return RAWDTW_OK;
}

int rawdtw_batch_wide_ms(rawdtw_ctx *ctx, rawdtw_batch *batch, float *ms)
{
    if (!ctx || !batch || batch->ctx != ctx || !ms) return fail(ctx, RAWDTW_ERR_INVALID, "bad arguments to batch_wide_ms");
    *ms = 0.0f;
    if (!batch->stream || !batch->ev_plan[1] || !batch->ev_plan[2]) return RAWDTW_OK;
    HIP_TRY(ctx, hipEventSynchronize(batch->ev_plan[2]));
    HIP_TRY(ctx, hipEventElapsedTime(ms, batch->ev_plan[1], batch->ev_plan[2]));
    return RAWDTW_OK;
}

int rawdtw_batch_stream_counter_index(const char *name)
{
    static const struct { const char *name; int index; } table[] = {
        {"bad", kCntBad}, {"overflow", kCntOverflow}, {"unsupported", kCntUnsupported}, {"side_jobs", kCntOthers}, {"class0", kCntCls0},
        {"cells", kCntCells}, {"tile_jobs", kCntTileJobs}, {"tile_bytes", kCntTileBytes}, {"side_bytes", kCntOtherBytes}, {"todo", kCntTodo},
        {"reused", kCntReused}, {"pool", kCntPool}, {"stamp0", kCntStamp0}};
    if (!name) return -1;
    for (const auto &t : table) if (strcmp(name, t.name) == 0) return t.index;
    return -1;
}

int rawdtw_batch_stream_counters(rawdtw_ctx *ctx, rawdtw_batch *batch, uint64_t *out, uint32_t cap, uint32_t *n_out)
{
    if (!ctx || !batch || batch->ctx != ctx || !n_out) return fail(ctx, RAWDTW_ERR_INVALID, "bad arguments to batch_stream_counters");
    *n_out = 0;
    if (!batch->stream) return RAWDTW_OK;
    batch->cnt_valid = false; // (a diagnostic call: runs since the last look have moved the phase stamps on)
    const int st = stream_counters(ctx, batch);
    if (st != RAWDTW_OK) return st;
    const uint32_t n = (uint32_t)kCntHeads; // (the queue heads behind them are the kernel's scratch)
    *n_out = n;
    for (uint32_t i = 0; i < n && i < cap && out; i++) out[i] = batch->h_cnt[i];
    return RAWDTW_OK;
}


int rawdtw_batch_fetch_destroy(rawdtw_ctx *ctx, rawdtw_batch *batch, float *score, uint8_t *keep)
{
    const int st = rawdtw_batch_fetch(ctx, batch, score, keep, nullptr);
    if (batch && batch->ctx == ctx) rawdtw_batch_destroy(batch); // (a batch of another context is the caller's mistake, not ours to free)
    return st;
}

// everything of a batch that lives on the device or in its context's pools; `ctx` = the batch's context
} // extern "C"
namespace rawdtw { namespace capi {
void batch_detach(rawdtw_ctx *ctx, rawdtw_batch *b)
{
    round_end_forget(ctx, b); // (before the arrays a pending round end reads go)
    keep_forget(ctx, b);      // (... and a pending keep launch)
    for (auto &e : b->ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : b->ev_plan) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    b->ev.clear(); b->ev_runs = 0;
    batch_release_device(b); // (also destroys the job-list plan, which unregisters itself)
    ws_release(ctx, b->ws);
    b->stream = false;       // neither form left: every entry point but destroy refuses the batch (batch_dead)
}

int batch_settle(rawdtw_ctx *ctx, rawdtw_batch *b, bool *redone)
{
    *redone = false;
    if (!b->stream) return RAWDTW_OK;
    int st = stream_counters(ctx, b);
    if (st != RAWDTW_OK || !stream_declined(b)) return st;
    *redone = true;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (the counters may have come home earlier: nothing may still read the workspace the fall-back gives back)
    b->dirty = false;
    return stream_fallback(ctx, b);
}
} } // namespace rawdtw::capi
extern "C" {

int rawdtw_batch_destroy(rawdtw_batch *b)
{
    if (!b) return RAWDTW_OK;
    if (rawdtw_ctx *ctx = b->ctx) { // (null: rawdtw_destroy came first and took the device side with it)
        (void)hipSetDevice(ctx->device);
        if (b->dirty) (void)hipStreamSynchronize(ctx->stream); // its workspace goes back to the pool
        batch_detach(ctx, b);
        unregister(ctx->live_batches, b);
    }
    delete b;
    return RAWDTW_OK;
}

} // extern "C"
