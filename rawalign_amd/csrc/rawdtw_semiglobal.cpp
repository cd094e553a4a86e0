// rawdtw_semiglobal.cpp -- subsequence DTW behind the C ABI: rawdtw_semiglobal_batch, rawdtw_semiglobal_span_batch,
// rawdtw_semiglobal_traceback_steps and the single-call drop-ins for DTW_semiglobal / DTW_semiglobal_tb (dtw.hpp; dtw.cpp:526-593,
// 669-753) and for the span.  Host code only: validation, the jobs' classes and their launches; the traceback's sub-batches are the
// driver's (rawdtw_tb_driver.cpp).  The job-list planner (rawdtw_planner.cpp) knows nothing of these jobs: they are bucketed here, by
// the class rawdtw_semiglobal.h defines, longest first inside a class (a launch takes as long as its longest job).  There is no CPU
// fallback: the kernels run or the call returns an error status.
#include "rawdtw_capi.h"
#include "rawdtw_semiglobal.h"
#include "rawdtw_semi_window.h"
#include "rawdtw_tb_driver.h"

using namespace rawdtw;
using namespace rawdtw::capi;

namespace {

enum class SemiForm { Cost, Traceback, Span };

// columns (the traceback form only; rawdtw_semi_window.h): the window width; a class's windowed jobs (m > columns) follow its other
// jobs as a launch of their own (ClassLaunch::max_k = 1), and a windowed job's stretch of the direction workspace is one window's
// directions and its checkpoints.  0: no job is windowed, and keys, order and launches are what they were without the argument.
void semi_plan(const rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t cnt, SemiForm form, ClassPlan &pl, uint32_t columns = 0)
{
    std::vector<Keyed> keyed(cnt);
    const uint64_t lim = (1ull << 28) - 1;
    for (uint64_t k = 0; k < cnt; k++) {
        const rawdtw_job_t &j = jobs[k];
        const uint64_t c = (uint64_t)semi_class(j.n, j.m, ctx->full_wg);
        const uint64_t w = form == SemiForm::Traceback && semi_window::windowed(j.m, columns) ? 1 : 0;
        keyed[k] = Keyed{(c << 57) | (w << 56) | ((lim - std::min<uint64_t>(j.m, lim)) << 28) | (lim - std::min<uint64_t>(j.n, lim)), (uint32_t)k};
    }
    sort_keyed(keyed);
    pl.order.resize(cnt); pl.jobs.resize(cnt); pl.aux.assign(cnt, FullAux{0, 0});
    for (uint64_t p = 0; p < cnt; p++) {
        const uint32_t k = keyed[p].idx;
        const rawdtw_job_t &j = jobs[k];
        const int c = (int)(keyed[p].key >> 57);
        const uint32_t w = (uint32_t)(keyed[p].key >> 56) & 1u;
        pl.order[p] = k;
        DevJob &d = pl.jobs[p];
        d.ref_off = j.ref_off; d.read_off = j.read_off; d.n = j.n; d.m = j.m; d.R = -1;
        d.flags = j.exclude_last ? kFlagExcludeLast : 0u; d.aux = k;
        pl.aux[p].bnd_off = pl.bnd_floats;
        pl.bnd_floats += form == SemiForm::Span ? semi_span_bnd_floats(j.n, j.m, c) : semi_bnd_floats(j.n, j.m, c);
        if (form == SemiForm::Traceback) {
            pl.aux[p].dir_off = pl.dir_bytes;
            pl.dir_bytes += w ? semi_window::job_bytes(j.n, j.m, columns, (uint32_t)semi_rpl(c)) : (semi_dir_bytes(j.n, j.m, c) + 255) & ~255ull;
        }
        if (pl.launches.empty() || pl.launches.back().cls != c || pl.launches.back().max_k != w) pl.launches.push_back(ClassLaunch{c, p, 0, w});
        pl.launches.back().count++;
    }
}

// Every refusal, before anything is enqueued: INVALID for a zero length or a banded job, RANGE for a window outside the arenas.
int semi_check(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, bool arena, uint64_t n_events)
{
    if (arena && !ctx->d_ev) return fail(ctx, RAWDTW_ERR_INVALID, "the context has no event arena");
    if (!ctx->d_ref) return fail(ctx, RAWDTW_ERR_INVALID, "the context has no reference arena");
    const uint64_t n_ev = arena ? ctx->n_ev : n_events;
    for (uint64_t k = 0; k < n_jobs; k++) {
        const rawdtw_job_t &j = jobs[k];
        if (j.n == 0 || j.m == 0 || j.n >= 0x7fffffffu || j.m >= 0x7fffffffu)
            return fail(ctx, RAWDTW_ERR_INVALID, "job " + std::to_string(k) + ": zero length (dtw.cpp:527-528, 670 assert)");
        if (j.band_radius != RAWDTW_FULL)
            return fail(ctx, RAWDTW_ERR_INVALID, "job " + std::to_string(k) + ": a semiglobal job has no band (band_radius must be RAWDTW_FULL)");
        if ((uint64_t)j.read_off + j.n > n_ev || j.ref_off > ctx->n_ref || j.ref_off + j.m > ctx->n_ref)
            return fail(ctx, RAWDTW_ERR_RANGE, "job " + std::to_string(k) + ": window outside the arenas");
    }
    return RAWDTW_OK;
}

// records up, fill launches of one plan; cost and end_j (the span form: and j0, in the slot's extra word) are left on the device (indexed
// inside the stretch)
int semi_fill(rawdtw_ctx *ctx, const ClassPlan &pl, SemiForm form, const TbSlot &slot, uint8_t *d_dir)
{
    const uint64_t cnt = pl.jobs.size();
    HIP_TRY(ctx, hipMemcpyAsync(slot.jobs, pl.jobs.data(), cnt * sizeof(DevJob), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(slot.aux, pl.aux.data(), cnt * sizeof(FullAux), hipMemcpyHostToDevice, ctx->stream));
    for (const ClassLaunch &L : pl.launches) {
        hipError_t e = form == SemiForm::Span
                           ? launch_semi_span_wave(L.cls, slot.jobs + L.first, L.count, slot.aux + L.first, ctx->d_ev, ctx->d_ref, slot.cost, slot.extra,
                                                   slot.endj, slot.bnd, ctx->stream)
                           : launch_semi_wave(L.cls, form == SemiForm::Traceback, slot.jobs + L.first, L.count, slot.aux + L.first, ctx->d_ev,
                                              ctx->d_ref, slot.cost, slot.endj, slot.bnd, d_dir, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "semiglobal fill launch");
    }
    return RAWDTW_OK;
}

// the cost form (out_j0 unused) and the span form: one pass, no sub-batches, nothing but boundary rows in the workspace
int semi_batch(rawdtw_ctx *ctx, SemiForm form, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events, uint64_t n_events,
               float *out_cost, uint32_t *out_j0, uint32_t *out_end_j)
{
    const bool span = form == SemiForm::Span;
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (n_jobs == 0) return RAWDTW_OK;
    if (!jobs || !out_cost || !out_end_j || (span && !out_j0)) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n_jobs >= 0x7fffffffull) return fail(ctx, RAWDTW_ERR_INVALID, "too many jobs for one call");
    const bool arena = h_events == nullptr;
    int st = semi_check(ctx, jobs, n_jobs, arena, n_events);
    if (st != RAWDTW_OK) return st;
    if (!arena && (st = rawdtw_upload_events(ctx, h_events, n_events)) != RAWDTW_OK) return st;
    ClassPlan pl;
    semi_plan(ctx, jobs, n_jobs, form, pl);
    DevBlock blk(ctx, "semiglobal");
    const tb::Recs R = tb::recs(n_jobs, sizeof(DevJob), sizeof(FullAux), true, span, pl.bnd_floats);
    if ((st = blk.reserve(R.need)) != RAWDTW_OK) return st;
    const TbSlot slot{reinterpret_cast<DevJob *>(blk.p + R.jobs.at), reinterpret_cast<FullAux *>(blk.p + R.aux.at), reinterpret_cast<float *>(blk.p + R.cost.at),
                      reinterpret_cast<uint32_t *>(blk.p + R.endj.at), reinterpret_cast<float *>(blk.p + R.bnd.at), nullptr, nullptr,
                      reinterpret_cast<uint32_t *>(blk.p + R.j0.at), nullptr, nullptr, nullptr, nullptr}; // (no paths; extra: the span form's j0)
    EventPair ev;
    for (int k = 0; k < 2; k++) HIP_TRY(ctx, hipEventCreate(&ev.e[k]));
    ctx->semi = TbTiming{};
    HIP_TRY(ctx, hipEventRecord(ev.e[0], ctx->stream));
    if ((st = semi_fill(ctx, pl, form, slot, nullptr)) != RAWDTW_OK) return st;
    HIP_TRY(ctx, hipEventRecord(ev.e[1], ctx->stream));
    // (a record's aux is the caller's job index: the results come home in job order)
    HIP_TRY(ctx, hipMemcpyAsync(out_cost, slot.cost, n_jobs * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out_end_j, slot.endj, n_jobs * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (span) HIP_TRY(ctx, hipMemcpyAsync(out_j0, slot.extra, n_jobs * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) ctx->semi.fill_ms = ms;
    return RAWDTW_OK;
}

// The semiglobal path as the driver takes it (rawdtw_tb_driver.h): a stretch's records (job, aux, cost, end_j, boundary rows) lie in the
// slot; the extra word a job is j0, the path's first column.
uint64_t semi_job_dir_bytes(const rawdtw_ctx *ctx, const rawdtw_job_t &j) { return semi_dir_bytes(j.n, j.m, semi_class(j.n, j.m, ctx->full_wg)) + 256; }
int semi_stretch(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t cnt, TbStretch *out)
{
    ClassPlan *pl = new ClassPlan;
    semi_plan(ctx, jobs, cnt, SemiForm::Traceback, *pl);
    *out = class_stretch(pl, true);
    return RAWDTW_OK;
}
int semi_tb_fill(rawdtw_ctx *ctx, const TbStretch &s, const TbSlot &slot)
{
    return semi_fill(ctx, *static_cast<const ClassPlan *>(s.plan), SemiForm::Traceback, slot, ctx->d_tb_dir);
}
int semi_tb_walk(rawdtw_ctx *ctx, const TbStretch &s, const TbSlot &slot)
{
    const ClassPlan &pl = *static_cast<const ClassPlan *>(s.plan);
    for (const ClassLaunch &L : pl.launches) {
        hipError_t e = launch_semi_walk(L.cls, slot.jobs + L.first, L.count, slot.aux + L.first, ctx->d_ev, ctx->d_ref, ctx->d_tb_dir, slot.endj,
                                        slot.poff + L.first, slot.plen + L.first, slot.extra + L.first, slot.ti, slot.tj, slot.mv, slot.pd, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "semiglobal walk launch");
    }
    return RAWDTW_OK;
}

// The windowed form of the same (include/rawdtw.h, "semiglobal, in windows"; the context's rawdtw_set_semiglobal_window): a stretch's
// windowed launches fill with k_semi_ckpt_wave (cost, end_j and the checkpoint columns) and walk with k_semi_window + k_semi_finish; its
// jobs with m <= columns take the launches above, records and all.  Nothing here waits for the device.
uint64_t semi_win_job_dir_bytes(const rawdtw_ctx *ctx, const rawdtw_job_t &j)
{
    if (!semi_window::windowed(j.m, ctx->semi_window)) return semi_job_dir_bytes(ctx, j);
    return semi_window::job_bytes(j.n, j.m, ctx->semi_window, (uint32_t)semi_rpl(semi_class(j.n, j.m, ctx->full_wg)));
}
int semi_win_stretch(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t cnt, TbStretch *out)
{
    ClassPlan *pl = new ClassPlan;
    semi_plan(ctx, jobs, cnt, SemiForm::Traceback, *pl, ctx->semi_window);
    *out = class_stretch(pl, true);
    return RAWDTW_OK;
}
int semi_win_fill(rawdtw_ctx *ctx, const TbStretch &s, const TbSlot &slot)
{
    const ClassPlan &pl = *static_cast<const ClassPlan *>(s.plan);
    const uint64_t cnt = pl.jobs.size();
    HIP_TRY(ctx, hipMemcpyAsync(slot.jobs, pl.jobs.data(), cnt * sizeof(DevJob), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(slot.aux, pl.aux.data(), cnt * sizeof(FullAux), hipMemcpyHostToDevice, ctx->stream));
    for (const ClassLaunch &L : pl.launches) {
        hipError_t e = L.max_k ? launch_semi_ckpt_wave(L.cls, slot.jobs + L.first, L.count, slot.aux + L.first, ctx->d_ev, ctx->d_ref, slot.cost, slot.endj,
                                                       slot.bnd, ctx->d_tb_dir, ctx->semi_window, ctx->stream)
                               : launch_semi_wave(L.cls, true, slot.jobs + L.first, L.count, slot.aux + L.first, ctx->d_ev, ctx->d_ref, slot.cost, slot.endj,
                                                  slot.bnd, ctx->d_tb_dir, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "semiglobal fill launch");
    }
    return RAWDTW_OK;
}
int semi_win_walk(rawdtw_ctx *ctx, const TbStretch &s, const TbSlot &slot)
{
    const ClassPlan &pl = *static_cast<const ClassPlan *>(s.plan);
    for (const ClassLaunch &L : pl.launches) {
        hipError_t e = L.max_k ? launch_semi_window(L.cls, slot.jobs + L.first, L.count, slot.aux + L.first, ctx->d_ev, ctx->d_ref, slot.bnd, ctx->d_tb_dir, slot.endj,
                                                    slot.poff + L.first, slot.plen + L.first, slot.extra + L.first, slot.ti, slot.tj, slot.mv, slot.pd,
                                                    ctx->semi_window, ctx->d_semi_win_stats, ctx->stream)
                               : launch_semi_walk(L.cls, slot.jobs + L.first, L.count, slot.aux + L.first, ctx->d_ev, ctx->d_ref, ctx->d_tb_dir, slot.endj,
                                                  slot.poff + L.first, slot.plen + L.first, slot.extra + L.first, slot.ti, slot.tj, slot.mv, slot.pd, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "semiglobal walk launch");
    }
    return RAWDTW_OK;
}

// Exactly one of path_step and (path_i, path_j) is given.
int semi_traceback(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events, uint64_t n_events, float *out_cost,
                   uint32_t *out_j0, const uint64_t *path_off, uint32_t *path_len, uint8_t *path_step, uint32_t *path_i, uint32_t *path_j,
                   float *path_d)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (n_jobs == 0) return RAWDTW_OK;
    if (!jobs || !out_cost || !out_j0 || !path_off || !path_len || !path_d || (!path_step && (!path_i || !path_j)))
        return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n_jobs >= 0x7fffffffull) return fail(ctx, RAWDTW_ERR_INVALID, "too many jobs for one call");
    const bool arena = h_events == nullptr;
    int st = semi_check(ctx, jobs, n_jobs, arena, n_events);
    if (st != RAWDTW_OK) return st;
    if (!arena && (st = rawdtw_upload_events(ctx, h_events, n_events)) != RAWDTW_OK) return st;
    static const TbPath semiglobal{&rawdtw_ctx::semi, false, true, "semiglobal workspace allocation failed", semi_job_dir_bytes, semi_stretch, semi_tb_fill,
                                   semi_tb_walk, class_release};
    static const TbPath windowed{&rawdtw_ctx::semi, false, true, "semiglobal workspace allocation failed", semi_win_job_dir_bytes, semi_win_stretch, semi_win_fill,
                                 semi_win_walk, class_release};
    ctx->semi_win_jobs = ctx->semi_win_windows = ctx->semi_win_max = ctx->semi_win_ckpt_bytes = 0;
    const TbOut out{out_cost, out_j0, path_off, path_len, path_step, path_i, path_j, path_d};
    uint64_t win_jobs = 0, ckpt_bytes = 0;
    for (uint64_t k = 0; k < n_jobs; k++)
        if (semi_window::windowed(jobs[k].m, ctx->semi_window)) {
            win_jobs++;
            ckpt_bytes += semi_window::ckpt_bytes(jobs[k].n, jobs[k].m, ctx->semi_window);
        }
    if (!win_jobs) return tb_run(ctx, semiglobal, jobs, n_jobs, out, nullptr); // (setter off, or short-b jobs only: the call as it was)
    // the window kernel's two counters: zeroed in front of the call's first launch, read once the driver has returned (its streams are idle)
    if (!ctx->d_semi_win_stats) HIP_TRY(ctx, hipMalloc(&ctx->d_semi_win_stats, 2 * sizeof(unsigned long long)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_semi_win_stats, 0, 2 * sizeof(unsigned long long), ctx->stream));
    if ((st = tb_run(ctx, windowed, jobs, n_jobs, out, nullptr)) != RAWDTW_OK) return st;
    unsigned long long got[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpy(got, ctx->d_semi_win_stats, sizeof(got), hipMemcpyDeviceToHost));
    ctx->semi_win_jobs = win_jobs; ctx->semi_win_ckpt_bytes = ckpt_bytes;
    ctx->semi_win_windows = got[0]; ctx->semi_win_max = got[1];
    return RAWDTW_OK;
}

} // namespace

// semi_plan and semi_fill in the form a batch owns (rawdtw_capi.h): the cost form's plan laid into a rawdtw_plan, so that a local batch is a
// job-list batch in everything but its launches -- run, timed runs, launch statistics, fetch and the fold read the plan as they read the
// planner's.  Refusals as rawdtw_semiglobal_batch's, before anything is enqueued.
namespace rawdtw { namespace capi {
int build_semi_plan(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, rawdtw_plan **out)
{
    *out = nullptr;
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (n_jobs > 0 && !jobs) return fail(ctx, RAWDTW_ERR_INVALID, "jobs is NULL");
    if (n_jobs >= 0x7fffffffull) return fail(ctx, RAWDTW_ERR_INVALID, "too many jobs for one call");
    int st = n_jobs ? semi_check(ctx, jobs, n_jobs, true, 0) : RAWDTW_OK;
    if (st != RAWDTW_OK) return st;
    rawdtw_plan *pl = new (std::nothrow) rawdtw_plan;
    if (!pl) return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    pl->ctx = ctx;
    ClassPlan sp;
    try {
        semi_plan(ctx, jobs, n_jobs, SemiForm::Cost, sp);
        pl->order.resize(n_jobs); pl->h_jobs.resize(n_jobs);
        pl->h_aux = sp.aux;
        pl->run_order.resize(sp.launches.size());
    } catch (const std::bad_alloc &) { delete pl; return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    pl->n_jobs = n_jobs;
    pl->bnd_floats = sp.bnd_floats;
    for (uint64_t p = 0; p < n_jobs; p++) {
        pl->order[p] = sp.order[p]; pl->h_jobs[p] = sp.jobs[p];
        pl->need_ev = std::max<uint64_t>(pl->need_ev, (uint64_t)sp.jobs[p].read_off + sp.jobs[p].n);
        pl->need_ref = std::max<uint64_t>(pl->need_ref, sp.jobs[p].ref_off + sp.jobs[p].m);
        pl->info.algorithmic_bytes += 4ull * ((uint64_t)sp.jobs[p].n + sp.jobs[p].m) + 4 + 32;
    }
    for (const ClassLaunch &L : sp.launches) // (class order is longest last: the launches run in that order, as semi_fill's)
        pl->launches.push_back(Launch{kKindSemiWave, wave_class_param(L.cls), L.first, L.count});
    for (uint32_t i = 0; i < pl->run_order.size(); i++) pl->run_order[i] = i;
    pl->info.n_jobs = n_jobs; pl->info.n_full_jobs = n_jobs; pl->info.n_launches = (uint32_t)pl->launches.size();
    pl->info.workspace_bytes = n_jobs * (sizeof(DevJob) + sizeof(FullAux) + 8) + sp.bnd_floats * 4;
    ctx->live_plans.push_back(pl);
    if ((st = dev_alloc(ctx, &pl->d_jobs, n_jobs)) != RAWDTW_OK || (st = dev_alloc(ctx, &pl->d_aux, n_jobs)) != RAWDTW_OK ||
        (st = dev_alloc(ctx, &pl->d_cost, n_jobs)) != RAWDTW_OK || (st = dev_alloc(ctx, &pl->d_end_j, n_jobs)) != RAWDTW_OK ||
        (st = dev_alloc(ctx, &pl->d_bnd, pl->bnd_floats)) != RAWDTW_OK) {
        rawdtw_plan_destroy(pl);
        return st;
    }
    if (n_jobs) {
        hipError_t e = hipMemcpyAsync(pl->d_jobs, pl->h_jobs.data(), n_jobs * sizeof(DevJob), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(pl->d_aux, pl->h_aux.data(), n_jobs * sizeof(FullAux), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { rawdtw_plan_destroy(pl); return hip_fail(ctx, e, "uploading job descriptors"); }
    }
    *out = pl;
    return RAWDTW_OK;
}
} } // namespace rawdtw::capi

extern "C" {

int rawdtw_semiglobal_batch(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events, uint64_t n_events,
                            float *out_cost, uint32_t *out_end_j)
{
    return semi_batch(ctx, SemiForm::Cost, jobs, n_jobs, h_events, n_events, out_cost, nullptr, out_end_j);
}

int rawdtw_semiglobal_span_batch(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events, uint64_t n_events,
                                 float *out_cost, uint32_t *out_j0, uint32_t *out_end_j)
{
    return semi_batch(ctx, SemiForm::Span, jobs, n_jobs, h_events, n_events, out_cost, out_j0, out_end_j);
}

int rawdtw_semiglobal_traceback_steps(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events, uint64_t n_events,
                                      float *out_cost, uint32_t *out_j0, const uint64_t *path_off, uint32_t *path_len, uint8_t *path_step,
                                      float *path_d)
{
    if (ctx && n_jobs && !path_step) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    return semi_traceback(ctx, jobs, n_jobs, h_events, n_events, out_cost, out_j0, path_off, path_len, path_step, nullptr, nullptr, path_d);
}

int rawdtw_semiglobal_timing(const rawdtw_ctx *ctx, float *fill_ms, float *walk_ms, uint64_t *direction_bytes, uint64_t *path_elements)
{
    return tb_timing_get(ctx, &rawdtw_ctx::semi, fill_ms, walk_ms, direction_bytes, path_elements);
}

int rawdtw_semiglobal_window_stats(const rawdtw_ctx *ctx, uint64_t *jobs_windowed, uint64_t *windows, uint64_t *max_windows_a_job, uint64_t *checkpoint_bytes)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (jobs_windowed) *jobs_windowed = ctx->semi_win_jobs;
    if (windows) *windows = ctx->semi_win_windows;
    if (max_windows_a_job) *max_windows_a_job = ctx->semi_win_max;
    if (checkpoint_bytes) *checkpoint_bytes = ctx->semi_win_ckpt_bytes;
    return RAWDTW_OK;
}

int rawdtw_dtw_semiglobal(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m, int exclude_last, float *cost)
{
    (void)exclude_last; // DTW_semiglobal takes the argument and never reads it (dtw.cpp:526-550)
    if (!ctx || !a || !b || !cost) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n == 0 || m == 0) return fail(ctx, RAWDTW_ERR_INVALID, "zero length (dtw.cpp:527-528 assert)");
    PrivateRef pr(ctx);
    int st = pr.put(b, m);
    if (st != RAWDTW_OK) return st;
    rawdtw_job_t j{0, 0, n, m, RAWDTW_FULL, 0u, 0};
    uint32_t end_j = 0;
    return semi_batch(ctx, SemiForm::Cost, &j, 1, a, n, cost, nullptr, &end_j);
}

int rawdtw_dtw_semiglobal_span(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m, int exclude_last, float *cost,
                               uint32_t *j0, uint32_t *end_j)
{
    if (!ctx || !a || !b || !cost || !j0 || !end_j) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n == 0 || m == 0) return fail(ctx, RAWDTW_ERR_INVALID, "zero length (dtw.cpp:670 asserts)");
    PrivateRef pr(ctx);
    int st = pr.put(b, m);
    if (st != RAWDTW_OK) return st;
    rawdtw_job_t j{0, 0, n, m, RAWDTW_FULL, exclude_last ? 1u : 0u, 0};
    return semi_batch(ctx, SemiForm::Span, &j, 1, a, n, cost, j0, end_j);
}

int rawdtw_dtw_semiglobal_tb(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m, int exclude_last, float *cost,
                             uint32_t *path_len, uint32_t *path_i, uint32_t *path_j, float *path_d)
{
    if (!ctx || !a || !b || !cost || !path_len || !path_i || !path_j || !path_d) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n == 0 || m == 0) return fail(ctx, RAWDTW_ERR_INVALID, "zero length (dtw.cpp:670 asserts)");
    PrivateRef pr(ctx);
    int st = pr.put(b, m);
    if (st != RAWDTW_OK) return st;
    rawdtw_job_t j{0, 0, n, m, RAWDTW_FULL, exclude_last ? 1u : 0u, 0};
    uint64_t off = 0;
    uint32_t j0 = 0;
    return semi_traceback(ctx, &j, 1, a, n, cost, &j0, &off, path_len, nullptr, path_i, path_j, path_d);
}

} // extern "C"
