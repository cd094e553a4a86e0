// rawdtw_band_tb.cpp -- the banded global traceback behind the C ABI: rawdtw_banded_traceback_steps, its timing and the single-call
// drop-in rawdtw_dtw_global_banded_tb (the definition of the banded path: include/rawdtw.h).  Host code only: validation, the jobs'
// launch classes; the sub-batches under "tb_workspace_mb" are the driver's (rawdtw_tb_driver.cpp).  The job-list planner (rawdtw_planner.cpp) keeps refusing a banded
// traceback job; these jobs are bucketed here, by band width (the fill kernel's LDS is three antidiagonals of the launch's widest
// band), longest first inside a class.  There is no CPU fallback: the kernels run or the call returns an error status.
#include "rawdtw_capi.h"
#include "rawdtw_band_tb.h"
#include "rawdtw_tb_driver.h"

using namespace rawdtw;
using namespace rawdtw::capi;

namespace {

// launch classes by K = slanted radius + 1: one wave a job up to one chunk of 64 slots, four waves beyond; the bounds above that only
// keep a narrow band's workgroup from reserving a wide band's LDS
constexpr uint32_t kBandTbClassK[4] = {64, 1024, 4096, (uint32_t)kMaxWaveBandK};
inline int band_tb_class(uint32_t K) { return K <= kBandTbClassK[0] ? 0 : K <= kBandTbClassK[1] ? 1 : K <= kBandTbClassK[2] ? 2 : 3; }

void band_plan(const rawdtw_job_t *jobs, uint64_t cnt, ClassPlan &pl)
{
    std::vector<Keyed> keyed(cnt);
    const uint64_t lim = (1ull << 40) - 1;
    for (uint64_t k = 0; k < cnt; k++) {
        const rawdtw_job_t &j = jobs[k];
        const uint64_t c = (uint64_t)band_tb_class((uint32_t)slanted_radius(j.n, j.m, j.band_radius) + 1u);
        keyed[k] = Keyed{(c << 56) | (lim - std::min<uint64_t>((uint64_t)j.n + j.m, lim)), (uint32_t)k};
    }
    sort_keyed(keyed);
    pl.order.resize(cnt); pl.jobs.resize(cnt); pl.aux.assign(cnt, FullAux{0, 0});
    for (uint64_t p = 0; p < cnt; p++) {
        const uint32_t k = keyed[p].idx;
        const rawdtw_job_t &j = jobs[k];
        const int c = (int)(keyed[p].key >> 56);
        pl.order[p] = k;
        DevJob &d = pl.jobs[p];
        d.ref_off = j.ref_off; d.read_off = j.read_off; d.n = j.n; d.m = j.m; d.R = slanted_radius(j.n, j.m, j.band_radius);
        d.flags = j.exclude_last ? kFlagExcludeLast : 0u; d.aux = k;
        pl.aux[p].dir_off = pl.dir_bytes;
        pl.dir_bytes += al256(band_tb_dir_bytes(j.n, j.m, d.R));
        if (pl.launches.empty() || pl.launches.back().cls != c) pl.launches.push_back(ClassLaunch{c, p, 0, 0});
        pl.launches.back().count++;
        pl.launches.back().max_k = std::max(pl.launches.back().max_k, (uint32_t)d.R + 1u);
    }
}

// Every refusal, before anything is enqueued
int band_check(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, bool arena, uint64_t n_events)
{
    if (arena && !ctx->d_ev) return fail(ctx, RAWDTW_ERR_INVALID, "the context has no event arena");
    if (!ctx->d_ref) return fail(ctx, RAWDTW_ERR_INVALID, "the context has no reference arena");
    const uint64_t n_ev = arena ? ctx->n_ev : n_events;
    for (uint64_t k = 0; k < n_jobs; k++) {
        const rawdtw_job_t &j = jobs[k];
        if (j.n == 0 || j.m == 0 || j.n >= 0x7fffffffu || j.m >= 0x7fffffffu || j.band_radius < 0)
            return fail(ctx, RAWDTW_ERR_INVALID, "job " + std::to_string(k) + ": zero length or negative band radius (dtw.cpp:274-277 asserts; "
                                                 "a full-matrix job goes to rawdtw_traceback_batch*)");
        if ((uint64_t)j.read_off + j.n > n_ev || j.ref_off > ctx->n_ref || j.ref_off + j.m > ctx->n_ref)
            return fail(ctx, RAWDTW_ERR_RANGE, "job " + std::to_string(k) + ": window outside the arenas");
        const int R = slanted_radius(j.n, j.m, j.band_radius);
        if (R < 0 || R + 1 > kMaxWaveBandK) return fail(ctx, RAWDTW_ERR_UNSUPPORTED, "band radius too large for the LDS-resident band kernel");
    }
    return RAWDTW_OK;
}

// The banded path as the driver takes it (rawdtw_tb_driver.h): a stretch's records (job, aux, cost) lie in the slot (the driver sends them), the walk is one launch
// over the stretch and k_tb_finish behind it.  A job whose walk left the cell set comes home with length 0: it has no path.
uint64_t band_job_dir_bytes(const rawdtw_ctx *, const rawdtw_job_t &j) { return al256(band_tb_dir_bytes(j.n, j.m, slanted_radius(j.n, j.m, j.band_radius))); }
int band_stretch(rawdtw_ctx *, const rawdtw_job_t *jobs, uint64_t cnt, TbStretch *out)
{
    ClassPlan *pl = new ClassPlan;
    band_plan(jobs, cnt, *pl);
    *out = class_stretch(pl, false);
    return RAWDTW_OK;
}
int band_fill(rawdtw_ctx *ctx, const TbStretch &s, const TbSlot &slot)
{
    const ClassPlan &pl = *static_cast<const ClassPlan *>(s.plan);
    for (const ClassLaunch &L : pl.launches) {
        hipError_t e = launch_band_tb_fill(slot.jobs + L.first, L.count, slot.aux + L.first, band_tb_threads(kBandTbClassK[L.cls]), 3 * L.max_k,
                                           ctx->d_ev, ctx->d_ref, slot.cost, ctx->d_tb_dir, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "banded traceback fill launch");
    }
    return RAWDTW_OK;
}
int band_walk(rawdtw_ctx *ctx, const TbStretch &s, const TbSlot &slot)
{
    const uint64_t cnt = static_cast<const ClassPlan *>(s.plan)->jobs.size();
    hipError_t e = launch_band_tb_walk(slot.jobs, cnt, slot.aux, ctx->d_tb_dir, slot.poff, slot.plen, slot.ti, slot.tj, ctx->stream);
    if (e == hipSuccess) e = launch_tb_finish(slot.jobs, cnt, ctx->d_ev, ctx->d_ref, slot.poff, slot.plen, slot.ti, slot.tj, slot.mv, slot.pd, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "banded traceback walk launch");
    return RAWDTW_OK;
}

// Exactly one of path_step and (path_i, path_j) is given.
int band_traceback(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events, uint64_t n_events, float *out_cost,
                   const uint64_t *path_off, uint32_t *path_len, uint8_t *path_step, uint32_t *path_i, uint32_t *path_j, float *path_d)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (n_jobs == 0) return RAWDTW_OK;
    if (!jobs || !out_cost || !path_off || !path_len || !path_d || (!path_step && (!path_i || !path_j)))
        return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n_jobs >= 0x7fffffffull) return fail(ctx, RAWDTW_ERR_INVALID, "too many jobs for one call");
    const bool arena = h_events == nullptr;
    int st = band_check(ctx, jobs, n_jobs, arena, n_events);
    if (st != RAWDTW_OK) return st;
    if (!arena && (st = rawdtw_upload_events(ctx, h_events, n_events)) != RAWDTW_OK) return st;
    static const TbPath banded{&rawdtw_ctx::band_tb, false, false, "banded traceback workspace allocation failed", band_job_dir_bytes, band_stretch, band_fill,
                               band_walk, class_release};
    return tb_run(ctx, banded, jobs, n_jobs, TbOut{out_cost, nullptr, path_off, path_len, path_step, path_i, path_j, path_d}, nullptr);
}

} // namespace

extern "C" {

int rawdtw_banded_traceback_steps(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events, uint64_t n_events,
                                  float *out_cost, const uint64_t *path_off, uint32_t *path_len, uint8_t *path_step, float *path_d)
{
    if (ctx && n_jobs && !path_step) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    return band_traceback(ctx, jobs, n_jobs, h_events, n_events, out_cost, path_off, path_len, path_step, nullptr, nullptr, path_d);
}

int rawdtw_banded_traceback_timing(const rawdtw_ctx *ctx, float *fill_ms, float *walk_ms, uint64_t *direction_bytes, uint64_t *path_elements)
{
    return tb_timing_get(ctx, &rawdtw_ctx::band_tb, fill_ms, walk_ms, direction_bytes, path_elements);
}

int rawdtw_dtw_global_banded_tb(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m, int band_radius, int exclude_last,
                                float *cost, uint32_t *path_len, uint32_t *path_i, uint32_t *path_j, float *path_d)
{
    if (!ctx || !a || !b || !cost || !path_len || !path_i || !path_j || !path_d) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n == 0 || m == 0 || band_radius < 0) return fail(ctx, RAWDTW_ERR_INVALID, "zero length or negative band radius (dtw.cpp:274-277 asserts)");
    PrivateRef pr(ctx);
    int st = pr.put(b, m);
    if (st != RAWDTW_OK) return st;
    rawdtw_job_t j{0, 0, n, m, band_radius, exclude_last ? 1u : 0u, 0};
    uint64_t off = 0;
    return band_traceback(ctx, &j, 1, a, n, cost, &off, path_len, nullptr, path_i, path_j, path_d);
}

} // extern "C"
