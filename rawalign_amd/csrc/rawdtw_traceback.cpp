// rawdtw_traceback.cpp -- DTW_global_tb for batches (rawdtw_traceback_batch*: dtw.hpp:28 at rmap.cpp:221,284) and the
// single-call drop-ins with the reference's own signatures (dtw.hpp:21,25,28).  Host code only.
#include "rawdtw_capi.h"
#include "rawdtw_tb_driver.h"

using namespace rawdtw;
using namespace rawdtw::capi;

extern "C" {

// The full-matrix path as the driver takes it (rawdtw_tb_driver.h): a stretch is a rawdtw_plan of the job-list planner, which owns its
// records and costs; the walk is one wave per job over the direction buffer, then start-first order, steps and distances (k_tb_finish).
static uint64_t full_job_dir_bytes(const rawdtw_ctx *, const rawdtw_job_t &j) { return dir_bytes_for(j.n, j.m, full_rpl(std::min(j.n, j.m))) + 256; }
static int full_plan(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t cnt, TbStretch *out)
{
    rawdtw_plan *pl = nullptr;
    if (int st = build_plan(ctx, jobs, cnt, true, &pl)) return st;
    *out = TbStretch{pl, pl->order.data(), pl->h_jobs.data(), pl->dir_bytes, tb::Recs{}, pl->d_cost};
    return RAWDTW_OK;
}
static int full_fill(rawdtw_ctx *ctx, const TbStretch &s, const TbSlot &)
{
    rawdtw_plan *pl = static_cast<rawdtw_plan *>(s.plan);
    pl->d_dir = ctx->d_tb_dir; // (the context's direction workspace may have grown while the later stretches were planned)
    return rawdtw_plan_run(ctx, pl);
}
static int full_walk(rawdtw_ctx *ctx, const TbStretch &s, const TbSlot &slot)
{
    const rawdtw_plan *pl = static_cast<const rawdtw_plan *>(s.plan);
    for (const Launch &L : pl->launches) {
        hipError_t e = launch_tb_walk_wave(pl->d_jobs + L.first, L.count, pl->d_aux + L.first, wave_class_of(L.param), ctx->d_ev, ctx->d_ref, pl->d_dir,
                                           slot.poff + L.first, slot.plen + L.first, slot.ti, slot.tj, slot.mv, slot.pd, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "traceback walk launch");
    }
    return RAWDTW_OK;
}
static void full_release(void *plan) { rawdtw_plan_destroy(static_cast<rawdtw_plan *>(plan)); }

// The entries' common prologue.  `arena`: the jobs' read_off index the context's event arena as it lies (rawdtw_traceback_arena_steps) --
// nothing is uploaded and h_events / n_events are not looked at; else the arena is replaced by h_events first.  That is the one
// difference.  `tx`: the text form (rawdtw_traceback_batch_text / _arena_text).
static int traceback_core(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, bool arena, const float *h_events,
                          uint64_t n_events, float *out_cost, const uint64_t *path_off, uint32_t *path_len,
                          uint32_t *path_i, uint32_t *path_j, uint8_t *path_step, float *path_d, const TbText *tx = nullptr)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (tx) {
        if (!tx->text_off || !tx->bytes || (n_jobs && (!jobs || !out_cost || !path_len || !tx->recs))) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
        for (uint64_t k = 0; k < n_jobs; k++)
            if (tx->recs[k].mode > 1) return fail(ctx, RAWDTW_ERR_INVALID, "a rec's mode is neither 0 nor 1");
    } else if (n_jobs && (!jobs || !out_cost || !path_off || !path_len || !path_d || (!path_step && (!path_i || !path_j))))
        return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (arena) { // (before anything is enqueued)
        if (!ctx->d_ev) return fail(ctx, RAWDTW_ERR_INVALID, "the context has no event arena");
        for (uint64_t k = 0; k < n_jobs; k++)
            if ((uint64_t)jobs[k].read_off + jobs[k].n > ctx->n_ev) return fail(ctx, RAWDTW_ERR_INVALID, "a traceback job reads beyond the event arena");
    }
    int st = arena ? RAWDTW_OK : rawdtw_upload_events(ctx, h_events, n_events);
    if (st != RAWDTW_OK) return st;
    if (tx) { ctx->aln_count_ms = ctx->aln_write_ms = 0.f; ctx->aln_text_bytes = 0; }
    ctx->tb = TbTiming{};
    ctx->tb_sub_batches = 0;
    for (uint64_t k = 0; k < n_jobs; k++)
        if (jobs[k].n == 0 || jobs[k].m == 0) return fail(ctx, RAWDTW_ERR_INVALID, "zero-length traceback job");
    static const TbPath full{&rawdtw_ctx::tb, true, false, "path buffer allocation failed", full_job_dir_bytes, full_plan, full_fill, full_walk, full_release};
    return tb_run(ctx, full, jobs, n_jobs, TbOut{out_cost, nullptr, path_off, path_len, path_step, path_i, path_j, path_d}, tx);
}

int rawdtw_traceback_batch(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events,
                           uint64_t n_events, float *out_cost, const uint64_t *path_off, uint32_t *path_len,
                           uint32_t *path_i, uint32_t *path_j, float *path_d)
{
    if (n_jobs && (!path_i || !path_j)) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    return traceback_core(ctx, jobs, n_jobs, false, h_events, n_events, out_cost, path_off, path_len, path_i, path_j, nullptr, path_d);
}

int rawdtw_traceback_batch_steps(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events,
                                 uint64_t n_events, float *out_cost, const uint64_t *path_off, uint32_t *path_len,
                                 uint8_t *path_step, float *path_d)
{
    if (n_jobs && !path_step) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    return traceback_core(ctx, jobs, n_jobs, false, h_events, n_events, out_cost, path_off, path_len, nullptr, nullptr, path_step, path_d);
}

int rawdtw_traceback_arena_steps(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, float *out_cost, const uint64_t *path_off,
                                 uint32_t *path_len, uint8_t *path_step, float *path_d)
{
    if (n_jobs && !path_step) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    return traceback_core(ctx, jobs, n_jobs, true, nullptr, 0, out_cost, path_off, path_len, nullptr, nullptr, path_step, path_d);
}

int rawdtw_traceback_batch_text(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const float *h_events, uint64_t n_events,
                                const rawdtw_aln_rec_t *recs, float *out_cost, uint32_t *path_len, uint64_t *text_off, char *text, uint64_t text_cap,
                                uint64_t *text_bytes)
{
    const TbText tx{recs, text_off, text, text_cap, text_bytes};
    return traceback_core(ctx, jobs, n_jobs, false, h_events, n_events, out_cost, nullptr, path_len, nullptr, nullptr, nullptr, nullptr, &tx);
}

int rawdtw_traceback_arena_text(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, const rawdtw_aln_rec_t *recs, float *out_cost,
                                uint32_t *path_len, uint64_t *text_off, char *text, uint64_t text_cap, uint64_t *text_bytes)
{
    const TbText tx{recs, text_off, text, text_cap, text_bytes};
    return traceback_core(ctx, jobs, n_jobs, true, nullptr, 0, out_cost, nullptr, path_len, nullptr, nullptr, nullptr, nullptr, &tx);
}

// ---- single-call drop-ins ----------------------------------------------------------------------
static int single_call(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m, int radius,
                       int excl, float *cost)
{
    if (!ctx || !a || !b || !cost) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n == 0 || m == 0 || radius < RAWDTW_FULL) return fail(ctx, RAWDTW_ERR_INVALID, "zero length or negative radius");
    PrivateRef pr(ctx);
    int st = pr.put(b, m);
    if (st != RAWDTW_OK) return st;
    rawdtw_job_t j{0, 0, n, m, radius, excl ? 1u : 0u, 0};
    return rawdtw_score_batch(ctx, &j, 1, a, n, cost);
}

int rawdtw_dtw_global(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m, int exclude_last,
                      float *cost)
{
    return single_call(ctx, a, n, b, m, RAWDTW_FULL, exclude_last, cost);
}

int rawdtw_dtw_global_slantedbanded_antidiagonalwise(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b,
                                                     uint32_t m, int band_radius, int exclude_last, float *cost)
{
    if (band_radius < 0) return fail(ctx, RAWDTW_ERR_INVALID, "negative band radius (dtw.cpp:277 asserts)");
    return single_call(ctx, a, n, b, m, band_radius, exclude_last, cost);
}

int rawdtw_dtw_global_tb(rawdtw_ctx *ctx, const float *a, uint32_t n, const float *b, uint32_t m, int exclude_last,
                         float *cost, uint32_t *path_len, uint32_t *path_i, uint32_t *path_j, float *path_d)
{
    if (!ctx || !a || !b || !cost || !path_len || !path_i || !path_j || !path_d)
        return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n == 0 || m == 0) return fail(ctx, RAWDTW_ERR_INVALID, "zero length (dtw.cpp:596 asserts)");
    PrivateRef pr(ctx);
    int st = pr.put(b, m);
    if (st != RAWDTW_OK) return st;
    rawdtw_job_t j{0, 0, n, m, RAWDTW_FULL, exclude_last ? 1u : 0u, 0};
    uint64_t off = 0;
    return rawdtw_traceback_batch(ctx, &j, 1, a, n, cost, &off, path_len, path_i, path_j, path_d);
}

int rawdtw_traceback_timing(const rawdtw_ctx *ctx, float *fill_ms, float *walk_ms, uint64_t *direction_bytes, uint64_t *path_elements)
{
    return tb_timing_get(ctx, &rawdtw_ctx::tb, fill_ms, walk_ms, direction_bytes, path_elements);
}

} // extern "C"
