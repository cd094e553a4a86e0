// rawdtw_band_tb.cpp -- the banded global traceback behind the C ABI: rawdtw_banded_traceback_steps, its timing and the single-call
// drop-in rawdtw_dtw_global_banded_tb (the definition of the banded path: include/rawdtw.h).  Host code only: validation, the jobs'
// launch classes, the sub-batches under "tb_workspace_mb".  The job-list planner (rawdtw_planner.cpp) keeps refusing a banded
// traceback job; these jobs are bucketed here, by band width (the fill kernel's LDS is three antidiagonals of the launch's widest
// band), longest first inside a class.  There is no CPU fallback: the kernels run or the call returns an error status.
#include "rawdtw_capi.h"
#include "rawdtw_band_tb.h"

using namespace rawdtw;
using namespace rawdtw::capi;

namespace {

// launch classes by K = slanted radius + 1: one wave a job up to one chunk of 64 slots, four waves beyond; the bounds above that only
// keep a narrow band's workgroup from reserving a wide band's LDS
constexpr uint32_t kBandTbClassK[4] = {64, 1024, 4096, (uint32_t)kMaxWaveBandK};
inline int band_tb_class(uint32_t K) { return K <= kBandTbClassK[0] ? 0 : K <= kBandTbClassK[1] ? 1 : K <= kBandTbClassK[2] ? 2 : 3; }

struct BandLaunch { int cls; uint64_t first, count; uint32_t max_k; };

// the jobs [begin, begin + cnt) in launch order; a record's aux is the job's index inside the stretch
struct BandPlan {
    std::vector<uint32_t> order; // position -> index inside the stretch
    std::vector<DevJob> jobs;
    std::vector<FullAux> aux;
    std::vector<BandLaunch> launches;
    uint64_t dir_bytes = 0;
};

void band_plan(const rawdtw_job_t *jobs, uint64_t cnt, BandPlan &pl)
{
    struct Keyed { uint64_t key; uint32_t idx; };
    std::vector<Keyed> keyed(cnt);
    const uint64_t lim = (1ull << 40) - 1;
    for (uint64_t k = 0; k < cnt; k++) {
        const rawdtw_job_t &j = jobs[k];
        const uint64_t c = (uint64_t)band_tb_class((uint32_t)slanted_radius(j.n, j.m, j.band_radius) + 1u);
        keyed[k] = Keyed{(c << 56) | (lim - std::min<uint64_t>((uint64_t)j.n + j.m, lim)), (uint32_t)k};
    }
    std::sort(keyed.begin(), keyed.end(), [](const Keyed &x, const Keyed &y) { return x.key != y.key ? x.key < y.key : x.idx < y.idx; });
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
        if (pl.launches.empty() || pl.launches.back().cls != c) pl.launches.push_back(BandLaunch{c, p, 0, 0});
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

// Sub-batches under the direction-buffer budget ("tb_workspace_mb", as rawdtw_traceback_batch*), one after another: fill, walk, finish,
// paths home, written into the caller's arrays.  Exactly one of path_step and (path_i, path_j) is given.
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

    const uint64_t budget = tb_budget_bytes(ctx);
    // the split: a job joins the current sub-batch unless that passes the budget (a job over the budget goes alone)
    struct Sub { uint64_t begin, cnt, acc; BandPlan pl; };
    std::vector<Sub> subs;
    for (uint64_t begin = 0; begin < n_jobs;) {
        uint64_t end = begin, bytes = 0;
        while (end < n_jobs) {
            const rawdtw_job_t &j = jobs[end];
            const uint64_t b = al256(band_tb_dir_bytes(j.n, j.m, slanted_radius(j.n, j.m, j.band_radius)));
            if (end > begin && bytes + b > budget) break;
            bytes += b;
            end++;
        }
        subs.push_back(Sub{begin, end - begin, 0, BandPlan{}});
        begin = end;
    }
    ctx->tb_sub_batches = subs.size();
    size_t dev_need = 0;
    uint64_t dir_need = 0, acc_max = 0, cnt_max = 0;
    std::vector<std::vector<uint64_t>> poff(subs.size());
    for (size_t q = 0; q < subs.size(); q++) {
        Sub &sb = subs[q];
        band_plan(jobs + sb.begin, sb.cnt, sb.pl);
        poff[q].resize(sb.cnt);
        for (uint64_t p = 0; p < sb.cnt; p++) { poff[q][p] = sb.acc; sb.acc += (uint64_t)sb.pl.jobs[p].n + sb.pl.jobs[p].m - 1; }
        const size_t need = al256(sb.cnt * sizeof(DevJob)) + al256(sb.cnt * sizeof(FullAux)) + 2 * al256(sb.cnt * 4) + al256(sb.cnt * 8) +
                            3 * al256(sb.acc * 4) + al256(sb.acc);
        dev_need = std::max(dev_need, need); dir_need = std::max(dir_need, sb.pl.dir_bytes);
        acc_max = std::max(acc_max, sb.acc); cnt_max = std::max(cnt_max, sb.cnt);
    }
    if ((st = ensure_tb_dir(ctx, dir_need)) != RAWDTW_OK) return st;
    DevBlock blk(ctx, "banded traceback");
    if ((st = blk.reserve(dev_need)) != RAWDTW_OK) return st;
    EventPair ev;
    for (hipEvent_t &e : ev.e) HIP_TRY(ctx, hipEventCreate(&e));
    ctx->band_tb_fill_ms = ctx->band_tb_walk_ms = 0.f; ctx->band_tb_dir_written = 0; ctx->band_tb_path_elems = 0;
    std::vector<float> h_cost(cnt_max), h_pd(acc_max);
    std::vector<uint32_t> h_len(cnt_max);
    std::vector<uint8_t> h_mv(acc_max);

    for (size_t q = 0; q < subs.size(); q++) {
        const Sub &sb = subs[q];
        char *p = blk.p;
        DevJob *d_jobs = carve<DevJob>(p, sb.cnt);
        FullAux *d_aux = carve<FullAux>(p, sb.cnt);
        float *d_cost = carve<float>(p, sb.cnt);
        uint32_t *d_plen = carve<uint32_t>(p, sb.cnt);
        uint64_t *d_poff = carve<uint64_t>(p, sb.cnt);
        uint32_t *d_ti = carve<uint32_t>(p, sb.acc);
        uint32_t *d_tj = carve<uint32_t>(p, sb.acc);
        float *d_pd = carve<float>(p, sb.acc);
        uint8_t *d_mv = carve<uint8_t>(p, sb.acc);
        HIP_TRY(ctx, hipMemcpyAsync(d_jobs, sb.pl.jobs.data(), sb.cnt * sizeof(DevJob), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_aux, sb.pl.aux.data(), sb.cnt * sizeof(FullAux), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_poff, poff[q].data(), sb.cnt * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ev.e[0], ctx->stream));
        for (const BandLaunch &L : sb.pl.launches) {
            hipError_t e = launch_band_tb_fill(d_jobs + L.first, L.count, d_aux + L.first, band_tb_threads(kBandTbClassK[L.cls]), 3 * L.max_k,
                                               ctx->d_ev, ctx->d_ref, d_cost, ctx->d_tb_dir, ctx->stream);
            if (e != hipSuccess) return hip_fail(ctx, e, "banded traceback fill launch");
        }
        HIP_TRY(ctx, hipEventRecord(ev.e[1], ctx->stream));
        hipError_t e = launch_band_tb_walk(d_jobs, sb.cnt, d_aux, ctx->d_tb_dir, d_poff, d_plen, d_ti, d_tj, ctx->stream);
        if (e == hipSuccess) e = launch_tb_finish(d_jobs, sb.cnt, ctx->d_ev, ctx->d_ref, d_poff, d_plen, d_ti, d_tj, d_mv, d_pd, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "banded traceback walk launch");
        HIP_TRY(ctx, hipEventRecord(ev.e[2], ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_cost.data(), d_cost, sb.cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_len.data(), d_plen, sb.cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_pd.data(), d_pd, sb.acc * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_mv.data(), d_mv, sb.acc, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) ctx->band_tb_fill_ms += ms;
        if (hipEventElapsedTime(&ms, ev.e[1], ev.e[2]) == hipSuccess) ctx->band_tb_walk_ms += ms;
        ctx->band_tb_dir_written += sb.pl.dir_bytes;
        for (uint64_t pp = 0; pp < sb.cnt; pp++) {
            const uint64_t k = sb.begin + sb.pl.order[pp];
            out_cost[k] = h_cost[sb.pl.order[pp]]; // (costs are indexed inside the stretch, lengths by position)
            const uint32_t len = h_len[pp];        // 0: the walk left the cell set, the job has no path
            // start-first already (k_tb_finish); the last element is popped when exclude_last is set (dtw.cpp:659-663)
            const uint32_t outlen = (jobs[k].exclude_last && len) ? len - 1 : len;
            const uint64_t src = poff[q][pp], dst = path_off[k];
            if (path_step) memcpy(path_step + dst, h_mv.data() + src, outlen);
            else {
                uint32_t i = 0, j = 0;
                for (uint32_t e2 = 0; e2 < outlen; e2++) { i += h_mv[src + e2] & 1u; j += h_mv[src + e2] >> 1; path_i[dst + e2] = i; path_j[dst + e2] = j; }
            }
            memcpy(path_d + dst, h_pd.data() + src, (size_t)outlen * 4);
            path_len[k] = outlen;
            ctx->band_tb_path_elems += outlen;
        }
    }
    return RAWDTW_OK;
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
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (fill_ms) *fill_ms = ctx->band_tb_fill_ms;
    if (walk_ms) *walk_ms = ctx->band_tb_walk_ms;
    if (direction_bytes) *direction_bytes = ctx->band_tb_dir_written;
    if (path_elements) *path_elements = ctx->band_tb_path_elems;
    return RAWDTW_OK;
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
