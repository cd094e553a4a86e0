// rawdtw_tb_driver.cpp -- the traceback driver (rawdtw_tb_driver.h).  Host code only.
//
// What leaves the device per path element is its distance and ONE byte, the step from the element before it (k_tb_finish):
// 5 bytes over the bus instead of 12.  The steps form hands exactly that to the caller (the mapper's aln:s: writer walks the steps
// while it formats); the (i, j) form rebuilds (i, j) from the steps while it writes the caller's three arrays.  Sub-batches (only a
// batch whose direction buffers exceed the budget has several) run as a two-deep pipeline: sub-batch k's paths come home on a second
// stream and are written out by a few host threads while sub-batch k + 1 fills and walks.  (Cutting a batch that fits into quarters
// to hide the download behind the kernels was tried and cost more than it hid: a fill or walk launch takes as long as its longest job
// -- fill 9.0 -> 18.8 ms, walk 1.9 -> 7.4 ms for 8 080 paths in five launches each.)
// The text form (`tx`; include/rawdtw.h, "aln text"): steps and distances stay on the device.  Behind a sub-batch's walk go k_aln_count,
// k_aln_scan and k_aln_write (rawdtw_aln_text.hip), the text into a block sized by rawdtw_aln_text_bound -- so the write needs no word
// from the host --, and what comes home with the costs and lengths is 8 bytes a job of text offsets.  The text itself is copied once
// those have landed and say how long it is, straight to its final place, on a stream of its own beside the next sub-batch's fill.
// Sub-batches hold whole jobs in job order, so a sub-batch's text is one stretch behind the one before it.
#include <numeric>

#include "rawdtw_tb_driver.h"
#include "rawdtw_aln_text.h"

namespace rawdtw {
namespace capi {

namespace {

struct Sub {
    TbStretch s;
    uint64_t begin = 0, cnt = 0, acc = 0;
    std::vector<uint64_t> poff;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // fill start, fill end, walk end, download end; text form: count + scan end, write end
    std::vector<AlnDevRec> hrec; // text form: the paths' records, plan order; where the slot's text block keeps the offsets and the text
    uint64_t text_bound = 0;
    uint64_t *d_toff = nullptr; char *d_text = nullptr;
    int slot = 0;
    bool in_flight = false;
    bool dense = false;   // the path allows it, steps form, and the caller's offsets of these jobs are one dense ascending stretch: the device
    uint64_t lo = 0;      // writes the paths in the CALLER's layout (from element lo on) and they come home as two copies, into the caller's
    bool direct = false;  // arrays when those are page-locked (rawdtw_host_alloc), else through the landing zone and one memcpy a thread
};

bool page_locked(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}

// a grow-only block of the context, two slots of `need` bytes, device or page-locked; contents are not kept
bool grow(void *&p, size_t &bytes, size_t need, bool pinned)
{
    if (bytes >= 2 * need) return true;
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr; bytes = 0;
    const size_t want = tb::block_bytes(need);
    if ((pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want)) != hipSuccess) { p = nullptr; (void)hipGetLastError(); return false; }
    bytes = want;
    return true;
}

template <typename T> T *at(void *block, size_t slot_off, const tb::Region &r) { return reinterpret_cast<T *>(static_cast<char *>(block) + slot_off + r.at); }

// a finished sub-batch out of its landing zone `hp` into the caller's arrays (pageable memory: spread over a few threads); (i, j) from the
// steps.  -> the path elements written
uint64_t copy_out(const rawdtw_ctx *ctx, const TbPath &path, const rawdtw_job_t *jobs, const Sub &sb, const char *hp, const TbOut &out, bool text)
{
    const tb::Landing H = tb::landing(sb.cnt, sb.acc, path.extra, text);
    const float *h_pd = reinterpret_cast<const float *>(hp + H.pd.at);
    const uint8_t *h_mv = reinterpret_cast<const uint8_t *>(hp + H.mv.at);
    const float *h_cost = reinterpret_cast<const float *>(hp + H.cost.at);
    const uint32_t *h_plen = reinterpret_cast<const uint32_t *>(hp + H.plen.at);
    const uint32_t *h_extra = path.extra ? reinterpret_cast<const uint32_t *>(hp + H.extra.at) : nullptr;
    int T = ctx->plan_threads > 0 ? ctx->plan_threads : (int)std::min<uint64_t>(std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 8u), sb.acc / (1u << 20) + 1);
    T = std::max(1, std::min(T, 16));
    std::vector<uint64_t> elems(T, 0);
    parallel_for(T, [&](int t) {
        for (uint64_t p = sb.cnt * (uint64_t)t / T; p < sb.cnt * (uint64_t)(t + 1) / T; p++) {
            const uint64_t k = sb.begin + sb.s.order[p];
            out.cost[k] = h_cost[sb.s.order[p]]; // (costs are indexed inside the stretch, lengths and the extra word by position)
            if (h_extra) out.extra[k] = h_extra[p];
            const uint32_t len = h_plen[p]; // 0: the job has no path (a banded walk that left the cell set)
            // device paths are start-first already (k_tb_finish, dtw.cpp:656-657); the reference pops the last element when
            // exclude_last_element is set (dtw.cpp:659-663, 744-748)
            const uint32_t outlen = (jobs[k].exclude_last && len) ? len - 1 : len;
            out.len[k] = outlen;
            elems[t] += outlen;
            if (sb.dense || text) continue; // (the stretch is copied whole below, or came home in place; the text form's paths stay on the device)
            const uint64_t src = sb.poff[p], dst = out.off[k];
            const uint8_t *mv = h_mv + src;
            if (out.step) memcpy(out.step + dst, mv, outlen);
            else {
                uint32_t i = 0, j = h_extra ? h_extra[p] : 0;
                uint32_t *pi = out.i + dst, *pj = out.j + dst;
                for (uint32_t q = 0; q < outlen; q++) { i += mv[q] & 1u; j += mv[q] >> 1; pi[q] = i; pj[q] = j; }
            }
            memcpy(out.d + dst, h_pd + src, (size_t)outlen * 4);
        }
        if (sb.dense && !sb.direct) { // this thread's share of the stretch
            const uint64_t a0 = sb.acc * (uint64_t)t / T, a1 = sb.acc * (uint64_t)(t + 1) / T;
            memcpy(out.step + sb.lo + a0, h_mv + a0, a1 - a0);
            memcpy(out.d + sb.lo + a0, h_pd + a0, (a1 - a0) * 4);
        }
    });
    return std::accumulate(elems.begin(), elems.end(), (uint64_t)0);
}

} // namespace

int tb_run(rawdtw_ctx *ctx, const TbPath &path, const rawdtw_job_t *jobs, uint64_t n_jobs, const TbOut &out, const TbText *tx)
{
    static const bool timing = getenv("RAWDTW_PLAN_TIMING") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!timing) return;
        auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[traceback] %-14s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count());
        t_prev = t;
    };
    if (!ctx->tb_copy) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->tb_copy, hipStreamNonBlocking));
    if (tx && !ctx->tb_text) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->tb_text, hipStreamNonBlocking));
    TbTiming &tm = ctx->*path.timing;

    std::vector<Sub> subs;
    struct Guard { // plans and events go when the call ends (a plan's hipFree waits for the device: not in the middle of the pipeline)
        std::vector<Sub> &v; rawdtw_ctx *c; const TbPath &path;
        ~Guard()
        {
            (void)hipStreamSynchronize(c->stream);
            if (c->tb_copy) (void)hipStreamSynchronize(c->tb_copy);
            if (c->tb_text) (void)hipStreamSynchronize(c->tb_text);
            for (Sub &sb : v) { if (sb.s.plan) path.release(sb.s.plan); for (hipEvent_t &e : sb.ev) if (e) (void)hipEventDestroy(e); }
        }
    } guard{subs, ctx, path};
    {
        std::vector<uint64_t> job_bytes(n_jobs);
        for (uint64_t k = 0; k < n_jobs; k++) job_bytes[k] = path.job_dir_bytes(ctx, jobs[k]);
        const std::vector<tb::Cut> cuts = tb::split(job_bytes.data(), n_jobs, tb_budget_bytes(ctx));
        subs.resize(cuts.size());
        for (size_t q = 0; q < cuts.size(); q++) { subs[q].begin = cuts[q].begin; subs[q].cnt = cuts[q].cnt; subs[q].slot = (int)(q & 1); }
    }
    ctx->tb_sub_batches = subs.size();
    // ---- all sub-batches planned first (host planner, device allocations, job records' upload: while nothing is in flight) ----
    const bool caller_pinned = path.dense && out.step && n_jobs && page_locked(out.step) && page_locked(out.d);
    size_t dn = 0, hn = 0, tn = 0, dir_need = 0;
    for (Sub &sb : subs) {
        const uint64_t begin = sb.begin, end = sb.begin + sb.cnt;
        if (int st = path.plan(ctx, jobs + begin, sb.cnt, &sb.s)) return st;
        for (int q = 0; q < (tx ? 6 : 4); q++) HIP_TRY(ctx, hipEventCreate(&sb.ev[q]));
        sb.poff.resize(sb.cnt);
        uint64_t acc = 0;
        sb.dense = path.dense && out.step != nullptr;
        for (uint64_t k = begin; sb.dense && k + 1 < end; k++) sb.dense = out.off[k + 1] == out.off[k] + jobs[k].n + jobs[k].m - 1;
        if (sb.dense) {
            sb.lo = out.off[begin];
            for (uint64_t p = 0; p < sb.cnt; p++) sb.poff[p] = out.off[begin + sb.s.order[p]] - sb.lo;
            acc = out.off[end - 1] + jobs[end - 1].n + jobs[end - 1].m - 1 - sb.lo;
            sb.direct = caller_pinned;
        } else
            for (uint64_t p = 0; p < sb.cnt; p++) { sb.poff[p] = acc; acc += (uint64_t)sb.s.jobs[p].n + sb.s.jobs[p].m - 1; }
        sb.acc = acc;
        dn = std::max(dn, tb::paths(sb.cnt, acc, path.extra, sb.s.recs.need).need);
        hn = std::max(hn, tb::landing(sb.cnt, acc, path.extra, tx != nullptr).need);
        dir_need = std::max(dir_need, sb.s.dir_bytes);
        if (tx) {
            sb.hrec.resize(sb.cnt);
            for (uint64_t p = 0; p < sb.cnt; p++) {
                const uint64_t k = begin + sb.s.order[p];
                sb.hrec[p] = aln_dev_rec(tx->recs[k], jobs[k].exclude_last != 0, sb.s.order[p]);
            }
            sb.text_bound = rawdtw_aln_text_bound(jobs + begin, tx->recs + begin, sb.cnt);
            tn = std::max(tn, tb::text(sb.cnt, sb.text_bound).need);
        }
    }
    // The context's grow-only blocks.  Path buffers, the path's own records, the landing zone and the text block have two slots each.  The
    // direction workspace stays single: fill and walk of consecutive sub-batches are ordered on ctx->stream, and only the download (which
    // reads a slot's path buffers, never the directions) runs beside them.
    if (int st = ensure_tb_dir(ctx, dir_need)) return st;
    if (!grow(ctx->d_tb_paths, ctx->tb_paths_bytes, dn, false)) return fail(ctx, RAWDTW_ERR_OOM, path.oom);
    if (!grow(ctx->d_tb_text, ctx->tb_text_bytes, tn, false)) return fail(ctx, RAWDTW_ERR_OOM, "text buffer allocation failed");
    if (!grow(ctx->h_pinned, ctx->pinned_bytes, hn, true)) return fail(ctx, RAWDTW_ERR_OOM, "pinned host allocation failed");
    tm = TbTiming{};
    lap("plans + alloc");

    uint64_t text_base = 0;  // text form: the bytes of the sub-batches finished so far
    bool text_short = false; // ... and one of them did not fit text_cap: sizes are still filled, no more text is copied
    // the second half of a sub-batch: wait for its download, write the caller's arrays
    auto finish = [&](Sub &sb) -> int {
        if (!sb.in_flight) return RAWDTW_OK;
        sb.in_flight = false;
        hipError_t e = hipEventSynchronize(sb.ev[3]);
        if (e != hipSuccess) return hip_fail(ctx, e, "traceback download");
        lap("wait download");
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, sb.ev[0], sb.ev[1]) == hipSuccess) tm.fill_ms += ms;
        if (hipEventElapsedTime(&ms, sb.ev[1], sb.ev[2]) == hipSuccess) tm.walk_ms += ms;
        tm.dir_written += sb.s.dir_bytes;
        const char *hp = static_cast<const char *>(ctx->h_pinned) + tb::slot_at(ctx->pinned_bytes, sb.slot);
        tm.path_elems += copy_out(ctx, path, jobs, sb, hp, out, tx != nullptr);
        lap("copy out");
        if (tx) {
            const uint64_t *h_toff = reinterpret_cast<const uint64_t *>(hp + tb::landing(sb.cnt, sb.acc, path.extra, true).toff.at);
            const uint64_t total = h_toff[sb.cnt];
            for (uint64_t q = 0; q <= sb.cnt; q++) tx->text_off[sb.begin + q] = text_base + h_toff[q];
            if (total > sb.text_bound) return fail(ctx, RAWDTW_ERR_INTERNAL, "a sub-batch's text is longer than its bound");
            if (text_base + total > tx->cap) text_short = true;
            if (tx->text && total && !text_short) {
                e = hipMemcpyAsync(tx->text + text_base, sb.d_text, total, hipMemcpyDeviceToHost, ctx->tb_text);
                if (e == hipSuccess) e = hipStreamSynchronize(ctx->tb_text);
                if (e != hipSuccess) return hip_fail(ctx, e, "text download");
            }
            text_base += total;
            if (hipEventElapsedTime(&ms, sb.ev[2], sb.ev[4]) == hipSuccess) ctx->aln_count_ms += ms;
            if (hipEventElapsedTime(&ms, sb.ev[4], sb.ev[5]) == hipSuccess) ctx->aln_write_ms += ms;
            lap("text home");
        }
        return RAWDTW_OK;
    };

    for (size_t k = 0; k < subs.size(); k++) {
        Sub &sb = subs[k];
        if (k >= 2) { if (int st = finish(subs[k - 2])) return st; } // (its slot's buffers are this sub-batch's now)
        const tb::Paths P = tb::paths(sb.cnt, sb.acc, path.extra, sb.s.recs.need);
        const size_t pb = tb::slot_at(ctx->tb_paths_bytes, sb.slot);
        char *rb = at<char>(ctx->d_tb_paths, pb, P.recs);
        const tb::Recs &R = sb.s.recs;
        const TbSlot slot{at<DevJob>(rb, 0, R.jobs), at<FullAux>(rb, 0, R.aux), at<float>(rb, 0, R.cost), at<uint32_t>(rb, 0, R.endj), at<float>(rb, 0, R.bnd),
                          at<uint64_t>(ctx->d_tb_paths, pb, P.poff), at<uint32_t>(ctx->d_tb_paths, pb, P.plen), at<uint32_t>(ctx->d_tb_paths, pb, P.extra),
                          at<uint32_t>(ctx->d_tb_paths, pb, P.ti), at<uint32_t>(ctx->d_tb_paths, pb, P.tj), at<float>(ctx->d_tb_paths, pb, P.pd),
                          at<uint8_t>(ctx->d_tb_paths, pb, P.mv)};
        hipError_t e = hipMemcpyAsync(slot.poff, sb.poff.data(), sb.cnt * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && sb.s.aux) e = hipMemcpyAsync(slot.jobs, sb.s.jobs, sb.cnt * sizeof(DevJob), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && sb.s.aux) e = hipMemcpyAsync(slot.aux, sb.s.aux, sb.cnt * sizeof(FullAux), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "path offsets upload");
        AlnDevRec *d_rec = nullptr; uint64_t *d_tot = nullptr;
        if (tx) {
            const tb::Text X = tb::text(sb.cnt, sb.text_bound);
            const size_t xb = tb::slot_at(ctx->tb_text_bytes, sb.slot);
            d_rec = at<AlnDevRec>(ctx->d_tb_text, xb, X.rec); d_tot = at<uint64_t>(ctx->d_tb_text, xb, X.tot);
            sb.d_toff = at<uint64_t>(ctx->d_tb_text, xb, X.toff); sb.d_text = at<char>(ctx->d_tb_text, xb, X.text);
            e = hipMemcpyAsync(d_rec, sb.hrec.data(), sb.cnt * sizeof(AlnDevRec), hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) return hip_fail(ctx, e, "text records upload");
        }
        (void)hipEventRecord(sb.ev[0], ctx->stream);
        if (int st = path.fill(ctx, sb.s, slot)) return st;
        (void)hipEventRecord(sb.ev[1], ctx->stream);
        if (int st = path.walk(ctx, sb.s, slot)) return st;
        (void)hipEventRecord(sb.ev[2], ctx->stream);
        if (tx) { // measure, scan, write: all behind the walk, none of them waits for the host
            e = launch_aln_count(slot.mv, slot.pd, slot.poff, slot.plen, d_rec, sb.cnt, d_tot, ctx->stream);
            if (e == hipSuccess) e = launch_aln_scan(d_tot, sb.cnt, sb.d_toff, ctx->stream);
            if (e == hipSuccess) e = hipEventRecord(sb.ev[4], ctx->stream);
            if (e == hipSuccess) e = launch_aln_write(slot.mv, slot.pd, slot.poff, slot.plen, d_rec, sb.cnt, sb.d_toff, sb.d_text, ctx->stream);
            if (e == hipSuccess) e = hipEventRecord(sb.ev[5], ctx->stream);
            if (e != hipSuccess) return hip_fail(ctx, e, "aln text launch");
        }
        // the download: on the second stream, behind the walk; everything lands in pinned memory (a download into pageable
        // memory makes the call wait for the kernels in front of it)
        const tb::Landing H = tb::landing(sb.cnt, sb.acc, path.extra, tx != nullptr);
        char *hp = static_cast<char *>(ctx->h_pinned) + tb::slot_at(ctx->pinned_bytes, sb.slot);
        auto home = [&](void *dst, const void *src, size_t bytes) {
            if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->tb_copy);
        };
        e = hipStreamWaitEvent(ctx->tb_copy, sb.ev[tx ? 5 : 2], 0);
        home(hp + H.cost.at, sb.s.d_cost ? sb.s.d_cost : slot.cost, sb.cnt * 4);
        home(hp + H.plen.at, slot.plen, sb.cnt * 4);
        if (path.extra) home(hp + H.extra.at, slot.extra, sb.cnt * 4);
        if (tx) home(hp + H.toff.at, sb.d_toff, (sb.cnt + 1) * 8);
        else {
            home(sb.direct ? static_cast<void *>(out.d + sb.lo) : static_cast<void *>(hp + H.pd.at), slot.pd, sb.acc * 4);
            home(sb.direct ? static_cast<void *>(out.step + sb.lo) : static_cast<void *>(hp + H.mv.at), slot.mv, sb.acc);
        }
        if (e == hipSuccess) e = hipEventRecord(sb.ev[3], ctx->tb_copy);
        if (e != hipSuccess) return hip_fail(ctx, e, "traceback download");
        sb.in_flight = true;
        lap("enqueue");
        // ... and while all that runs: the sub-batch before this one
        if (k >= 1) { if (int st = finish(subs[k - 1])) return st; }
    }
    for (size_t k = subs.size() >= 2 ? subs.size() - 2 : 0; k < subs.size(); k++) { if (int st = finish(subs[k])) return st; }
    if (tx) {
        if (n_jobs == 0) tx->text_off[0] = 0;
        *tx->bytes = text_base; ctx->aln_text_bytes = text_base;
        if (tx->text && text_short) return fail(ctx, RAWDTW_ERR_RANGE, "text_cap is below the text's size");
    }
    return RAWDTW_OK;
}

} // namespace capi
} // namespace rawdtw
