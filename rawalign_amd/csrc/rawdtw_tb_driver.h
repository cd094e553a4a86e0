// rawdtw_tb_driver.h -- the one host driver of every traceback (rawdtw_tb_driver.cpp): full matrix (rawdtw_traceback.cpp), banded
// (rawdtw_band_tb.cpp) and semiglobal (rawdtw_semiglobal.cpp).  The driver owns the split under "tb_workspace_mb", the two slots, the
// path buffers, the landing zone, the download beside the next sub-batch's kernels, the copy-out and the text form's tail; a unit hands
// it a TbPath, the few things that are its own.  Internal.
#pragma once
#include "rawdtw_capi.h"
#include "rawdtw_tb_layout.h"

namespace rawdtw {
namespace capi {

// a planned stretch of jobs, as the path's `plan` leaves it; `plan` is the path's own record of it
struct TbStretch {
    void *plan = nullptr;
    const uint32_t *order = nullptr; // position -> index inside the stretch
    const DevJob *jobs = nullptr;    // by position (the driver reads n and m: a path has n + m - 1 elements at most)
    uint64_t dir_bytes = 0;          // of the direction workspace this stretch writes
    tb::Recs recs;                   // the device records the path wants in the slot (need 0: the plan owns them) ...
    const float *d_cost = nullptr;   // ... and then the plan's costs; null: the slot's.  Indexed inside the stretch, lengths by position
    const FullAux *aux = nullptr;    // non-null: the driver puts jobs and aux into the slot in front of the fill's first event (banded: fill_ms never held them)
};

// a slot's device pointers for one stretch (rawdtw_tb_layout.h): the path's records, then the paths
struct TbSlot {
    DevJob *jobs; FullAux *aux; float *cost; uint32_t *endj; float *bnd;
    uint64_t *poff; uint32_t *plen, *extra, *ti, *tj; float *pd; uint8_t *mv;
};

struct TbPath {
    TbTiming rawdtw_ctx::*timing; // which of the context's records the call accumulates into
    bool dense;                   // the full-matrix steps entries: a stretch whose caller's offsets are dense is written in the caller's layout
    bool extra;                   // one more uint32 a job comes home by position, and seeds j when (i, j) is rebuilt (semiglobal's j0)
    const char *oom;              // the message when the slots' device block cannot be had
    uint64_t (*job_dir_bytes)(const rawdtw_ctx *ctx, const rawdtw_job_t &j); // as the split counts them
    int (*plan)(rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t cnt, TbStretch *out);
    int (*fill)(rawdtw_ctx *ctx, const TbStretch &s, const TbSlot &slot); // enqueue on ctx->stream: records up, the fill launches
    int (*walk)(rawdtw_ctx *ctx, const TbStretch &s, const TbSlot &slot); // ... the walk launches: lengths, steps and distances are in the slot behind them
    void (*release)(void *plan);                                          // called once the streams are idle
};

// What the banded and the semiglobal unit plan of a stretch [begin, begin + cnt): the jobs in launch order -- by class, the longest
// first inside a class (keys ascending, then job order) --, one launch a class; a record's aux is the job's index inside the stretch.
struct ClassLaunch { int cls; uint64_t first, count; uint32_t max_k; };
struct ClassPlan {
    std::vector<uint32_t> order; // position -> index inside the stretch
    std::vector<DevJob> jobs;
    std::vector<FullAux> aux;
    std::vector<ClassLaunch> launches;
    uint64_t bnd_floats = 0, dir_bytes = 0;
};
struct Keyed { uint64_t key; uint32_t idx; };
inline void sort_keyed(std::vector<Keyed> &v) { std::sort(v.begin(), v.end(), [](const Keyed &x, const Keyed &y) { return x.key != y.key ? x.key < y.key : x.idx < y.idx; }); }
// ... as the driver takes it: the records in the slot (end columns and boundary rows: semiglobal), released by class_release
inline TbStretch class_stretch(ClassPlan *pl, bool endj)
{
    return TbStretch{pl, pl->order.data(), pl->jobs.data(), pl->dir_bytes, tb::recs(pl->jobs.size(), sizeof(DevJob), sizeof(FullAux), endj, false, pl->bnd_floats), nullptr,
                     endj ? nullptr : pl->aux.data()}; // (semi_fill, which the cost and span forms share, sends its own records)
}
inline void class_release(void *plan) { delete static_cast<ClassPlan *>(plan); }

// where the paths go: exactly one of step and (i, j); extra iff the path has one.  The text form gives none of off, step, i, j, d.
struct TbOut { float *cost; uint32_t *extra; const uint64_t *off; uint32_t *len; uint8_t *step; uint32_t *i, *j; float *d; };

// the text form (include/rawdtw.h, "aln text"): full matrix only
struct TbText { const rawdtw_aln_rec_t *recs; uint64_t *text_off; char *text; uint64_t cap; uint64_t *bytes; };

// Everything behind a unit's refusals and its event upload.  Sets "tb_sub_batches" and the path's timing record.
int tb_run(rawdtw_ctx *ctx, const TbPath &path, const rawdtw_job_t *jobs, uint64_t n_jobs, const TbOut &out, const TbText *tx);

// the one body of rawdtw_traceback_timing, rawdtw_banded_traceback_timing and rawdtw_semiglobal_timing
inline int tb_timing_get(const rawdtw_ctx *ctx, TbTiming rawdtw_ctx::*which, float *fill_ms, float *walk_ms, uint64_t *direction_bytes, uint64_t *path_elements)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    const TbTiming &t = ctx->*which;
    if (fill_ms) *fill_ms = t.fill_ms;
    if (walk_ms) *walk_ms = t.walk_ms;
    if (direction_bytes) *direction_bytes = t.dir_written;
    if (path_elements) *path_elements = t.path_elems;
    return RAWDTW_OK;
}

} // namespace capi
} // namespace rawdtw
