// The host's readers of a device-planned batch's plan (rawdtw_plan_check.cpp): pure functions over host arrays, no HIP --
// rawdtw_batch.cpp downloads the plan and calls them, tests/abi/plan_fmt.cpp calls them on a hand-built plan.
#pragma once
#include <string>

#include "../../include/rawdtw.h"
#include "rawdtw_plan_fmt.h"

namespace rawdtw {

// A batch's plan on the host: the scalars of its StreamArgs, its counters, the downloaded arrays.
struct StreamPlanView {
    uint64_t n_anchors = 0, n_chains = 0;
    uint32_t n_tiles = 0, n_slots = 0, lds_floats = 0, lane_max_n = 0;
    int32_t lane_max_radius = 0;
    uint64_t n_first = 0, n_pool = 0, n_other = 0, n_reused = 0; // cnt[kCntTodo], [kCntPool], [kCntOthers], [kCntReused]
    // the work list's entries in use, one behind the other: entry q < n_first sits at slot q, entry q >= n_first at slot
    // n_tiles + (q - n_first)
    const PassEntry *todo = nullptr;
    const JobRec *recs = nullptr;       // all of them: n_tiles x kStreamRecStride
    const CopyOrder *runtab = nullptr;  // the slots in use, in the order of `todo`: entry q's orders at q * 2 kStreamMaxSeg
    const DevJob *side = nullptr;       // the side list: n_other records
    const uint64_t *anchor_off = nullptr; // n_chains + 1
    uint64_t n_todo() const { return n_first + n_pool; }
    bool fits_slots() const { return n_first <= n_tiles && n_tiles <= n_slots && n_pool <= n_slots - n_tiles; }
    uint32_t slot_of(uint64_t q) const { return (uint32_t)(q < n_first ? q : n_tiles + (q - n_first)); }
};

struct StreamPlanStats { uint64_t tile_jobs = 0, tile_bytes = 0, other_bytes = 0; }; // what k_stream_stats must sum to

// The plan against the job list the host builds from the same chains (rawdtw_batch_build_jobs).  Returns the first thing
// that is wrong, or "" -- then `expect` holds the statistics the jobs add up to.
std::string check_stream_plan(const StreamPlanView &v, const rawdtw_job_t *jobs, uint64_t n_jobs, StreamPlanStats *expect);

// The tile launch's chunks, counted from the plan as k_runs walks it: per body class -- 0 quad_dp_r3, 1 lane_dp_r2,
// 2 lane_dp_r12, 3 lane_dp_r1, 4 lane_dp_gen -- jobs, chunks, the chunks' columns (a chunk runs for its longest side) and
// the jobs' own columns; word 20 the passes.  flat_map: the map without a boundary at the radius-1 run (rawdtw_chunks.h).
// False: a work list entry is out of range.
bool stream_chunk_profile(const StreamPlanView &v, bool flat_map, uint64_t w[21]);

} // namespace rawdtw
