// The chunk map of a pass of k_runs: which of the pass's sorted job records a wave takes together.  Shared by the kernel
// (rawdtw_runs.hip: run_dp), the plan's profile (rawdtw_plan_check.cpp) and plain C++ test programs
// (tests/abi/chunk_map.cpp, tests/abi/plan_fmt.cpp): no HIP include here.  The records themselves: rawdtw_plan_fmt.h.
//
// A pass's records are sorted radius 3 first, then 2, then 1, each run by longer side, descending (k_plan).  With
//   n3      the radius-3 records the quads take: those among the pass's first 64,
//   n_hi    the index of the pass's first radius-1 record (= the records of radius >= 2),
//   n_jobs  the pass's records,                                       n3 <= n_hi <= n_jobs,
// the chunks are, in order:
//   ceil(n3 / 16)            quad chunks of 16 records over [0, n3)        (four lanes a job: quad_dp_r3),
//   ceil((n_hi - n3) / 64)   lane chunks of 64 records over [n3, n_hi)     (radius 2; radius-3 records beyond the first 64),
//   ceil((n_jobs - n_hi) / 64) lane chunks of 64 records over [n_hi, n_jobs) (radius 1).
// No chunk holds records of both sides of n_hi: a wave never runs the shortest radius-2 parts and the longest radius-1
// parts of a pass under one body for the longest side of the two.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RAWDTW_CHUNK_FN __host__ __device__ inline
#else
#define RAWDTW_CHUNK_FN inline
#endif

namespace rawdtw {

struct ChunkRange {
    uint32_t first, end; // records [first, end) of the pass's order
    bool quad;           // sixteen records, four lanes each
};

RAWDTW_CHUNK_FN uint32_t chunk_map_quads(uint32_t n3) { return (n3 + 15u) >> 4; }
RAWDTW_CHUNK_FN uint32_t chunk_map_count(uint32_t n3, uint32_t n_hi, uint32_t n_jobs)
{
    return chunk_map_quads(n3) + ((n_hi - n3 + 63u) >> 6) + ((n_jobs - n_hi + 63u) >> 6);
}
// chunk c < chunk_map_count(n3, n_hi, n_jobs)
RAWDTW_CHUNK_FN ChunkRange chunk_map_range(uint32_t n3, uint32_t n_hi, uint32_t n_jobs, uint32_t c)
{
    const uint32_t q3 = chunk_map_quads(n3), c_lo = q3 + ((n_hi - n3 + 63u) >> 6); // the first radius-1 chunk
    ChunkRange r;
    r.quad = c < q3;
    if (r.quad) {
        r.first = c * 16u;
        r.end = r.first + 16u < n3 ? r.first + 16u : n3;
    } else if (c < c_lo) {
        r.first = n3 + (c - q3) * 64u;
        r.end = r.first + 64u < n_hi ? r.first + 64u : n_hi;
    } else {
        r.first = n_hi + (c - c_lo) * 64u;
        r.end = r.first + 64u < n_jobs ? r.first + 64u : n_jobs;
    }
    return r;
}
// (n_hi = n_jobs gives the map before the radius-1 run had a boundary of its own: the lane chunks cut every 64 records from
// n3 on -- what the plan's profile compares with)

} // namespace rawdtw
