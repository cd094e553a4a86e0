// rawdtw_semiglobal.h -- what rawdtw_semiglobal_kernels.hip (the kernels) and rawdtw_semiglobal.cpp (validation, classes, launches, sub-batches)
// share: a job's class, the sizes of its boundary rows (the cost and traceback forms', the span form's) and of its packed directions,
// and the launchers.
#pragma once
#include <cstdint>

#include "rawdtw_internal.h"

namespace rawdtw {

// A semiglobal job's wave class: 0..3 = 1, 2, 4, 8 rows a lane on one wave, by n ALONE (a always lies over the lanes: the rule of the
// full-matrix classes, full_rpl, applied to n), 4 = 8 rows a lane on four pipelined waves: three strips or more, under the guards of
// the progress word (m < 2^21 columns, fewer than 2^11 strips) and the context's "full_wg".
constexpr int kSemiClasses = kWaveClasses; // (the wave classes of rawdtw_launches.h)
inline int semi_rpl(int cls) { return kWaveClass[cls].rows; }
inline int semi_class(uint32_t n, uint32_t m, bool full_wg)
{
    const int c = n <= 64 ? 0 : n <= 128 ? 1 : n <= 256 ? 2 : 3;
    if (c == 3 && n > 2 * 512u && full_wg && m < (1u << 21) && (n + 511u) / 512u < (1u << 11)) return 4;
    return c;
}
// floats of boundary rows (none for a one-strip job; a ring of kFullWgWaves rows for the pipelined class)
inline uint64_t semi_bnd_floats(uint32_t n, uint32_t m, int cls)
{
    if (n <= 64u * (uint32_t)semi_rpl(cls)) return 0;
    return (uint64_t)kWaveClass[cls].waves * (((uint64_t)m + 63) & ~63ull);
}
// the span form's boundary rows, in floats: a slot holds the row of costs and behind it the row of start columns
inline uint64_t semi_span_bnd_floats(uint32_t n, uint32_t m, int cls) { return 2 * semi_bnd_floats(n, m, cls); }
// bytes of packed directions: [strip][block][lane][step in block], blocks of 16 bytes a lane (k_semi_wave)
inline uint64_t semi_dir_bytes(uint32_t n, uint32_t m, int cls)
{
    const uint64_t rpl = (uint64_t)semi_rpl(cls);
    const uint64_t strips = (n + 64 * rpl - 1) / (64 * rpl);
    const uint64_t spb = rpl == 8 ? 8 : 16;
    return strips * (((uint64_t)m + 63 + spb - 1) / spb) * 64 * 16;
}

hipError_t launch_semi_wave(int cls, bool traceback, const DevJob *jobs, uint64_t count, const FullAux *aux, const float *ev,
                            const float *ref, float *out_cost, uint32_t *out_end_j, float *bnd_ws, uint8_t *dir_ws, hipStream_t s);
// the span form (k_semi_span_wave): cost, j0 and end_j; bnd_ws laid out by semi_span_bnd_floats
hipError_t launch_semi_span_wave(int cls, const DevJob *jobs, uint64_t count, const FullAux *aux, const float *ev, const float *ref,
                                 float *out_cost, uint32_t *out_j0, uint32_t *out_end_j, float *bnd_ws, hipStream_t s);
// the walk from (n - 1, end_j) to row 0 (end-first (i, j) into tmp_i / tmp_j), then start-first steps, distances and j0
hipError_t launch_semi_walk(int cls, const DevJob *jobs, uint64_t count, const FullAux *aux, const float *ev, const float *ref,
                            const uint8_t *dir_ws, const uint32_t *end_j, const uint64_t *path_off, uint32_t *path_len,
                            uint32_t *path_j0, uint32_t *tmp_i, uint32_t *tmp_j, uint8_t *path_mv, float *path_d, hipStream_t s);
// The traceback in windows (rawdtw_semi_window.h): the cost form that also keeps the checkpoint columns (k_semi_ckpt_wave; dir_ws: the
// jobs' stretches of window directions and checkpoints), and behind it the window kernel (k_semi_window: refill and walk, end-first
// (i, j) into tmp_i / tmp_j; stats[0] += windows entered, stats[1] = max over jobs) followed by k_semi_finish as in launch_semi_walk
hipError_t launch_semi_ckpt_wave(int cls, const DevJob *jobs, uint64_t count, const FullAux *aux, const float *ev, const float *ref,
                                 float *out_cost, uint32_t *out_end_j, float *bnd_ws, uint8_t *dir_ws, uint32_t columns, hipStream_t s);
hipError_t launch_semi_window(int cls, const DevJob *jobs, uint64_t count, const FullAux *aux, const float *ev, const float *ref,
                              float *bnd_ws, uint8_t *dir_ws, const uint32_t *end_j, const uint64_t *path_off, uint32_t *path_len,
                              uint32_t *path_j0, uint32_t *tmp_i, uint32_t *tmp_j, uint8_t *path_mv, float *path_d, uint32_t columns,
                              unsigned long long *stats, hipStream_t s);

} // namespace rawdtw
