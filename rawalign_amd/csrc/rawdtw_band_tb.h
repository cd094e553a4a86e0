// rawdtw_band_tb.h -- what rawdtw_band_tb.hip (the kernels) and rawdtw_band_tb.cpp (validation, launches, sub-batches) share: the layout of
// a banded traceback job's directions, and the launchers.  The definition of the banded path is in include/rawdtw.h.
//
// Direction layout of ONE job (n, m, R0), at FullAux::dir_off (256-byte aligned), N = max(n, m), M = min(n, m), R = slanted_radius,
// K = R + 1 slots an antidiagonal (dtw.cpp:301-305), I indexing the LONGER sequence and J the shorter (the reference's swap):
//
//   records   n + m - 1 of BandTbRec, one an antidiagonal sum s = I + J = 0 .. n + m - 2.  Every s is produced exactly once, as the
//             secondary or the primary antidiagonal of some column (s = 0: column 0's corner).  Offset o of the antidiagonal is the
//             cell (I, J) = (si - o, sj + o); the cell is in S (was evaluated) iff lo <= o < hi.
//   rows      n + m - 1 rows of band_tb_row_bytes(K) bytes, row s behind the records.  A row is ceil(K / 64) chunks of 16 bytes; chunk c
//             holds offsets 64 c .. 64 c + 63 as two 64-bit planes: bit (o & 63) of plane 0 is bit 0 of offset o's code, of plane 1
//             its bit 1.  Codes are the walk's (dtw.cpp:633-646) in the caller's UNSWAPPED i, j: 0 both, 1 i - 1, 2 j - 1; offsets
//             outside [lo, hi) hold 0.
#pragma once
#include <cstdint>

#include "rawdtw_internal.h"

namespace rawdtw {

struct BandTbRec { int32_t si, sj, lo, hi; };
static_assert(sizeof(BandTbRec) == 16, "one 16-byte record an antidiagonal");

inline uint64_t band_tb_row_bytes(uint32_t K) { return (((uint64_t)K + 63) / 64) * 16; }
// bytes of one job's records and rows (the host rounds a job up to 256)
inline uint64_t band_tb_dir_bytes(uint32_t n, uint32_t m, int R)
{
    return ((uint64_t)n + m - 1) * (sizeof(BandTbRec) + band_tb_row_bytes((uint32_t)R + 1));
}
// the fill kernel's workgroup: one wave for a band of one chunk, four beyond (a wave a 64-slot chunk, in turns)
inline uint32_t band_tb_threads(uint32_t K) { return K <= 64 ? 64u : 256u; }

// jobs: DevJob with R = the slanted radius; out_cost is indexed by DevJob::aux.  lds_floats = 3 * the largest K of the launch.
hipError_t launch_band_tb_fill(const DevJob *jobs, uint64_t count, const FullAux *aux, uint32_t threads, uint32_t lds_floats, const float *ev,
                               const float *ref, float *out_cost, uint8_t *dir_ws, hipStream_t s);
// the walk from (n - 1, m - 1) to (0, 0), end-first (i, j) into tmp_i / tmp_j; path_len 0 for a job without a path
hipError_t launch_band_tb_walk(const DevJob *jobs, uint64_t count, const FullAux *aux, const uint8_t *dir_ws, const uint64_t *path_off,
                               uint32_t *path_len, uint32_t *tmp_i, uint32_t *tmp_j, hipStream_t s);

} // namespace rawdtw
