// rawdtw_semi_window.h -- the semiglobal traceback in windows (include/rawdtw.h, "semiglobal, in windows") as numbers: which jobs are
// windowed, a job's checkpoint columns and where their floats lie, the window of a walk position, a windowed job's direction bytes and
// what the sub-batch split counts for it.  The kernels (rawdtw_semiglobal_kernels.hip), the host unit (rawdtw_semiglobal.cpp) and the
// host restatement (rawdtw_host.cpp) share it.  No HIP include: a plain compiler takes it (tests/abi/semi_window_layout.cpp).
//
// A windowed job's stretch of the direction workspace, from its dir_off on:
//   [ directions of one window: dir_bytes(n, m, C, rpl), rounded up to 256 ][ checkpoints: (m / C) columns of n floats, rounded up to 256 ]
// Checkpoint k - 1 (k >= 1) is column k C - 1 of D, row i at float (k - 1) n + i.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RAWDTW_SW_HD __host__ __device__
#else
#define RAWDTW_SW_HD
#endif

namespace rawdtw {
namespace semi_window {

constexpr uint32_t kMinColumns = 64, kMaxColumns = 1u << 20;

// what rawdtw_set_semiglobal_window stores: 0 (off) or a multiple of 64 in [64, 2^20]
RAWDTW_SW_HD inline bool valid_columns(uint64_t c) { return c == 0 || (c >= kMinColumns && c <= kMaxColumns && c % 64 == 0); }
// a job with m <= C has one window, the matrix: it is not windowed
RAWDTW_SW_HD inline bool windowed(uint32_t m, uint32_t C) { return C != 0 && m > C; }
RAWDTW_SW_HD inline uint64_t al256(uint64_t x) { return (x + 255) & ~255ull; }

// checkpoints: every k >= 1 with k C - 1 < m
RAWDTW_SW_HD inline uint64_t checkpoints(uint32_t m, uint32_t C) { return m / C; }
RAWDTW_SW_HD inline uint64_t ckpt_floats(uint32_t n, uint32_t m, uint32_t C) { return checkpoints(m, C) * n; }
RAWDTW_SW_HD inline uint64_t ckpt_bytes(uint32_t n, uint32_t m, uint32_t C) { return al256(ckpt_floats(n, m, C) * 4); }
// float offset of column `col` (== C - 1 mod C) inside the job's checkpoints
RAWDTW_SW_HD inline uint64_t ckpt_at(uint32_t n, uint32_t C, uint32_t col) { return (uint64_t)((col + 1) / C - 1) * n; }

// the window of a walk position (i, j), i > 0: columns lo(j, C) .. j; column lo - 1 is a checkpoint unless lo == 0
RAWDTW_SW_HD inline uint32_t lo(uint32_t j, uint32_t C) { return (j / C) * C; }
RAWDTW_SW_HD inline uint32_t width(uint32_t m, uint32_t C) { return C < m ? C : m; }

// bytes of one window's packed directions: k_semi_wave's layout over width(m, C) columns, i.e. semi_dir_bytes(n, min(C, m), cls)
// (rawdtw_semiglobal.h) -- [strip][block][lane][step in block], blocks of 16 bytes a lane; rpl: rows a lane of the job's class
RAWDTW_SW_HD inline uint64_t dir_bytes(uint32_t n, uint32_t m, uint32_t C, uint32_t rpl)
{
    const uint64_t strips = ((uint64_t)n + 64ull * rpl - 1) / (64ull * rpl);
    const uint64_t spb = rpl == 8 ? 8 : 16;
    return strips * (((uint64_t)width(m, C) + 63 + spb - 1) / spb) * 64 * 16;
}
// where the checkpoints start behind the job's dir_off, and the job's whole stretch: what the plan lays out and the split counts
RAWDTW_SW_HD inline uint64_t ckpt_off(uint32_t n, uint32_t m, uint32_t C, uint32_t rpl) { return al256(dir_bytes(n, m, C, rpl)); }
RAWDTW_SW_HD inline uint64_t job_bytes(uint32_t n, uint32_t m, uint32_t C, uint32_t rpl) { return ckpt_off(n, m, C, rpl) + ckpt_bytes(n, m, C); }

} // namespace semi_window
} // namespace rawdtw
