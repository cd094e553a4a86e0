// rawdtw_wavefront.h -- what the skewed-wavefront kernels of the full-matrix and semiglobal DP share, each piece once: the direction
// word, code, packing and flush of the fills (k_full_wave in rawdtw_kernels.hip; semi_wave_body and k_semi_window in
// rawdtw_semiglobal_kernels.hip), the step and the output buffer of the walks (k_tb_walk_wave, k_semi_walk_wave, k_semi_window), the
// finish -- device code --, and at the end the launchers' host-side class dispatch (with_wave_class, with_wave_rows).  Include from .hip
// files.
//
// The fill (the loop itself stands in each kernel: its borders, results and side outputs differ).  The sequence Y lies over the lanes,
// RPL consecutive rows a lane, 64 * RPL rows a strip; the sequence X is swept column by column with a one-column skew a lane (lane l
// works on column t - l at step t), so every step advances a 64-cell-wide anti-diagonal whose cells exchange values through DPP wave
// shifts only.  A strip hands its last row to the next one through a boundary row in HBM, read and written in 64-float chunks.
// WAVES = 1: one wave a job, strips in sequence.  WAVES > 1: the workgroup's waves take strips w, w + WAVES, ... as a pipeline, strip
// s + 1 trailing strip s by at least one chunk; boundary rows are then a ring of WAVES rows, a strip publishes the columns it has flushed
// through an LDS progress word, (strip << 21) | columns (it only ever grows), and its successor spins on that word before each chunk
// load.  With directions, the 2-bit move of the walk is decided at fill time from the cell's three neighbours and packed RPL codes a
// lane a step.
#pragma once
#include <type_traits>

#include "rawdtw_internal.h"
#include "rawdtw_dp.h"

namespace rawdtw {
namespace wf {

// DTW_global, DTW_global_tb and the semiglobal forms have no sentinel (dtw.cpp:37-66, 595-667: row 0 and column 0 are running sums,
// whatever they pass), so what lies beyond the matrix must lose every min: +inf, not the banded DP's 1e10 -- a border sum above 1e10
// would otherwise be replaced by it, and the direction codes of the interior decided from the replaced values.  Every cell has a
// finite neighbour, the corner's 0 or an assigned row 0, so no cell of the matrix is ever +inf itself.
constexpr float kNone = __builtin_inff();

// A lane's RPL 2-bit codes of a step are one direction word.  Words are written in blocks of SPB steps: a lane's SPB consecutive
// words are 16 contiguous bytes, so a block leaves the wave as one 1-KiB dwordx4 store: [strip][block][lane][step in block].
// (The hosts' sizes of that buffer: dir_bytes_for, semi_dir_bytes, semi_window::dir_bytes.)
template <int RPL> struct DirWord { using type = uint8_t; };
template <> struct DirWord<8> { using type = uint16_t; };
template <int RPL> constexpr uint32_t SPB = 16u / sizeof(typename DirWord<RPL>::type);
static_assert(SPB<1> == 16 && SPB<2> == 16 && SPB<4> == 16 && SPB<8> == 8, "the hosts' formulas: 8 steps a block at 8 rows a lane, else 16");
// blocks per strip of a fill over `cols` columns (T: the kernel's width of that number)
template <int RPL, typename T> __device__ __forceinline__ T strip_blocks(T cols) { return (cols + 63 + SPB<RPL> - 1) / SPB<RPL>; }

// The shared pieces take the loop's running values and return the new ones BY VALUE, never through a reference: a local whose address
// is taken stays in memory until the piece is inlined, and becomes a register in a later pass and another order than its neighbours
// -- the kernels' register allocation moves with that.  For the same reason a piece's guard stays with its caller where the guard
// shares a term with the caller's other text ("The wavefront pieces": what is shared, and what moved a stream and is not).

__device__ __forceinline__ float min2f(float a, float b)
{
    // (as the instruction: through fminf the compiler quiets signalling NaNs first, two more instructions an operand)
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// The direction code of a cell from its three neighbours, up = D(row - 1, column), left = D(row, column - 1), diag: the walk's rule
// (dtw.cpp:633-646, 717-730) is  up < min(left, diag) -> "up" ; else left < min(up, diag) -> "left" ; else the diagonal.  "up strictly
// best" and "left strictly best" exclude each other, so the code is two bit planes.  Six instructions a cell: per plane v_min_f32,
// v_cmp_lt_f32 into VCC and v_addc_co_u32 code = 2 code + VCC -- the compare's bit shifts in from below, no select, no shift-or.  The
// word grows most significant cell first, "up" before "left": dir_put turns it round.
__device__ __forceinline__ uint32_t dir_code(uint32_t code, float up, float left, float diag)
{
    const float t_up = min2f(left, diag);
    asm volatile("v_cmp_lt_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(code) : "v"(up), "v"(t_up) : "vcc");
    const float t_lf = min2f(up, diag);
    asm volatile("v_cmp_lt_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(code) : "v"(left), "v"(t_lf) : "vcc");
    return code;
}

// A step's word into the wave's LDS transposition buffer ([lane][step in block], 64 * SPB words).  Bit reversal puts cell k at bits
// 2k ("up": row - 1, code 1) and 2k + 1 ("left": column - 1, code 2).  `swapped` (k_full_wave, n > m: the rows are b's): the planes
// the other way round -- adjacent bits change places.
template <int RPL>
__device__ __forceinline__ void dir_put(typename DirWord<RPL>::type *tbuf, int lane, uint32_t t, uint32_t code, bool swapped = false)
{
    uint32_t w = __builtin_bitreverse32(code) >> (32 - 2 * RPL);
    if (swapped) w = ((w & 0x55555555u) << 1) | ((w >> 1) & 0x55555555u);
    tbuf[lane * SPB<RPL> + (t % SPB<RPL>)] = (typename DirWord<RPL>::type)w;
}

// Behind a block's last step (and the strip's), (t % SPB) == SPB - 1 || t + 1 == steps: each lane reads its 16 bytes back and the block
// leaves as one store.  TXB: blocks a strip.
template <int RPL>
__device__ __forceinline__ void dir_flush(const typename DirWord<RPL>::type *tbuf, uint4 *dirs, uint64_t TXB, uint32_t s, uint32_t t, int lane,
                                          bool has_rows)
{
    // same wave wrote and reads the buffer; LDS operations of a wave complete in order, the
    // fence keeps the compiler from reordering the differently typed accesses
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const uint4 blk = *reinterpret_cast<const uint4 *>(&tbuf[lane * SPB<RPL>]);
    if (has_rows) dirs[((uint64_t)s * TXB + t / SPB<RPL>) * 64u + lane] = blk;
}

// The walk, one wave a job.  (A lane-per-job walk chases one direction word a step through HBM: ~3.5 us a step, 5 ms for a thousand
// 1500-step paths.)  A path moving up the diagonal stays ~7 steps inside one 1-KiB block row of the direction buffer: the wave fetches
// the block row with one coalesced load into LDS (`row`, 64 * SPB words; `cur`: the one it holds, ~0 for none) and all lanes walk it
// in lockstep on uniform values.  (Prefetching the next row was measured: no gain, the walk's own dependent chain -- LDS read, decode,
// branch -- is what a step costs.)  One step from row y, column x of a fill whose strips have TXB blocks: i and j move by its code.
// The next block row overwrites `row` only behind the barrier that follows the load, which all lanes reach together, the walk being
// uniform; BARRIER_FIRST: one before the load as well (k_semi_window, whose refill comes between two walks).
struct WalkPos { uint32_t i, j; uint64_t cur; };
template <int RPL, bool BARRIER_FIRST>
__device__ __forceinline__ WalkPos walk_step(WalkPos p, const uint4 *dirs, typename DirWord<RPL>::type *row, uint64_t TXB, int lane,
                                             uint32_t y, uint32_t x, uint32_t x_lo = 0)
{
    const uint32_t sidx = y / (64u * RPL), l = (y / RPL) & 63u, kk = y % RPL;
    const uint32_t t = (x - x_lo) + l;
    const uint64_t key = (uint64_t)sidx * TXB + t / SPB<RPL>;
    if (key != p.cur) {
        if (BARRIER_FIRST) __builtin_amdgcn_s_barrier(); // (every lane has read the row that goes)
        reinterpret_cast<uint4 *>(row)[lane] = dirs[key * 64u + lane];
        p.cur = key;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    uint32_t word = row[l * SPB<RPL> + (t % SPB<RPL>)];
    word = (uint32_t)__builtin_amdgcn_readfirstlane((int)word);
    const uint32_t code = (word >> (2 * kk)) & 3u;
    if (code == 1u) p.i--;
    else if (code == 2u) p.j--;
    else { p.i--; p.j--; }
    return p;
}

// The walk's output, (i, j) end-first into tmp_i / tmp_j from `po` on: steps are buffered one a lane (lane = step & 63) and leave as
// coalesced 64-step stores.  Step 0 is the end cell, so a walk counts its steps k from 1; push takes k and returns k + 1.
struct PathBuf {
    uint32_t *tmp_i, *tmp_j;
    uint64_t po;
    int lane;
    uint32_t bi, bj;
    __device__ __forceinline__ void flush(uint32_t upto) // steps [upto - ((upto - 1) & 63) - 1 .. upto) sit in lanes 0..(upto-1)&63
    {
        const uint32_t base = (upto - 1) & ~63u;
        if ((uint32_t)lane <= ((upto - 1) & 63u)) { tmp_i[po + base + lane] = bi; tmp_j[po + base + lane] = bj; }
    }
    __device__ __forceinline__ uint32_t push(uint32_t k, uint32_t i, uint32_t j)
    {
        if ((uint32_t)lane == (k & 63u)) { bi = i; bj = j; }
        k++;
        if ((k & 63u) == 0) flush(k);
        return k;
    }
    __device__ __forceinline__ void finish(uint32_t k) { if ((k & 63u) != 0) flush(k); }
};

// Start-first order and the per-step distance, one thread per path element (blocks of 256, one a job).  What leaves the device per
// element is its distance and ONE byte: the step from the element before it (bit 0: i advanced, bit 1: j advanced; element 0's is 0)
// -- the host rebuilds (i, j) while it writes the caller's arrays; 5 bytes an element over the bus instead of 12.  J0: and the column
// the path starts in (a global path starts at (0, 0): dtw.cpp:640-655).  A job whose path_len is 0 gets nothing written.
template <bool J0>
__device__ __forceinline__ void finish_body(const DevJob *__restrict__ jobs, uint32_t count, const float *__restrict__ ev,
                                            const float *__restrict__ ref, const uint64_t *__restrict__ path_off,
                                            const uint32_t *__restrict__ path_len, const uint32_t *__restrict__ tmp_i,
                                            const uint32_t *__restrict__ tmp_j, uint32_t *__restrict__ path_j0,
                                            uint8_t *__restrict__ path_mv, float *__restrict__ path_d)
{
    const uint32_t g = blockIdx.x;
    if (g >= count) return;
    const DevJob jb = jobs[g];
    const float *a = ev + jb.read_off;
    const float *b = ref + jb.ref_off;
    const uint64_t po = path_off[g];
    const uint32_t len = path_len[g];
    for (uint32_t q = threadIdx.x; q < len; q += 256) {
        const uint32_t i = tmp_i[po + len - 1 - q], j = tmp_j[po + len - 1 - q];
        uint32_t mv = 0;
        if (q) mv = (i - tmp_i[po + len - q]) | ((j - tmp_j[po + len - q]) << 1);
        else if (J0) path_j0[g] = j;
        path_mv[po + q] = (uint8_t)mv; path_d[po + q] = dist(a[i], b[j]);
    }
}

} // namespace wf

// The launchers' dispatch: a wave class (rawdtw_launches.h) as compile-time (rows a lane, waves a job), and as rows a lane alone for
// the one-wave kernels behind the fill.  f returns the launch's hipError_t; a class outside the table is hipErrorInvalidValue.
template <int CLS = 0, typename F> hipError_t with_wave_class(int cls, F &&f)
{
    if constexpr (CLS == kWaveClasses) return hipErrorInvalidValue;
    else if (cls == CLS) return f(std::integral_constant<int, kWaveClass[CLS].rows>{}, std::integral_constant<int, kWaveClass[CLS].waves>{});
    else return with_wave_class<CLS + 1>(cls, f);
}
template <typename F> hipError_t with_wave_rows(int cls, F &&f)
{
    return with_wave_class(cls, [&](auto rpl, auto) { return f(rpl); });
}

} // namespace rawdtw
