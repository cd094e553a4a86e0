// rawdtw_semiglobal_kernels.hip -- gfx950 kernels for subsequence DTW: a aligned end to end against the best-matching substring of b.
//
// What they replace (reference file:line):
//   k_semi_wave<.,false>                                   : DTW_semiglobal, DTW_semiglobal_slow   src/dtw.cpp:526-593
//   k_semi_wave<.,true> + k_semi_walk_wave + k_semi_finish : DTW_semiglobal_tb                     src/dtw.cpp:669-753
//   k_semi_span_wave                                       : cost, end_j and path[0].j of DTW_semiglobal_tb, no direction matrix
//
// k_semi_wave is the sibling of k_full_wave (rawdtw_kernels.hip): both run the strip loop of rawdtw_wavefront.h, with the same packed
// 2-bit directions in the same buffer layout.  What differs:
//   no transposition  the recurrence is not symmetric: a ALWAYS lies over the lanes and b is swept, also when n > m, so a
//                     direction code never changes its meaning (1: i - 1, 2: j - 1, 0: both).
//   borders           row 0 is assigned, D(0, j) = d(0, j): the lane that holds it takes the distance itself, no minimum with a made-up
//                     neighbour.  Column 0 is the running sum as in the full matrix (beyond the matrix lies +inf, which loses every min).
//   result            the minimum of the last row and the FIRST column that attains it: the lane that owns row n - 1 keeps a running
//                     (minimum, column) pair over the columns it finishes, replaced on strict < only -- columns ascend in a lane, so
//                     the first one wins as in dtw.cpp:577-585.  No reduction over lanes, no second pass.  The register that holds
//                     row n - 1 is chosen OUTSIDE the column loop (a copy of the loop for each of the RPL places), so the loop
//                     pays one vector compare a column for it; the pair itself is kept by the scalar unit.
// Cell values do not depend on evaluation order (min is exact, each cell is one rounded subtract and one rounded add); built with
// -ffp-contract=off.  The sentinel-free recurrence: include/rawdtw.h, arithmetic contract.
#include <type_traits>

#include "rawdtw_internal.h"
#include "rawdtw_dp.h"
#include "rawdtw_semiglobal.h"
#include "rawdtw_semi_window.h"
#include "rawdtw_wavefront.h"

namespace rawdtw {

// The span form's choice of a cell's start: ab < t_up ? s_up : (left < t_lf ? s_left : s_diag), with t_up = min(left, diag) and
// t_lf = min(ab, diag) -- the TB form's two comparisons, each into a lane mask, and two selects on the masks.  One statement, because
// the compiler does not look inside an asm string: on gfx950 a vector instruction that writes a scalar register (the compare's mask)
// needs two wait states before a vector instruction reads that register, and here they are there by construction -- between the
// first compare and its select lie the second compare and the s_nop, between the second compare and its select the s_nop and the
// first select.  (As four statements the compiler's scheduler decided the distance, and padded it to one state only.)
__device__ __forceinline__ uint32_t span_pick(float ab, float t_up, float left, float t_lf, uint32_t s_up, uint32_t s_left, uint32_t s_diag)
{
    uint32_t r;
    lmask m_up, m_lf;
    asm("v_cmp_lt_f32_e64 %[mlf], %[left], %[tlf]\n\t"
        "v_cmp_lt_f32_e64 %[mup], %[ab], %[tup]\n\t"
        "s_nop 0\n\t"
        "v_cndmask_b32_e64 %[r], %[sdiag], %[sleft], %[mlf]\n\t"
        "v_cndmask_b32_e64 %[r], %[r], %[sup], %[mup]"
        : [r] "=&v"(r), [mlf] "=&s"(m_lf), [mup] "=&s"(m_up)
        : [ab] "v"(ab), [tup] "v"(t_up), [left] "v"(left), [tlf] "v"(t_lf), [sup] "v"(s_up), [sleft] "v"(s_left), [sdiag] "v"(s_diag));
    return r;
}

// WAVES = kFullWgWaves: jobs of three strips or more; the progress word holds (strip << 21) | columns, so m < 2^21 and fewer than
// 2^11 strips (semi_class sees to it).
//
// SPAN (never with TB): every cell also carries S(i, j), the column in which the path that the walk would take from it starts
// (include/rawdtw.h, "span").  One more register a row register, chosen from the three neighbours' starts by the very
// comparisons the TB form packs into its 2-bit code; the start travels wherever the value travels -- to the next lane beside
// last_out, along the diagonal beside diag_in, down to the next strip in a second boundary row behind the row of costs
// ([costs: row_stride][starts: row_stride] a ring slot, semi_span_bnd_floats), both stored before the one release fence and the
// one progress word.  Column -1's starts are 0 and so is every start a column-0 cell can choose from (the cell above it lies in
// column 0, the other two in column -1): S(i, 0) = 0 whatever the values.  The scalar (minimum, step) pair gains the owner
// lane's start of the cell that improved the minimum, read by the same branch.
//
// CKPT (the cost form only; include/rawdtw.h, "semiglobal, in windows"): a lane that finishes a column == C - 1 (mod C) stores its RPL
// values, rows inside the job only, into the job's checkpoints (rawdtw_semi_window.h: behind its window's directions in dir_ws).
// Which lane that is, is decided by the scalar unit: with tm = t mod C and seg = t / C kept as scalar counters (no division in the
// loop; C is a multiple of 64 and a wave has 64 lanes), lane l works on column t - l, so a checkpoint column is finished by lane 0 at
// tm == C - 1 (checkpoint seg) and by lane tm + 1 at tm <= 62 (checkpoint seg - 1); at every other step, C - 64 of every C, the
// vector unit sees nothing of it.  Progress words and fences are untouched.
template <int RPL, bool TB, bool SPAN, int WAVES, bool CKPT = false>
__device__ __forceinline__ void semi_wave_body(const DevJob *__restrict__ jobs, const FullAux *__restrict__ aux,
                                               const float *__restrict__ ev, const float *__restrict__ ref,
                                               float *__restrict__ out_cost, uint32_t *__restrict__ out_j0,
                                               uint32_t *__restrict__ out_end_j, float *__restrict__ bnd_ws,
                                               uint8_t *__restrict__ dir_ws, uint32_t ck_columns = 0)
{
    static_assert(!(TB && SPAN), "the span form writes no directions");
    static_assert(!CKPT || (!TB && !SPAN), "checkpoints are the cost form's");
    using word_t = typename wf::DirWord<RPL>::type;
    constexpr uint32_t SPB = wf::SPB<RPL>;
    constexpr float kNone = wf::kNone;
    const DevJob jb = jobs[blockIdx.x];
    const FullAux ax = aux[blockIdx.x];
    const int lane = threadIdx.x & 63;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // (wave-uniform, and known to be)
    const float *Y = ev + jb.read_off; // a: over the lanes
    const float *X = ref + jb.ref_off; // b: swept
    const uint32_t NY = jb.n, NX = jb.m;
    constexpr uint32_t STRIP = 64u * RPL;
    const uint32_t nstrips = (NY + STRIP - 1) / STRIP;
    const uint32_t TXB = (NX + 63 + SPB - 1) / SPB; // blocks per strip
    const uint32_t row_stride = (NX + 63u) & ~63u; // floats per boundary row (semi_bnd_floats)
    const uint32_t slot_stride = SPAN ? 2u * row_stride : row_stride; // (a span slot: the costs, then the starts)
    float *bnd_base = bnd_ws + ax.bnd_off;
    uint4 *dirs = reinterpret_cast<uint4 *>(dir_ws + ax.dir_off);
    float *ckpt = nullptr; // CKPT: the job's checkpoint columns
    if constexpr (CKPT) ckpt = reinterpret_cast<float *>(dir_ws + ax.dir_off + semi_window::ckpt_off(NY, NX, ck_columns, RPL));
    __shared__ __attribute__((aligned(16))) word_t tbuf_all[TB ? WAVES * 64 * SPB : 1];
    word_t *tbuf = tbuf_all + (TB ? wv * 64 * SPB : 0);
    __shared__ uint32_t progress[WAVES]; // progress[s % WAVES] = (s << 21) | columns of strip s flushed
    if (WAVES > 1) {
        if (threadIdx.x < WAVES) progress[threadIdx.x] = 0;
        __syncthreads();
    }

    // the lane that owns row n - 1, the running minimum of that row (its bits: wave-uniform), and the step at which the minimum last improved (strictly):
    // lane l works on column t - l at step t, so the first column that attains the minimum is best_t - owner
    const uint32_t owner = (uint32_t)__builtin_amdgcn_readfirstlane((int)(((NY - 1) / RPL) & 63u));
    const uint64_t owner_bit = 1ull << owner;
    uint32_t best_bits = 0x7f800000u; // +inf
    uint32_t best_t = owner;
    uint32_t best_s = 0; // SPAN: the start of the cell that holds the minimum
    for (uint32_t s = wv; s < nstrips; s += WAVES) {
        const float *bnd_in = bnd_base + (uint64_t)((s + WAVES - 1) % WAVES) * slot_stride; // written by strip s-1
        float *bnd = bnd_base + (uint64_t)(s % WAVES) * slot_stride;                          // read by strip s+1
        const uint32_t *sbnd_in = reinterpret_cast<const uint32_t *>(bnd_in) + row_stride;   // SPAN: the starts behind the costs
        uint32_t *sbnd = reinterpret_cast<uint32_t *>(bnd) + row_stride;
        const uint32_t y0 = (s * 64u + lane) * RPL;
        const uint32_t rows_here = (NY - s * STRIP) < STRIP ? (NY - s * STRIP) : STRIP;
        const uint32_t lanes_here = (rows_here + RPL - 1) / RPL;
        const uint32_t steps = NX + lanes_here - 1;
        const bool has_rows = y0 < NY;
        const bool hands_down = (s + 1 < nstrips); // then the strip is full and lane 63 owns its last row
        const bool row0 = (s == 0 && lane == 0); // this lane's first register is row 0: assigned, not minimised

        // The strip's column loop.  KK: the register of its lane in which row n - 1 lies (the last strip), -1: a strip above the last.
        auto strip = [&](auto kk_c) {
            constexpr int KK = decltype(kk_c)::value;
            float yv[RPL], v[RPL];
            uint32_t vs[RPL]; // SPAN: the starts of v[] (dead otherwise)
#pragma unroll
            for (int k = 0; k < RPL; k++) {
                uint32_t y = y0 + k;
                yv[k] = Y[y < NY ? y : NY - 1];
                v[k] = kNone; // column -1
                if (SPAN) vs[k] = 0;
            }
            float diag_in = kNone; // (row 0 has no corner to start from: it is assigned)
            float last_out = kNone, xval = 0.0f, xchunk = 0.0f, bchunk = kNone, wchunk = 0.0f;
            uint32_t sdiag_in = 0, slast_out = 0, sbchunk = 0, swchunk = 0; // SPAN: the starts beside diag_in, last_out, bchunk, wchunk
            uint32_t ck_tm = 0, ck_seg = 0; // CKPT: t mod C and t / C (wave-uniform)
            for (uint32_t t = 0; t < steps; t++) {
                if ((t & 63u) == 0) {
                    const uint32_t idx = t + lane;
                    xchunk = X[idx < NX ? idx : NX - 1];
                    if (s > 0) {
                        if (WAVES > 1) {
                            // wait until strip s-1 has flushed the columns of this chunk
                            const uint32_t need = ((s - 1) << 21) | ((t + 64u < NX) ? t + 64u : NX);
                            while (__hip_atomic_load(&progress[(s - 1) % WAVES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < need)
                                __builtin_amdgcn_s_sleep(1);
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                        }
                        bchunk = idx < NX ? bnd_in[idx] : kNone;
                        if (SPAN) sbchunk = idx < NX ? sbnd_in[idx] : 0u;
                    }
                }
                const float x0 = read_lane(xchunk, (int)(t & 63u));
                const float b0 = read_lane(bchunk, (int)(t & 63u));
                const float up_in = wave_shr1(last_out, b0);
                uint32_t sup_in = 0;
                if (SPAN) sup_in = wave_shr1(slast_out, read_lane(sbchunk, (int)(t & 63u)));
                xval = wave_shr1(xval, x0);
                const uint32_t x = t - (uint32_t)lane;
                if (x < NX) {
                    float d = diag_in, ab = up_in;
                    uint32_t sd = sdiag_in, sab = sup_in;
                    uint32_t code = 0;
#pragma unroll
                    for (int k = 0; k < RPL; k++) {
                        const float left = v[k];
                        const float dd = dist(xval, yv[k]);
                        float nv = min3f(ab, left, d) + dd;
                        if (k == 0) nv = row0 ? dd : nv; // D(0, j) = d(0, j)  (dtw.cpp:566-568, 679-681)
                        // dtw.cpp:717-730 with left = D[i-1][j] (here `ab`), top = D[i][j-1] (here `left`).  Row 0's codes are never read:
                        // the walk ends there.
                        if (TB) code = wf::dir_code(code, ab, left, d);
                        if (SPAN) {
                            // the TB form's two comparisons, each into a lane mask, and the start of the neighbour the walk would step
                            // to (else: the diagonal, the reference's quirk ab == left < d included).  Row 0 starts in its own column.
                            uint32_t ns = span_pick(ab, wf::min2f(left, d), left, wf::min2f(ab, d), sab, vs[k], sd);
                            if (k == 0) ns = row0 ? x : ns;
                            sd = vs[k]; sab = ns; vs[k] = ns;
                        }
                        d = left; ab = nv; v[k] = nv;
                    }
                    diag_in = up_in;
                    last_out = v[RPL - 1];
                    if (SPAN) { sdiag_in = sup_in; slast_out = vs[RPL - 1]; }
                    if constexpr (CKPT) {
                        const bool first = ck_tm == ck_columns - 1; // lane 0 finishes column t
                        if (first || ck_tm < 63u) {                  // (else: no lane is on a checkpoint column)
                            // (lane tm + 1 at seg == 0 would be in front of column 0: it is not inside `x < NX`)
                            if ((uint32_t)lane == (first ? 0u : ck_tm + 1u)) {
                                float *col = ckpt + (uint64_t)(first ? ck_seg : ck_seg - 1u) * NY;
#pragma unroll
                                for (int k = 0; k < RPL; k++)
                                    if (y0 + k < NY) col[y0 + k] = v[k];
                            }
                        }
                    }
                    if (TB) wf::dir_put<RPL>(tbuf, lane, t, code);
                }
                if constexpr (CKPT) {
                    if (++ck_tm == ck_columns) { ck_tm = 0; ck_seg++; }
                }
                if constexpr (KK >= 0) {
                    // (outside the lanes' `x < NX` block: a scalar register written under a divergent branch is no scalar to the compiler.  A lane
                    // outside its columns holds +inf or its last value in v[KK]: neither is below its minimum.)
                    // The running minimum of row n - 1 lives in a SCALAR register, and so does the step of its last strict improvement:
                    // one vector compare a column against the scalar, its mask cut down to the owner's bit; the scalar unit (which
                    // issues beside the other waves' vector work -- the loop is bound by the vector unit) branches over the update,
                    // a v_readlane of the new minimum and a move of the step, which a job takes a handful of times.  One vector
                    // instruction a column.  (As `if (cand < best)` on vector values the compiler built a branch around two moves.)
                    // The two statements below are one sequence; the span form's has two operands more (%2: the pair's start, %4: the
                    // starts' register), so its operand numbers differ from the other's: %3 there is %2 here, %5..%7 are %3..%5.
                    if constexpr (SPAN)
                        // (the same, and the owner lane's start of that cell)
                        asm volatile("v_cmp_gt_f32 vcc, %0, %3\n\t"
                                     "s_and_b64 vcc, vcc, %5\n\t"
                                     "s_cmp_lg_u64 vcc, 0\n\t"
                                     "s_cbranch_scc0 .Lsemi_keep_%=\n\t"
                                     "v_readlane_b32 %0, %3, %7\n\t"
                                     "v_readlane_b32 %2, %4, %7\n\t"
                                     "s_mov_b32 %1, %6\n"
                                     ".Lsemi_keep_%=:"
                                     : "+s"(best_bits), "+s"(best_t), "+s"(best_s)
                                     : "v"(v[KK]), "v"(vs[KK]), "s"(owner_bit), "s"(t), "s"(owner)
                                     : "vcc", "scc");
                    else
                        asm volatile("v_cmp_gt_f32 vcc, %0, %2\n\t"
                                     "s_and_b64 vcc, vcc, %3\n\t"
                                     "s_cmp_lg_u64 vcc, 0\n\t"
                                     "s_cbranch_scc0 .Lsemi_keep_%=\n\t"
                                     "v_readlane_b32 %0, %2, %5\n\t"
                                     "s_mov_b32 %1, %4\n"
                                     ".Lsemi_keep_%=:"
                                     : "+s"(best_bits), "+s"(best_t)
                                     : "v"(v[KK]), "s"(owner_bit), "s"(t), "s"(owner)
                                     : "vcc", "scc");
                }
                if (TB && ((t % SPB) == SPB - 1 || t + 1 == steps)) wf::dir_flush<RPL>(tbuf, dirs, TXB, s, t, lane, has_rows);
                if (hands_down && t >= 63u) {
                    // lane 63 finished column c = t-63 in this step; gather 64 of them, store coalesced
                    const uint32_t c = t - 63u;
                    const float v63 = read_lane(last_out, 63);
                    if ((uint32_t)lane == (c & 63u)) wchunk = v63;
                    if (SPAN) {
                        const uint32_t s63 = read_lane(slast_out, 63);
                        if ((uint32_t)lane == (c & 63u)) swchunk = s63;
                    }
                    if ((c & 63u) == 63u || c == NX - 1) {
                        const uint32_t base = c & ~63u;
                        if (base + lane <= c) bnd[base + lane] = wchunk;
                        if (SPAN && base + lane <= c) sbnd[base + lane] = swchunk; // (before the one fence and the one progress word)
                        if (WAVES > 1) {
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                            if (lane == 0)
                                __hip_atomic_store(&progress[s % WAVES], (s << 21) | (c + 1u), __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                }
            }
        };
        if (hands_down) strip(std::integral_constant<int, -1>{});
        else {
            const uint32_t kk = (NY - 1) % RPL; // wave-uniform
            if constexpr (RPL == 1) strip(std::integral_constant<int, 0>{});
            else if constexpr (RPL == 2) {
                if (kk == 0) strip(std::integral_constant<int, 0>{});
                else strip(std::integral_constant<int, 1>{});
            } else if constexpr (RPL == 4) {
                switch (kk) {
                case 0: strip(std::integral_constant<int, 0>{}); break;
                case 1: strip(std::integral_constant<int, 1>{}); break;
                case 2: strip(std::integral_constant<int, 2>{}); break;
                default: strip(std::integral_constant<int, 3>{}); break;
                }
            } else {
                switch (kk) {
                case 0: strip(std::integral_constant<int, 0>{}); break;
                case 1: strip(std::integral_constant<int, 1>{}); break;
                case 2: strip(std::integral_constant<int, 2>{}); break;
                case 3: strip(std::integral_constant<int, 3>{}); break;
                case 4: strip(std::integral_constant<int, 4>{}); break;
                case 5: strip(std::integral_constant<int, 5>{}); break;
                case 6: strip(std::integral_constant<int, 6>{}); break;
                default: strip(std::integral_constant<int, 7>{}); break;
                }
            }
        }
        __threadfence_block();
    }
    // the wave that ran the last strip owns the result, its lane that holds row n - 1 the pair
    if (nstrips > 0 && ((nstrips - 1) % WAVES) == wv) {
        float result = __builtin_bit_cast(float, best_bits);
        const uint32_t end_j = best_t - owner;
        if (lane == 0) {
            if (jb.flags & kFlagExcludeLast) result = result - dist(Y[NY - 1], X[end_j]); // dtw.cpp:587-589, 744-746
            out_cost[jb.aux] = result;
            out_end_j[jb.aux] = end_j;
            if (SPAN) out_j0[jb.aux] = best_s;
        }
    }
}

template <int RPL, bool TB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_semi_wave(const DevJob *__restrict__ jobs, const FullAux *__restrict__ aux,
                                                          const float *__restrict__ ev, const float *__restrict__ ref,
                                                          float *__restrict__ out_cost, uint32_t *__restrict__ out_end_j,
                                                          float *__restrict__ bnd_ws, uint8_t *__restrict__ dir_ws)
{
    semi_wave_body<RPL, TB, false, WAVES>(jobs, aux, ev, ref, out_cost, nullptr, out_end_j, bnd_ws, dir_ws);
}

// the span form: (cost, j0, end_j), no directions
template <int RPL, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_semi_span_wave(const DevJob *__restrict__ jobs, const FullAux *__restrict__ aux,
                                                               const float *__restrict__ ev, const float *__restrict__ ref,
                                                               float *__restrict__ out_cost, uint32_t *__restrict__ out_j0,
                                                               uint32_t *__restrict__ out_end_j, float *__restrict__ bnd_ws)
{
    semi_wave_body<RPL, false, true, WAVES>(jobs, aux, ev, ref, out_cost, out_j0, out_end_j, bnd_ws, nullptr);
}

// the cost form that also keeps the checkpoint columns of the traceback in windows (dir_ws: the job's stretch, rawdtw_semi_window.h)
template <int RPL, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_semi_ckpt_wave(const DevJob *__restrict__ jobs, const FullAux *__restrict__ aux,
                                                               const float *__restrict__ ev, const float *__restrict__ ref,
                                                               float *__restrict__ out_cost, uint32_t *__restrict__ out_end_j,
                                                               float *__restrict__ bnd_ws, uint8_t *__restrict__ dir_ws, uint32_t columns)
{
    semi_wave_body<RPL, false, false, WAVES, true>(jobs, aux, ev, ref, out_cost, nullptr, out_end_j, bnd_ws, dir_ws, columns);
}

// The traceback in windows (include/rawdtw.h, "semiglobal, in windows"), one wave per job, behind k_semi_ckpt_wave: as long as i > 0,
// refill the window lo(j) .. j of the current position with directions -- k_semi_wave<., true>'s strip loop (rawdtw_wavefront.h)
// over the window's columns, its column -1 the checkpoint in front of the window (v[], and the diagonal input of each lane's first
// row, which for lane 0 of a strip below the first is the row above the strip), rows down to the strip that holds i only: the walk
// never moves down --, then walk as k_semi_walk_wave does until i == 0 or a step leaves the window on the left (that step is emitted).
// Strips run in sequence on the one wave, also for jobs of the pipelined class; the boundary row between them is the job's own (the
// cost pass is done with it), indexed by the column inside the window.  No spin-wait and no progress word: every round of the outer
// loop takes at least one step of the walk, and a walk has at most n + m - 1 elements.
// Output as k_semi_walk_wave's: (i, j) end-first into tmp_i / tmp_j, the length; k_semi_finish follows unchanged.  stats: windows
// entered over the launch ([0], summed) and by one job at most ([1]).
template <int RPL>
__global__ __launch_bounds__(64) void k_semi_window(const DevJob *__restrict__ jobs, const FullAux *__restrict__ aux,
                                                    const float *__restrict__ ev, const float *__restrict__ ref,
                                                    float *__restrict__ bnd_ws, uint8_t *__restrict__ dir_ws,
                                                    const uint32_t *__restrict__ end_j, const uint64_t *__restrict__ path_off,
                                                    uint32_t *__restrict__ path_len, uint32_t *__restrict__ tmp_i,
                                                    uint32_t *__restrict__ tmp_j, uint32_t columns, unsigned long long *__restrict__ stats)
{
    using word_t = typename wf::DirWord<RPL>::type;
    constexpr uint32_t SPB = wf::SPB<RPL>;
    constexpr float kNone = wf::kNone;
    constexpr uint32_t STRIP = 64u * RPL;
    __shared__ __attribute__((aligned(16))) word_t tbuf[64 * SPB]; // the fill's staging: [lane][step in block]
    __shared__ __attribute__((aligned(16))) word_t row[64 * SPB];  // the walk's block row
    const int lane = threadIdx.x;
    const DevJob jb = jobs[blockIdx.x];
    const FullAux ax = aux[blockIdx.x];
    const float *Y = ev + jb.read_off;
    const float *X = ref + jb.ref_off;
    const uint32_t NY = jb.n, NX = jb.m, C = columns;
    const uint64_t TXB = ((uint64_t)semi_window::width(NX, C) + 63u + SPB - 1) / SPB; // blocks per strip of a window
    uint4 *dirs = reinterpret_cast<uint4 *>(dir_ws + ax.dir_off);
    const float *ckpt = reinterpret_cast<const float *>(dir_ws + ax.dir_off + semi_window::ckpt_off(NY, NX, C, RPL));
    float *bnd = bnd_ws + ax.bnd_off;
    const uint64_t po = path_off[blockIdx.x];
    uint32_t i = NY - 1, j = end_j[jb.aux], k = 1; // step 0: the end cell (lane 0's slot holds it)
    if (j >= NX) j = NX - 1; // (never: the fill wrote a column of the matrix)
    uint32_t bi = i, bj = j;
    uint32_t entered = 0;
    auto flush = [&](uint32_t upto) {
        const uint32_t base = (upto - 1) & ~63u;
        if ((uint32_t)lane <= ((upto - 1) & 63u)) { tmp_i[po + base + lane] = bi; tmp_j[po + base + lane] = bj; }
    };
    while (i > 0) {
        const uint32_t c_lo = semi_window::lo(j, C), wcols = j - c_lo + 1; // wave-uniform
        const float *ck = c_lo ? ckpt + semi_window::ckpt_at(NY, C, c_lo - 1) : nullptr; // column c_lo - 1 of D
        const uint32_t ns = i / STRIP + 1; // strips that hold rows 0 .. i
        entered++;
        // ---- the fill ----
        for (uint32_t s = 0; s < ns; s++) {
            const uint32_t y0 = (s * 64u + lane) * RPL;
            const uint32_t rows_here = (NY - s * STRIP) < STRIP ? (NY - s * STRIP) : STRIP;
            const uint32_t lanes_here = (rows_here + RPL - 1) / RPL;
            const uint32_t steps = wcols + lanes_here - 1;
            const bool has_rows = y0 < NY;
            const bool hands_down = (s + 1 < ns); // then the strip is full and lane 63 owns its last row
            const bool row0 = (s == 0 && lane == 0);
            float yv[RPL], v[RPL];
#pragma unroll
            for (int q = 0; q < RPL; q++) {
                const uint32_t y = y0 + q < NY ? y0 + q : NY - 1;
                yv[q] = Y[y];
                v[q] = ck ? ck[y] : kNone; // column c_lo - 1
            }
            float diag_in = kNone; // D(y0 - 1, c_lo - 1)
            if (ck && y0 > 0) diag_in = ck[y0 - 1 < NY ? y0 - 1 : NY - 1];
            float last_out = kNone, xval = 0.0f, xchunk = 0.0f, bchunk = kNone, wchunk = 0.0f;
            for (uint32_t t = 0; t < steps; t++) {
                if ((t & 63u) == 0) {
                    const uint32_t idx = t + lane;
                    xchunk = X[c_lo + (idx < wcols ? idx : wcols - 1)];
                    if (s > 0) bchunk = idx < wcols ? bnd[idx] : kNone;
                }
                const float x0 = read_lane(xchunk, (int)(t & 63u));
                const float b0 = read_lane(bchunk, (int)(t & 63u));
                const float up_in = wave_shr1(last_out, b0);
                xval = wave_shr1(xval, x0);
                const uint32_t x = t - (uint32_t)lane; // the column inside the window
                if (x < wcols) {
                    float d = diag_in, ab = up_in;
                    uint32_t code = 0;
#pragma unroll
                    for (int q = 0; q < RPL; q++) {
                        const float left = v[q];
                        const float dd = dist(xval, yv[q]);
                        float nv = min3f(ab, left, d) + dd;
                        if (q == 0) nv = row0 ? dd : nv;
                        code = wf::dir_code(code, ab, left, d);
                        d = left; ab = nv; v[q] = nv;
                    }
                    diag_in = up_in;
                    last_out = v[RPL - 1];
                    wf::dir_put<RPL>(tbuf, lane, t, code);
                }
                if ((t % SPB) == SPB - 1 || t + 1 == steps) wf::dir_flush<RPL>(tbuf, dirs, TXB, s, t, lane, has_rows);
                if (hands_down && t >= 63u) {
                    // lane 63 finished column c = t-63 in this step; gather 64 of them, store coalesced
                    const uint32_t c = t - 63u;
                    const float v63 = read_lane(last_out, 63);
                    if ((uint32_t)lane == (c & 63u)) wchunk = v63;
                    if ((c & 63u) == 63u || c == wcols - 1) {
                        const uint32_t base = c & ~63u;
                        if (base + lane <= c) bnd[base + lane] = wchunk;
                    }
                }
            }
            __threadfence(); // the boundary row and the directions are read back by this wave, at addresses it has read before
        }
        // ---- the walk inside the window ----
        uint64_t cur = ~0ull; // (a refilled window has new block rows)
        while (i > 0) {
            if (j == 0) i--; // global column 0 only
            else {
                const wf::WalkPos p = wf::walk_step<RPL, true>({i, j, cur}, dirs, row, TXB, lane, i, j, c_lo);
                i = p.i; j = p.j; cur = p.cur;
            }
            if ((uint32_t)lane == (k & 63u)) { bi = i; bj = j; }
            k++;
            if ((k & 63u) == 0) flush(k);
            if (j < c_lo) break; // the step left the window (never at c_lo == 0)
        }
    }
    if ((k & 63u) != 0) flush(k);
    if (lane == 0) {
        path_len[blockIdx.x] = k;
        atomicAdd(&stats[0], (unsigned long long)entered);
        atomicMax(&stats[1], (unsigned long long)entered);
    }
}

// The walk, one wave per job (rawdtw_wavefront.h): from (n - 1, end_j) until i == 0 (dtw.cpp:709-738; at j == 0 it moves up).
// Output: (i, j) end-first, at most n + m - 1 elements.
template <int RPL>
__global__ __launch_bounds__(64) void k_semi_walk_wave(const DevJob *__restrict__ jobs, const FullAux *__restrict__ aux,
                                                       const uint8_t *__restrict__ dir_ws, const uint32_t *__restrict__ end_j,
                                                       const uint64_t *__restrict__ path_off, uint32_t *__restrict__ path_len,
                                                       uint32_t *__restrict__ tmp_i, uint32_t *__restrict__ tmp_j)
{
    using word_t = typename wf::DirWord<RPL>::type;
    __shared__ __attribute__((aligned(16))) word_t row[64 * wf::SPB<RPL>]; // one block row: [lane][step in block]
    const int lane = threadIdx.x;
    const DevJob jb = jobs[blockIdx.x];
    const FullAux ax = aux[blockIdx.x];
    const uint64_t TXB = wf::strip_blocks<RPL>((uint64_t)jb.m);
    const uint4 *dirs = reinterpret_cast<const uint4 *>(dir_ws + ax.dir_off);
    const uint64_t po = path_off[blockIdx.x];
    uint32_t i = jb.n - 1, j = end_j[jb.aux], k = 1;
    if (j >= jb.m) j = jb.m - 1; // (never: the fill wrote a column of the matrix)
    wf::PathBuf path{tmp_i, tmp_j, po, lane, i, j};
    uint64_t cur = ~0ull;
    while (i > 0) {
        if (j == 0) i--;
        else {
            const wf::WalkPos p = wf::walk_step<RPL, false>({i, j, cur}, dirs, row, TXB, lane, i, j);
            i = p.i; j = p.j; cur = p.cur;
        }
        k = path.push(k, i, j);
    }
    path.finish(k);
    if (lane == 0) path_len[blockIdx.x] = k;
}

// k_tb_finish, and the column j0 the path starts in
__global__ __launch_bounds__(256) void k_semi_finish(const DevJob *__restrict__ jobs, uint32_t count, const float *__restrict__ ev,
                                                     const float *__restrict__ ref, const uint64_t *__restrict__ path_off,
                                                     const uint32_t *__restrict__ path_len, const uint32_t *__restrict__ tmp_i,
                                                     const uint32_t *__restrict__ tmp_j, uint32_t *__restrict__ path_j0,
                                                     uint8_t *__restrict__ path_mv, float *__restrict__ path_d)
{
    wf::finish_body<true>(jobs, count, ev, ref, path_off, path_len, tmp_i, tmp_j, path_j0, path_mv, path_d);
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
hipError_t launch_semi_wave(int cls, bool tb, const DevJob *jobs, uint64_t count, const FullAux *aux, const float *ev,
                            const float *ref, float *out_cost, uint32_t *out_end_j, float *bnd_ws, uint8_t *dir_ws, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    return with_wave_class(cls, [&](auto rpl, auto waves) {
        constexpr int RPL = decltype(rpl)::value, WAVES = decltype(waves)::value;
        const auto kern = tb ? k_semi_wave<RPL, true, WAVES> : k_semi_wave<RPL, false, WAVES>;
        hipLaunchKernelGGL(kern, dim3((uint32_t)count), dim3(64 * WAVES), 0, s,
                           jobs, aux, ev, ref, out_cost, out_end_j, bnd_ws, dir_ws);
        return hipGetLastError();
    });
}

hipError_t launch_semi_span_wave(int cls, const DevJob *jobs, uint64_t count, const FullAux *aux, const float *ev, const float *ref,
                                 float *out_cost, uint32_t *out_j0, uint32_t *out_end_j, float *bnd_ws, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    return with_wave_class(cls, [&](auto rpl, auto waves) {
        constexpr int RPL = decltype(rpl)::value, WAVES = decltype(waves)::value;
        hipLaunchKernelGGL((k_semi_span_wave<RPL, WAVES>), dim3((uint32_t)count), dim3(64 * WAVES), 0, s, jobs, aux, ev, ref, out_cost,
                           out_j0, out_end_j, bnd_ws);
        return hipGetLastError();
    });
}

hipError_t launch_semi_ckpt_wave(int cls, const DevJob *jobs, uint64_t count, const FullAux *aux, const float *ev, const float *ref,
                                 float *out_cost, uint32_t *out_end_j, float *bnd_ws, uint8_t *dir_ws, uint32_t columns, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    return with_wave_class(cls, [&](auto rpl, auto waves) {
        constexpr int RPL = decltype(rpl)::value, WAVES = decltype(waves)::value;
        hipLaunchKernelGGL((k_semi_ckpt_wave<RPL, WAVES>), dim3((uint32_t)count), dim3(64 * WAVES), 0, s, jobs, aux, ev, ref, out_cost,
                           out_end_j, bnd_ws, dir_ws, columns);
        return hipGetLastError();
    });
}

// k_semi_finish behind a walk: start-first steps, distances and j0
static hipError_t launch_semi_finish(hipError_t walk, const DevJob *jobs, uint64_t count, const float *ev, const float *ref,
                                     const uint64_t *path_off, const uint32_t *path_len, const uint32_t *tmp_i, const uint32_t *tmp_j,
                                     uint32_t *path_j0, uint8_t *path_mv, float *path_d, hipStream_t s)
{
    if (walk != hipSuccess) return walk;
    hipLaunchKernelGGL(k_semi_finish, dim3((uint32_t)count), dim3(256), 0, s, jobs, (uint32_t)count, ev, ref, path_off, path_len, tmp_i, tmp_j,
                       path_j0, path_mv, path_d);
    return hipGetLastError();
}

hipError_t launch_semi_window(int cls, const DevJob *jobs, uint64_t count, const FullAux *aux, const float *ev, const float *ref,
                              float *bnd_ws, uint8_t *dir_ws, const uint32_t *end_j, const uint64_t *path_off, uint32_t *path_len,
                              uint32_t *path_j0, uint32_t *tmp_i, uint32_t *tmp_j, uint8_t *path_mv, float *path_d, uint32_t columns,
                              unsigned long long *stats, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    const hipError_t e = with_wave_rows(cls, [&](auto rpl) {
        hipLaunchKernelGGL(k_semi_window<decltype(rpl)::value>, dim3((uint32_t)count), dim3(64), 0, s, jobs, aux, ev, ref, bnd_ws, dir_ws, end_j,
                           path_off, path_len, tmp_i, tmp_j, columns, stats);
        return hipGetLastError();
    });
    return launch_semi_finish(e, jobs, count, ev, ref, path_off, path_len, tmp_i, tmp_j, path_j0, path_mv, path_d, s);
}

hipError_t launch_semi_walk(int cls, const DevJob *jobs, uint64_t count, const FullAux *aux, const float *ev, const float *ref,
                            const uint8_t *dir_ws, const uint32_t *end_j, const uint64_t *path_off, uint32_t *path_len,
                            uint32_t *path_j0, uint32_t *tmp_i, uint32_t *tmp_j, uint8_t *path_mv, float *path_d, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    const hipError_t e = with_wave_rows(cls, [&](auto rpl) {
        hipLaunchKernelGGL(k_semi_walk_wave<decltype(rpl)::value>, dim3((uint32_t)count), dim3(64), 0, s, jobs, aux, dir_ws, end_j, path_off,
                           path_len, tmp_i, tmp_j);
        return hipGetLastError();
    });
    return launch_semi_finish(e, jobs, count, ev, ref, path_off, path_len, tmp_i, tmp_j, path_j0, path_mv, path_d, s);
}

} // namespace rawdtw
