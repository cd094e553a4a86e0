// rawdtw_band_tb.hip -- the banded global traceback (include/rawdtw.h, "banded traceback"): the matrix of
// DTW_global_slantedbanded_antidiagonalwise (src/dtw.cpp:273-520) filled with the walk's directions beside it, and DTW_global_tb's walk
// (dtw.cpp:625-647) over them.
//
//   k_band_tb_fill : the recurrence with k_band_wave's geometry (three rotating antidiagonals in LDS, the reference's physical slots and
//                    guarded reads), one workgroup a job; every slot of an antidiagonal that is no cell of S is written as 1e10, so a
//                    neighbour outside S reads 1e10 whatever the slot held three antidiagonals ago.  A wave takes 64 slots at a time
//                    and hands their 2-bit codes out as two ballots: one 16-byte store a wave and chunk (rawdtw_band_tb.h).
//   k_band_tb_walk : one wave a job, all lanes in lockstep on uniform values; the records of 64 antidiagonals and 128 slots of their
//                    rows around the path are fetched together into LDS (a path moves at most one slot an antidiagonal), steps are
//                    buffered one a lane and leave as 64-step stores, as in k_tb_walk_wave.  k_tb_finish follows.
#include "rawdtw_band_tb.h"
#include "rawdtw_dp.h"

namespace rawdtw {

__global__ __launch_bounds__(256) void k_band_tb_fill(const DevJob *__restrict__ jobs, const FullAux *__restrict__ aux,
                                                      const float *__restrict__ ev, const float *__restrict__ ref,
                                                      float *__restrict__ out, uint8_t *__restrict__ dir_ws)
{
    extern __shared__ float lds[];
    const DevJob jb = jobs[blockIdx.x];
    const FullAux ax = aux[blockIdx.x];
    const int tid = threadIdx.x, nt = blockDim.x;
    const float *A = ev + jb.read_off;
    const float *B = ref + jb.ref_off;
    uint32_t N = jb.n, M = jb.m;
    const bool swapped = N < M; // dtw.cpp:284-292: A is the longer one; the codes stay in the caller's i (a) and j (b)
    if (swapped) {
        const float *tp = A; A = B; B = tp;
        uint32_t tn = N; N = M; M = tn;
    }
    const int R = jb.R;
    const int P = R + ((R % 2 == 0) ? 1 : 0);
    const int S = R + ((R % 2 == 1) ? 1 : 0);
    const int K = P > S ? P : S;
    const int SH = P > S ? 0 : 1;
    const int Kpad = (K + 63) & ~63;
    const uint32_t chunks = (uint32_t)Kpad >> 6;
    BandTbRec *recs = reinterpret_cast<BandTbRec *>(dir_ws + ax.dir_off);
    uint4 *rows = reinterpret_cast<uint4 *>(dir_ws + ax.dir_off + ((uint64_t)N + M - 1) * sizeof(BandTbRec));
    float *d0 = lds, *d1 = lds + K, *d2 = lds + 2 * K;
    for (int x = tid; x < 3 * K; x += nt) lds[x] = kInf;
    __syncthreads();
    if (tid == 0) {
        d1[P / 2 + SH] = dist(A[0], B[0]);
        recs[0] = BandTbRec{P / 2 + SH, -(P / 2 + SH), P / 2 + SH, P / 2 + SH + 1}; // column 0: the corner alone (dtw.cpp:317-347)
    }
    __syncthreads();

    int row = 0;
    uint32_t rem = 0;
    int prev_adv = 0;
    for (uint32_t col = 1; col < N; col++) {
        rem += M;
        const int adv = rem >= N;
        if (adv) { rem -= N; row++; }
        for (int pass = adv ? 0 : 1; pass < 2; pass++) {
            const int len = pass == 0 ? S : P;
            const int si = pass == 0 ? (int)col + S / 2 - 1 : (int)col + P / 2;
            const int sj = pass == 0 ? row - S / 2 : row - P / 2;
            int lo = 0, hi = len;
            if (si - (int)N + 1 > lo) lo = si - (int)N + 1;
            if (-sj > lo) lo = -sj;
            if (si + 1 < hi) hi = si + 1;
            if ((int)M - sj < hi) hi = (int)M - sj;
            // neighbour rule of this antidiagonal kind (k_band_wave; dtw.cpp:368-485)
            int dt, dtl, dl, ds, g_top_first, g_tl_first, g_left_last;
            if (SH == 0) {
                if (pass == 0) { dt = 0; dtl = 0; dl = 1; ds = 0; g_top_first = 0; g_tl_first = 0; g_left_last = 0; }
                else if (adv)  { dt = -1; dtl = 0; dl = 0; ds = 0; g_top_first = 1; g_tl_first = 0; g_left_last = 1; }
                else           { dt = -1; dtl = -1; dl = 0; ds = 0; g_top_first = 1; g_tl_first = 1; g_left_last = 0; }
            } else {
                if (pass == 0) { dt = 0; dtl = 0; dl = 1; ds = 0; g_top_first = 1; g_tl_first = !prev_adv; g_left_last = 1; }
                else if (adv)  { dt = 0; dtl = 1; dl = 1; ds = 1; g_top_first = 0; g_tl_first = 0; g_left_last = 0; }
                else           { dt = 0; dtl = 0; dl = 1; ds = 1; g_top_first = 1; g_tl_first = !prev_adv; g_left_last = 0; }
            }
            const uint32_t s = (uint32_t)(si + sj); // = I + J of every cell of this antidiagonal
            // (the record speaks of SLOTS x = o + ds: slot x is the cell (si + ds - x, sj - ds + x))
            if (tid == 0) recs[s] = BandTbRec{si + ds, sj - ds, lo + ds, hi + ds};
            uint4 *rowp = rows + (uint64_t)s * chunks;
            for (int x = tid; x < Kpad; x += nt) { // (whole waves: Kpad and nt are multiples of 64)
                const int o = x - ds;
                float v = kInf;
                uint32_t code = 0;
                if (o >= lo && o < hi) {
                    const bool first = (o == 0), last = (o == len - 1);
                    const float top = (g_top_first && first) ? kInf : d1[o + dt];   // (I, J - 1)
                    const float tl = (g_tl_first && first) ? kInf : d0[o + dtl];    // (I - 1, J - 1)
                    const float left = (g_left_last && last) ? kInf : d1[o + dl];   // (I - 1, J)
                    v = min3f(top, left, tl) + dist(A[si - o], B[sj + o]);
                    // the walk's rule on the caller's names (dtw.cpp:633-646): L = (i - 1, j), T = (i, j - 1)
                    const float L = swapped ? top : left, T = swapped ? left : top;
                    const float m_t = tl < T ? tl : T, m_l = tl < L ? tl : L;
                    code = L < m_t ? 1u : (T < m_l ? 2u : 0u);
                }
                if (x < K) d2[x] = v;
                const unsigned long long b0 = __ballot(code & 1u), b1 = __ballot(code & 2u);
                if ((tid & 63) == 0)
                    rowp[x >> 6] = make_uint4((uint32_t)b0, (uint32_t)(b0 >> 32), (uint32_t)b1, (uint32_t)(b1 >> 32));
            }
            __syncthreads();
            float *t = d0; d0 = d1; d1 = d2; d2 = t;
        }
        prev_adv = adv;
    }
    if (tid == 0) {
        float res = d1[P / 2 + SH];
        if (jb.flags & kFlagExcludeLast) res = res - dist(A[N - 1], B[M - 1]);
        out[jb.aux] = res;
    }
}

__global__ __launch_bounds__(64) void k_band_tb_walk(const DevJob *__restrict__ jobs, const FullAux *__restrict__ aux,
                                                     const uint8_t *__restrict__ dir_ws, const uint64_t *__restrict__ path_off,
                                                     uint32_t *__restrict__ path_len, uint32_t *__restrict__ tmp_i,
                                                     uint32_t *__restrict__ tmp_j)
{
    __shared__ BandTbRec srec[64];                              // records of antidiagonals rec_s, rec_s - 1, ..
    __shared__ __attribute__((aligned(16))) uint4 srow[64][2];  // chunks row_c, row_c + 1 of rows row_s, row_s - 1, ..
    const int lane = threadIdx.x;
    const DevJob jb = jobs[blockIdx.x];
    const FullAux ax = aux[blockIdx.x];
    const bool swapped = jb.n < jb.m;
    const uint32_t K = (uint32_t)jb.R + 1u, chunks = (K + 63u) >> 6;
    const BandTbRec *recs = reinterpret_cast<const BandTbRec *>(dir_ws + ax.dir_off);
    const uint4 *rows = reinterpret_cast<const uint4 *>(dir_ws + ax.dir_off + ((uint64_t)jb.n + jb.m - 1) * sizeof(BandTbRec));
    const uint64_t po = path_off[blockIdx.x];
    uint32_t i = jb.n - 1, j = jb.m - 1, k = 0;
    uint32_t bi = 0, bj = 0; // this lane's slot of the 64-step output buffer (lane = step & 63)
    int rec_s = -1, row_s = -1, row_c = 0;
    bool no_path = false;
    auto flush = [&](uint32_t upto) { // steps [upto - ((upto - 1) & 63) - 1 .. upto) sit in lanes 0..(upto-1)&63
        const uint32_t base = (upto - 1) & ~63u;
        if ((uint32_t)lane <= ((upto - 1) & 63u)) { tmp_i[po + base + lane] = bi; tmp_j[po + base + lane] = bj; }
    };
    for (;;) {
        const int I = (int)(swapped ? j : i);
        const int s = (int)(i + j);
        if (s > rec_s || rec_s - s >= 64) { // (uniform: every lane takes the same branches throughout)
            __syncthreads();
            rec_s = s;
            if (s - lane >= 0) srec[lane] = recs[s - lane];
            __syncthreads();
        }
        const BandTbRec rc = srec[rec_s - s];
        const int x = __builtin_amdgcn_readfirstlane(rc.si - I);
        const int lo = __builtin_amdgcn_readfirstlane(rc.lo), hi = __builtin_amdgcn_readfirstlane(rc.hi);
        if (x < lo || x >= hi) { no_path = true; break; } // the walk left S: no path (only where sums reach 1e10)
        if ((uint32_t)lane == (k & 63u)) { bi = i; bj = j; }
        k++;
        if ((k & 63u) == 0) flush(k);
        if (i == 0 && j == 0) break;
        if (i == 0) j--;
        else if (j == 0) i--;
        else {
            if (s > row_s || row_s - s >= 64 || x < 64 * row_c || x >= 64 * row_c + 128) {
                __syncthreads();
                row_s = s;
                row_c = x >= 32 ? (x - 32) >> 6 : 0; // (x < K: chunk row_c exists; row_c + 1 may not)
                if (s - lane >= 0) {
                    const uint4 *rp = rows + (uint64_t)(s - lane) * chunks + (uint32_t)row_c;
                    srow[lane][0] = rp[0];
                    srow[lane][1] = (uint32_t)row_c + 1u < chunks ? rp[1] : make_uint4(0u, 0u, 0u, 0u);
                }
                __syncthreads();
            }
            const int xx = x - 64 * row_c;
            const uint4 q = srow[row_s - s][xx >> 6];
            const uint32_t p0 = (xx & 32) ? q.y : q.x, p1 = (xx & 32) ? q.w : q.z;
            const uint32_t code = (uint32_t)__builtin_amdgcn_readfirstlane((int)(((p0 >> (xx & 31)) & 1u) | (((p1 >> (xx & 31)) & 1u) << 1)));
            if (code == 1u) i--;
            else if (code == 2u) j--;
            else { i--; j--; }
        }
    }
    if (no_path) k = 0;
    else if ((k & 63u) != 0) flush(k);
    if (lane == 0) path_len[blockIdx.x] = k;
}

hipError_t launch_band_tb_fill(const DevJob *jobs, uint64_t count, const FullAux *aux, uint32_t threads, uint32_t lds_floats, const float *ev,
                               const float *ref, float *out_cost, uint8_t *dir_ws, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    const size_t lds_bytes = (size_t)lds_floats * sizeof(float);
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_band_tb_fill), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_band_tb_fill, dim3((uint32_t)count), dim3(threads), lds_bytes, s, jobs, aux, ev, ref, out_cost, dir_ws);
    return hipGetLastError();
}

hipError_t launch_band_tb_walk(const DevJob *jobs, uint64_t count, const FullAux *aux, const uint8_t *dir_ws, const uint64_t *path_off,
                               uint32_t *path_len, uint32_t *tmp_i, uint32_t *tmp_j, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_band_tb_walk, dim3((uint32_t)count), dim3(64), 0, s, jobs, aux, dir_ws, path_off, path_len, tmp_i, tmp_j);
    return hipGetLastError();
}

} // namespace rawdtw
