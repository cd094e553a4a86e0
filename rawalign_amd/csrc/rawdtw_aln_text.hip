// rawdtw_aln_text.hip -- the aln:s: text of paths made on the device (include/rawdtw.h, "aln text"): count, scan, write, as the seeding
// does it.  One wave a path.  A tile is the wave's 64 elements: a lane reads its element's step byte and distance, the walk's (pi, pj)
// comes from a wave scan of the step bits on top of what the tiles before carried, the element is formatted by the shared formatter
// (rawdtw_fmt_g.h: the %g text in two registers, no local array) and the tile's byte count from a wave scan of the lengths.
//   k_aln_count  the bytes of each path's text, stored at the path's JOB (a traceback sub-batch's paths are in plan order)
//   k_aln_scan   one workgroup: the exclusive sums of the totals, n + 1 of them
//   k_aln_write  formats again; a lane writes its element into an LDS staging area at its scanned byte offset -- the area is laid so
//                that LDS address and global address agree mod 16 --, then the wave streams the area out: bytes up to the first
//                16-byte boundary, 16-byte stores, bytes behind the last one.  It writes text[text_off[job] .. + total) and nothing else.
// All offsets are 64-bit.  Formatting twice costs less than a fixed-stride scratch of 56 bytes an element would.
#include "rawdtw_aln_text.h"
#include "rawdtw_fmt_g.h"

namespace rawdtw {
namespace {

constexpr uint32_t kElemMax = 56;                          // "(" 20 "," 20 "," 12 ")"
constexpr uint32_t kStageVec = (15 + 64 * kElemMax + 15) / 16; // a tile's text behind up to 15 bytes of alignment, in 16-byte words

__device__ inline uint32_t wave_scan_u32(uint32_t v, uint32_t lane) // inclusive
{
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

__device__ inline uint64_t wave_scan_u64(uint64_t v, uint32_t lane) // inclusive
{
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
        if (lane >= o) v += (uint64_t)hi << 32 | lo;
    }
    return v;
}

template <bool kWrite>
__global__ __launch_bounds__(64) void k_aln_text(const uint8_t *__restrict__ step, const float *__restrict__ dist, const uint64_t *__restrict__ poff,
                                                 const uint32_t *__restrict__ plen, const capi::AlnDevRec *__restrict__ recs,
                                                 uint64_t *__restrict__ totals, const uint64_t *__restrict__ text_off, char *__restrict__ text)
{
    __shared__ uint4 stage[kWrite ? kStageVec : 1];
    const uint64_t p = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const capi::AlnDevRec rc = recs[p];
    uint32_t len = plen[p];
    if ((rc.flags & 0x100u) && len) len--;
    const uint64_t base = poff[p];
    const uint32_t mode = rc.flags & 1u;
    uint64_t pi = 0, pj = rc.j0, bytes = 0;
    char *const out = kWrite ? text + text_off[rc.job] : nullptr;
    for (uint32_t q0 = 0; q0 < len; q0 += 64) {
        const uint32_t q = q0 + lane;
        const bool act = q < len;
        const uint32_t st = act ? step[base + q] : 0u;
        const uint32_t bits = act ? __float_as_uint(dist[base + q]) : 0u;
        // i's steps in the low half, j's in the high half: a tile has at most 64 of each
        const uint32_t adv = wave_scan_u32((st & 1u) | ((st >> 1) & 1u) << 16, lane);
        uint64_t i, j;
        fmtg::elem_ij(rc.off_i, rc.off_j, mode, pi + (adv & 0xffffu), pj + (adv >> 16), q, len, i, j);
        const fmtg::Text g = fmtg::fmt_g(bits);
        const uint32_t mine = act ? fmtg::elem_len(i, j, g) : 0u;
        const uint32_t incl = wave_scan_u32(mine, lane);
        const uint32_t tile_bytes = __shfl(incl, 63, 64), tile_adv = __shfl(adv, 63, 64);
        if (kWrite) {
            char *const g0 = out + bytes;
            const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(g0) & 15u);
            char *const sb = reinterpret_cast<char *>(stage);
            if (act) (void)fmtg::elem_put(sb + a + (incl - mine), i, j, g);
            __syncthreads();
            const uint32_t head = min(tile_bytes, (16u - a) & 15u);
            for (uint32_t k = lane; k < head; k += 64) g0[k] = sb[a + k];
            const uint32_t nvec = (tile_bytes - head) >> 4, v0 = (a + head) >> 4; // (a + head is a multiple of 16 wherever nvec > 0)
            uint4 *const gv = reinterpret_cast<uint4 *>(g0 + head);
            for (uint32_t k = lane; k < nvec; k += 64) gv[k] = stage[v0 + k];
            for (uint32_t k = head + (nvec << 4) + lane; k < tile_bytes; k += 64) g0[k] = sb[a + k];
            __syncthreads(); // (the next tile's elements go into the same area)
        }
        pi += tile_adv & 0xffffu; pj += tile_adv >> 16; bytes += tile_bytes;
    }
    if (!kWrite && lane == 0) totals[rc.job] = bytes;
}

__global__ __launch_bounds__(256) void k_aln_scan(const uint64_t *__restrict__ totals, uint64_t n, uint64_t *__restrict__ text_off)
{
    __shared__ uint64_t wave_sum[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t carry = 0;
    for (uint64_t b = 0; b < n; b += 256) {
        const uint64_t k = b + tid;
        const uint64_t v = k < n ? totals[k] : 0;
        uint64_t incl = wave_scan_u64(v, lane);
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        uint64_t all = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
            if (w < wave) incl += wave_sum[w];
            all += wave_sum[w];
        }
        if (k < n) text_off[k] = carry + incl - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) text_off[n] = carry;
}

} // namespace

namespace capi {

hipError_t launch_aln_count(const uint8_t *step, const float *d, const uint64_t *poff, const uint32_t *plen, const AlnDevRec *recs, uint64_t n,
                            uint64_t *totals, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_aln_text<false>, dim3((uint32_t)n), dim3(64), 0, s, step, d, poff, plen, recs, totals, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_aln_scan(const uint64_t *totals, uint64_t n, uint64_t *text_off, hipStream_t s)
{
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_aln_scan, dim3(1), dim3(256), 0, s, totals, n, text_off);
    return hipGetLastError();
}

hipError_t launch_aln_write(const uint8_t *step, const float *d, const uint64_t *poff, const uint32_t *plen, const AlnDevRec *recs, uint64_t n,
                            const uint64_t *text_off, char *text, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_aln_text<true>, dim3((uint32_t)n), dim3(64), 0, s, step, d, poff, plen, recs, nullptr, text_off, text);
    return hipGetLastError();
}

} // namespace capi
} // namespace rawdtw

using namespace rawdtw;
using namespace rawdtw::capi;

extern "C" {

int rawdtw_aln_text_steps(rawdtw_ctx *ctx, const uint8_t *path_step, const float *path_d, const uint64_t *path_off, const uint32_t *path_len,
                          const rawdtw_aln_rec_t *recs, uint64_t n_jobs, uint64_t *text_off, char *text, uint64_t text_cap, uint64_t *text_bytes)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!text_off || !text_bytes || (n_jobs && (!path_step || !path_d || !path_off || !path_len || !recs))) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n_jobs >= (1ull << 31)) return fail(ctx, RAWDTW_ERR_INVALID, "more jobs than one launch has workgroups");
    uint64_t extent = 0;
    for (uint64_t k = 0; k < n_jobs; k++) {
        if (recs[k].mode > 1) return fail(ctx, RAWDTW_ERR_INVALID, "a rec's mode is neither 0 nor 1");
        if (path_len[k]) extent = std::max(extent, path_off[k] + path_len[k]);
    }
    ctx->aln_count_ms = ctx->aln_write_ms = 0.f; ctx->aln_text_bytes = 0;
    text_off[0] = 0; *text_bytes = 0;
    if (n_jobs == 0) return RAWDTW_OK;
    std::vector<AlnDevRec> hrec(n_jobs);
    for (uint64_t k = 0; k < n_jobs; k++) hrec[k] = aln_dev_rec(recs[k], false, k);
    DevBlock blk(ctx, "aln text"), txt(ctx, "aln text");
    const size_t need = al256(extent) + al256(extent * 4) + al256(n_jobs * 8) + al256(n_jobs * 4) + al256(n_jobs * 32) + al256(n_jobs * 8) + al256((n_jobs + 1) * 8);
    if (int st = blk.reserve(need)) return st;
    char *pb = blk.p;
    uint8_t *d_step = carve<uint8_t>(pb, extent);
    float *d_d = carve<float>(pb, extent);
    uint64_t *d_poff = carve<uint64_t>(pb, n_jobs);
    uint32_t *d_plen = carve<uint32_t>(pb, n_jobs);
    AlnDevRec *d_rec = carve<AlnDevRec>(pb, n_jobs);
    uint64_t *d_tot = carve<uint64_t>(pb, n_jobs);
    uint64_t *d_toff = carve<uint64_t>(pb, n_jobs + 1);
    EventPair ev, ev2; // count + scan: ev.e[0] .. ev.e[1]; write: ev2.e[0] .. ev2.e[1]
    for (int k = 0; k < 2; k++) { HIP_TRY(ctx, hipEventCreate(&ev.e[k])); HIP_TRY(ctx, hipEventCreate(&ev2.e[k])); }
    if (extent) {
        HIP_TRY(ctx, hipMemcpyAsync(d_step, path_step, extent, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_d, path_d, extent * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_poff, path_off, n_jobs * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_plen, path_len, n_jobs * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_rec, hrec.data(), n_jobs * sizeof(AlnDevRec), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ev.e[0], ctx->stream));
    HIP_TRY(ctx, launch_aln_count(d_step, d_d, d_poff, d_plen, d_rec, n_jobs, d_tot, ctx->stream));
    HIP_TRY(ctx, launch_aln_scan(d_tot, n_jobs, d_toff, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ev.e[1], ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(text_off, d_toff, (n_jobs + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipEventElapsedTime(&ctx->aln_count_ms, ev.e[0], ev.e[1]);
    const uint64_t total = text_off[n_jobs];
    *text_bytes = total; ctx->aln_text_bytes = total;
    if (!text || total == 0) return RAWDTW_OK;
    if (text_cap < total) return fail(ctx, RAWDTW_ERR_RANGE, "text_cap is below the text's size");
    if (int st = txt.reserve(total)) return st;
    HIP_TRY(ctx, hipEventRecord(ev2.e[0], ctx->stream));
    HIP_TRY(ctx, launch_aln_write(d_step, d_d, d_poff, d_plen, d_rec, n_jobs, d_toff, txt.p, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ev2.e[1], ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(text, txt.p, total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipEventElapsedTime(&ctx->aln_write_ms, ev2.e[0], ev2.e[1]);
    return RAWDTW_OK;
}

int rawdtw_aln_text_timing(const rawdtw_ctx *ctx, float *count_ms, float *write_ms, uint64_t *text_bytes)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (count_ms) *count_ms = ctx->aln_count_ms;
    if (write_ms) *write_ms = ctx->aln_write_ms;
    if (text_bytes) *text_bytes = ctx->aln_text_bytes;
    return RAWDTW_OK;
}

} // extern "C"
