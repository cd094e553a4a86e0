// rawdtw_refsig.hip -- the reference arena from bases on the device: ri_seq_to_sig (src/rsig.cpp:7-41) for both strands of every
// sequence as rawindex.cpp:132-149 calls it (forward = strand 1), bit-equal to the host restatement (rawdtw_refsig_host.cpp) and so
// to the reference, in the plain and the contracted form.
//
//   k_refsig_sums   a wave per (sequence, strand).  The lanes form the k-mers of 64 output elements and look their levels up (the
//                   model in LDS up to k = 6, in global memory above); kStepsAhead such loads are in flight before the wave advances
//                   sum and sum2 through them, a step (rawdtw_refsig.h) each, the next group's loads under way: one integer
//                   reduction (both sums' together) where the step is exact that way, else 64 dependent additions every lane
//                   performs alike out of LDS.  Lane 0 then leaves mean and std_dev.
//   k_refsig_write  a thread an output element: its k-mer again from k bases, the level, (float)(((double)v - mean) / std_dev)
//                   straight into the arena.
// The bases cross as they are through two pinned staging buffers; seq_nt4_table is applied on the device.  The new arena is
// installed only behind a build that succeeded.
#include "rawdtw_capi.h"
#include "rawdtw_refsig.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace rawdtw {
namespace {

using namespace refsig;

// the wave's sums of two values at once: the two chains of shuffles overlap
__device__ inline void wave_sum2(uint64_t &a, uint64_t &b)
{
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t ta = (uint64_t)__shfl_xor((unsigned long long)a, o, 64), tb = (uint64_t)__shfl_xor((unsigned long long)b, o, 64);
        a += ta; b += tb;
    }
}

// 64 dependent additions in emission order, alike in every lane (the block is this one wave; every branch here is wave-uniform)
__device__ inline double slow_step(double s, double x, uint32_t lane, uint32_t n, double *slow_x)
{
    __syncthreads();
    slow_x[lane] = x;
    __syncthreads();
    for (uint32_t t = 0; t < n; t++) s += slow_x[t];
    return s;
}

// one step of both running sums, which the wave holds uniformly: lane t < n carries addend t of each.  fast1 / fast2: which went fast.
__device__ inline void wave_step2(double &s1, double &s2, double x1, double x2, uint32_t lane, uint32_t n, double *slow_x, bool &fast1, bool &fast2)
{
    const uint64_t b1 = bits_of(s1), b2 = bits_of(s2);
    uint64_t d1 = 0, d2 = 0, n1 = 0, n2 = 0;
    bool ok1 = sum_fast_ready(b1), ok2 = sum_fast_ready(b2);
    if (ok1 && lane < n) ok1 = sum_addend_units(b1, x1, &d1);
    if (ok2 && lane < n) ok2 = sum_addend_units(b2, x2, &d2);
    ok1 = __all(ok1); ok2 = __all(ok2);
    if (lane >= n || !ok1) d1 = 0;
    if (lane >= n || !ok2) d2 = 0;
    if (ok1 || ok2) wave_sum2(d1, d2);
    fast1 = ok1 && sum_fast_finish(b1, d1, &n1);
    fast2 = ok2 && sum_fast_finish(b2, d2, &n2);
    s1 = fast1 ? double_of(n1) : slow_step(s1, x1, lane, n, slow_x);
    s2 = fast2 ? double_of(n2) : slow_step(s2, x2, lane, n, slow_x);
}

__global__ __launch_bounds__(64) void k_refsig_sums(const uint8_t *__restrict__ bases, const SeqRow *__restrict__ table, const float *__restrict__ model,
                                                    uint32_t k, int model_in_lds, int contracted, StrandSums *__restrict__ sums,
                                                    StrandSteps *__restrict__ steps)
{
    extern __shared__ float lds_model[];
    __shared__ double slow_x[kStep];
    const uint32_t pair = blockIdx.x, lane = threadIdx.x;
    const SeqRow row = table[pair >> 1];
    const int strand = (pair & 1) ? 0 : 1; // (forward first, rawindex.cpp:141-147)
    const uint32_t n = row.s_len;
    if (n == 0) {
        if (lane == 0) { sums[pair] = StrandSums{0, 0, 0, 0}; steps[pair] = StrandSteps{{0, 0}, {0, 0}}; }
        return;
    }
    const float *lv = model;
    if (model_in_lds) {
        for (uint32_t i = lane; i < (1u << (2 * k)); i += kStep) lds_model[i] = model[i];
        __syncthreads();
        lv = lds_model;
    }
    const uint8_t *b = bases + row.base_off;
    double sum = 0, sum2 = 0;
    uint64_t fast1 = 0, fast2 = 0, slow1 = 0, slow2 = 0;
    // the levels of kStepsAhead steps are loaded a group ahead: the next group's loads are in flight while this group's steps run
    auto load = [&](uint64_t j0, float *v) {
#pragma unroll
        for (uint32_t a = 0; a < kStepsAhead; a++) {
            const uint64_t j = j0 + a * kStep + lane;
            v[a] = j < n ? lv[kmer_of(b, row.len, k, strand, (uint32_t)j)] : 0.0f;
        }
    };
    float v[kStepsAhead], nxt[kStepsAhead];
    load(0, nxt);
    for (uint64_t j0 = 0; j0 < n; j0 += (uint64_t)kStep * kStepsAhead) {
#pragma unroll
        for (uint32_t a = 0; a < kStepsAhead; a++) v[a] = nxt[a];
        load(j0 + (uint64_t)kStep * kStepsAhead, nxt); // (beyond n: zeros, no load)
#pragma unroll
        for (uint32_t a = 0; a < kStepsAhead; a++) {
            const uint64_t at = j0 + a * kStep;
            if (at >= n) break;
            const uint32_t c = (uint32_t)(n - at < kStep ? n - at : kStep);
            const double x = (double)v[a];
            bool f1, f2;
            wave_step2(sum, sum2, x, x * x, lane, c, slow_x, f1, f2); // (the product of two floats is exact in double)
            if (f1) fast1++; else slow1++;
            if (f2) fast2++; else slow2++;
        }
    }
    if (lane == 0) {
        StrandSums o;
        o.sum = sum; o.sum2 = sum2;
        mean_std(sum, sum2, n, contracted, &o.mean, &o.std_dev);
        sums[pair] = o;
        steps[pair] = StrandSteps{{fast1, fast2}, {slow1, slow2}};
    }
}

__global__ __launch_bounds__(256) void k_refsig_write(const uint8_t *__restrict__ bases, const SeqRow *__restrict__ table, const float *__restrict__ model,
                                                      uint32_t k, const StrandSums *__restrict__ sums, float *__restrict__ arena)
{
    const uint32_t pair = blockIdx.x;
    const SeqRow row = table[pair >> 1];
    const int strand = (pair & 1) ? 0 : 1;
    const uint32_t n = row.s_len;
    const double mean = sums[pair].mean, std_dev = sums[pair].std_dev;
    const uint8_t *b = bases + row.base_off;
    float *out = arena + (strand ? row.arena_fwd : row.arena_rev);
    for (uint64_t j = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.y * blockDim.x)
        out[j] = normalised(model[kmer_of(b, row.len, k, strand, (uint32_t)j)], mean, std_dev);
}

} // namespace
} // namespace rawdtw

using namespace rawdtw;
using namespace rawdtw::capi;
using namespace rawdtw::refsig;

extern "C" {

int rawdtw_reference_from_bases(rawdtw_ctx *ctx, uint32_t n_seq, const char *const *bases, const uint64_t *len, const float *pore_vals, uint32_t k,
                                int contracted)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!pore_vals || (n_seq && (!bases || !len))) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (k < 1 || k > kMaxK) return fail(ctx, RAWDTW_ERR_INVALID, "k is 1 .. 12");
    if (n_seq >= (1u << 30)) return fail(ctx, RAWDTW_ERR_INVALID, "too many sequences");
    uint64_t total_bases = 0, total = 0, max_s_len = 0;
    std::vector<SeqRow> table;
    std::vector<uint64_t> ref_off;
    std::vector<uint32_t> ref_len;
    try {
        table.resize(n_seq); ref_off.assign(2ull * n_seq, 0); ref_len.resize(n_seq);
    } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    for (uint32_t s = 0; s < n_seq; s++) {
        if (len[s] >= (1ull << 31)) return fail(ctx, RAWDTW_ERR_INVALID, "a sequence of 2^31 bases or more");
        if (len[s] && !bases[s]) return fail(ctx, RAWDTW_ERR_INVALID, "null sequence");
        const uint32_t s_len = len[s] >= k ? (uint32_t)len[s] - k + 1 : 0;
        const uint64_t padded = ((uint64_t)s_len + 3) & ~3ull; // (the arena layout of rawdtw_upload_reference)
        ref_off[2 * s] = total; ref_off[2 * s + 1] = total + padded;
        table[s] = SeqRow{total_bases, total, total + padded, (uint32_t)len[s], s_len};
        ref_len[s] = s_len;
        total += 2 * padded;
        total_bases += len[s];
        max_s_len = std::max<uint64_t>(max_s_len, s_len);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t model_floats = 1ull << (2 * k);
    const Layout L = layout(n_seq, total_bases, model_floats);
    char *blk = nullptr;
    float *d_new = nullptr;
    const size_t CH = 8u << 20; // bytes a staging buffer
    uint8_t *stage[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr}, ev[3] = {nullptr, nullptr, nullptr};
    hipError_t e = hipMalloc((void **)&blk, L.need);
    if (e == hipSuccess) e = hipMalloc((void **)&d_new, std::max<uint64_t>(total, 4) * 4);
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        e = hipHostMalloc((void **)&stage[i], CH, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreate(&done[i]);
    }
    for (int i = 0; i < 3 && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
    RefHold *hold = e == hipSuccess ? new (std::nothrow) RefHold : nullptr;
    std::vector<StrandSteps> h_steps;
    if (e == hipSuccess && hold) {
        uint8_t *d_bases = (uint8_t *)(blk + L.bases.at);
        SeqRow *d_table = (SeqRow *)(blk + L.table.at);
        StrandSums *d_sums = (StrandSums *)(blk + L.sums.at);
        StrandSteps *d_steps = (StrandSteps *)(blk + L.steps.at);
        float *d_model = (float *)(blk + L.model.at);
        int which = 0;
        bool used[2] = {false, false};
        for (uint32_t s = 0; s < n_seq && e == hipSuccess; s++) {
            uint64_t left = len[s], from = 0;
            while (left && e == hipSuccess) {
                const size_t take = (size_t)std::min<uint64_t>(left, CH);
                if (used[which]) e = hipEventSynchronize(done[which]);
                if (e != hipSuccess) break;
                memcpy(stage[which], bases[s] + from, take);
                e = hipMemcpyAsync(d_bases + table[s].base_off + from, stage[which], take, hipMemcpyHostToDevice, ctx->stream);
                if (e == hipSuccess) e = hipEventRecord(done[which], ctx->stream);
                used[which] = true;
                which ^= 1; left -= take; from += take;
            }
        }
        if (e == hipSuccess && n_seq) e = hipMemcpyAsync(d_table, table.data(), n_seq * sizeof(SeqRow), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_model, pore_vals, model_floats * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(ev[0], ctx->stream);
        if (e == hipSuccess && n_seq) {
            const int in_lds = k <= kModelLdsMaxK;
            hipLaunchKernelGGL(k_refsig_sums, dim3(2 * n_seq), dim3(kStep), in_lds ? model_floats * 4 : 0, ctx->stream, d_bases, d_table, d_model, k,
                               in_lds, contracted != 0, d_sums, d_steps);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ev[1], ctx->stream);
        if (e == hipSuccess && n_seq && max_s_len) {
            const uint32_t gy = (uint32_t)std::min<uint64_t>((max_s_len + 255) / 256, 1024);
            hipLaunchKernelGGL(k_refsig_write, dim3(2 * n_seq, gy), dim3(256), 0, ctx->stream, d_bases, d_table, d_model, k, d_sums, d_new);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ev[2], ctx->stream);
        if (e == hipSuccess) {
            try { h_steps.resize(2ull * n_seq); } catch (const std::bad_alloc &) { e = hipErrorOutOfMemory; }
        }
        if (e == hipSuccess && n_seq) e = hipMemcpyAsync(h_steps.data(), d_steps, 2ull * n_seq * sizeof(StrandSteps), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        else (void)hipStreamSynchronize(ctx->stream); // (the staging buffers are still in flight)
    }
    float ms[2] = {0.f, 0.f};
    if (e == hipSuccess && hold) {
        (void)hipEventElapsedTime(&ms[0], ev[0], ev[1]);
        (void)hipEventElapsedTime(&ms[1], ev[1], ev[2]);
    }
    for (int i = 0; i < 2; i++) { if (stage[i]) (void)hipHostFree(stage[i]); if (done[i]) (void)hipEventDestroy(done[i]); }
    for (int i = 0; i < 3; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (blk) (void)hipFree(blk);
    if (e != hipSuccess || !hold) { // the context's previous reference stays as it was
        if (d_new) (void)hipFree(d_new);
        delete hold;
        return e != hipSuccess ? hip_fail(ctx, e, "rawdtw_reference_from_bases") : fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    }
    drop_reference(ctx);
    hold->d = d_new;
    ctx->ref_hold = hold; ctx->d_ref = d_new; ctx->n_ref = total;
    ctx->ref_off.swap(ref_off); ctx->ref_len.swap(ref_len);
    ctx->refsig_built = true;
    ctx->refsig_ms[0] = ms[0]; ctx->refsig_ms[1] = ms[1];
    for (int i = 0; i < 2; i++) ctx->refsig_fast[i] = ctx->refsig_slow[i] = 0;
    for (const StrandSteps &st : h_steps)
        for (int i = 0; i < 2; i++) { ctx->refsig_fast[i] += st.fast[i]; ctx->refsig_slow[i] += st.slow[i]; }
    return RAWDTW_OK;
}

int rawdtw_reference_fetch(rawdtw_ctx *ctx, uint32_t seq, int strand, float *out, uint64_t cap)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!ctx->d_ref || seq >= ctx->ref_len.size()) return fail(ctx, RAWDTW_ERR_INVALID, "no such sequence in the context's reference");
    const uint64_t n = ctx->ref_len[seq];
    if (cap < n) return fail(ctx, RAWDTW_ERR_RANGE, "out is shorter than the strand");
    if (!n) return RAWDTW_OK;
    if (!out) return fail(ctx, RAWDTW_ERR_INVALID, "null out");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_ref + ctx->ref_off[2ull * seq + (strand == 1 ? 0 : 1)], n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RAWDTW_OK;
}

int rawdtw_reference_build_stats(const rawdtw_ctx *ctx, uint64_t fast_steps[2], uint64_t slow_steps[2], float kernel_ms[2])
{
    if (!ctx || !ctx->refsig_built) return RAWDTW_ERR_INVALID;
    for (int i = 0; i < 2; i++) {
        if (fast_steps) fast_steps[i] = ctx->refsig_fast[i];
        if (slow_steps) slow_steps[i] = ctx->refsig_slow[i];
        if (kernel_ms) kernel_ms[i] = ctx->refsig_ms[i];
    }
    return RAWDTW_OK;
}

} // extern "C"
