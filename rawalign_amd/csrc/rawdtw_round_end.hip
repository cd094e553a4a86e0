// rawdtw_round_end.hip -- a chunk round's end on the device: what stands between a batch's score / keep and "this read is finished".
//
//   src/rmap.cpp:90-128    gen_primary_chains: the candidates sorted descending by the 7-key comparator of src/rmap.h:41-45, then the walk
//                          that keeps a chain unless it overlaps a kept one on its sequence, and ends below a third of the last kept score
//   src/rmap.cpp:65-88     comp_mapq for the first primary chain
//   src/rmap.cpp:594-665   is_mapped_with_high_confidence over the primary chains
// as restated on the host by rawdtw_round_end_host (rawdtw_host.cpp, over rawdtw_gen_primary_chains and
// rawdtw_is_mapped_with_high_confidence), which the tests compare this with read by read and bit for bit.
//
// A WAVE A READ, A LANE A CANDIDATE.  The chains that take part (rmap.cpp:525) are compacted into the lanes through 64 words of LDS -- the one
// use of LDS; everything else is in registers.  The comparator is a strict total order unless two records are equal on all seven keys, so a
// lane's place in the sorted order is the number of lanes whose tuple is greater: one pass over the read's own candidates, each broadcast
// with v_readlane.  The selection walks the sorted order as a wave-uniform loop: the candidate at place ci is the lane whose rank is ci
// (a ballot), the primaries kept so far live in lanes 0 .. nk - 1 and test the overlap together (a ballot), and the "below a third" test
// leaves the loop.  The stop rule's mean is a serial fp32 sum in primary order, as the source's.
//
// ARITHMETIC.  fp32 throughout; every division is __fdiv_rn (IEEE, correctly rounded); the unit is compiled with -ffp-contract=off, and no
// product feeds a sum here in any case; gfx950 keeps fp32 denormals (hipcc does not flush them unless asked to).
//
// WHAT IS DECLINED, a read at a time (flag bit 1; the caller ends that read with rawdtw_round_end_host): more than 64 chains taking part; two of
// them equal on all seven keys (std::sort's choice is its own, and it decides whose anchors survive); a NaN score; a quotient of comp_mapq or
// of the stop rule that is not finite, or comp_mapq's product outside int (x86's conversion there is not the device's).
//
// ONE ENQUEUE, ONE LAYOUT.  rawdtw_round_end (host arrays) and rawdtw_batch_round_end_begin (a batch's arrays where they lie) both go through
// round_end_begin: the workspace is described once (RoundEndLayout), whatever is on the host is copied up, one launch, one copy home.
#include "rawdtw_capi.h"

#include <cmath>
#include <cstring>

namespace rawdtw {
namespace {

constexpr uint32_t kReWaves = 4; // reads a workgroup

struct RoundEndArgs {
    const uint64_t *chain_off;
    const rawdtw_chain_rec_t *recs;
    const float *score;
    const uint8_t *keep;
    uint64_t n_reads, n_chains;
    rawdtw_select_opt_t opt;
    rawdtw_round_out_t *out;
    uint32_t *primary;
};

__device__ __forceinline__ void lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint32_t uni(const uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
// lane l's value in every lane (l wave-uniform)
__device__ __forceinline__ uint32_t lane_of(const uint32_t x, const uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)uni(l)); }
__device__ __forceinline__ float lane_of(const float x, const uint32_t l) { return __builtin_bit_cast(float, lane_of(__builtin_bit_cast(uint32_t, x), l)); }
__device__ __forceinline__ bool finite(const float x) { return fabsf(x) < __builtin_inff(); }

__global__ __launch_bounds__(64 * kReWaves) void k_round_end(const RoundEndArgs a)
{
    __shared__ uint32_t s_sel[kReWaves][64];
    const uint32_t lane = threadIdx.x & 63u, w = uni(threadIdx.x >> 6);
    const uint64_t r = (uint64_t)blockIdx.x * kReWaves + w;
    if (r >= a.n_reads) return; // (whole waves: no workgroup barrier below)
    uint64_t c0 = a.chain_off[r], c1 = a.chain_off[r + 1];
    const bool bad = c0 > c1 || c1 > a.n_chains; // (offsets the host forms have checked: nothing is read or written outside the arrays)
    if (bad) c0 = c1 = 0;
    const bool evaluate = a.opt.evaluate_chains != 0;
    uint32_t *sel = s_sel[w];

    // the chains that take part (rmap.cpp:525), in evaluation order, one a lane
    uint32_t n = 0;
    for (uint64_t b = c0; b < c1; b += 64) {
        const uint64_t c = b + lane;
        const bool part = c < c1 && (!evaluate || a.keep[c] != 0);
        const unsigned long long m = __ballot(part);
        const uint32_t pos = n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (part && pos < 64u) sel[pos] = (uint32_t)(c - c0);
        if (c < c1) a.primary[c] = RAWDTW_NO_PRIMARY;
        n = uni(n + (uint32_t)__popcll(m));
    }
    lds_sync();
    bool declined = bad || n > 64u;
    const bool live = !declined && lane < n;
    uint32_t idx = 0, na = 0, strand = 0, seq = 0, start = 0, end = 0;
    float as = 0.0f, cs = 0.0f;
    if (live) {
        idx = sel[lane];
        const rawdtw_chain_rec_t rec = a.recs[c0 + idx];
        as = a.score[c0 + idx]; cs = rec.chaining_score;
        na = rec.n_anchors; strand = rec.key & 1u; seq = rec.key >> 1; start = rec.start_position; end = rec.end_position;
    }
    if (__ballot(live && (as != as || cs != cs))) declined = true;

    // a lane's place in the descending order of rmap.h:41-45 = the lanes whose tuple is greater
    uint32_t rank = 0;
    bool dup = false;
    for (uint32_t j = 0; !declined && j < n; j++) {
        const float jas = lane_of(as, j), jcs = lane_of(cs, j);
        const uint32_t jna = lane_of(na, j), jst = lane_of(strand, j), jsq = lane_of(seq, j), jb = lane_of(start, j), je = lane_of(end, j);
        bool gt = false, eq = false;
        if (jas != as) gt = jas > as;
        else if (jcs != cs) gt = jcs > cs;
        else if (jna != na) gt = jna > na;
        else if (jst != strand) gt = jst > strand;
        else if (jsq != seq) gt = jsq > seq;
        else if (jb != start) gt = jb > start;
        else if (je != end) gt = je > end;
        else eq = true;
        rank += gt ? 1u : 0u;
        dup |= eq && j != lane;
    }
    if (__ballot(live && dup)) declined = true;

    // the walk of rmap.cpp:94-127: the primaries kept so far in lanes 0 .. nk - 1
    uint32_t nk = 0, na0 = 0;
    uint32_t p_seq = 0, p_start = 0, p_end = 0, p_idx = 0;
    float p_score = 0.0f, back = 0.0f;
    for (uint32_t ci = 0; !declined && ci < n; ci++) {
        const uint32_t src = (uint32_t)__builtin_ctzll(__ballot(live && rank == ci) | (1ull << 63));
        const float s = evaluate ? lane_of(as, src) : lane_of(cs, src);
        if (ci > 0 && s < __fdiv_rn(back, 3.0f)) break; // rmap.cpp:100-104
        const uint32_t c_seq = lane_of(seq, src), c_start = lane_of(start, src), c_end = lane_of(end, src), c_idx = lane_of(idx, src);
        const bool hit = lane < nk && p_seq == c_seq && max(c_start, p_start) <= min(c_end, p_end); // rmap.cpp:113-120
        if (__ballot(hit)) continue;
        if (nk == 0) na0 = lane_of(na, src);
        if (lane == nk) { p_seq = c_seq; p_start = c_start; p_end = c_end; p_idx = c_idx; p_score = s; }
        nk++;
        back = s;
    }

    uint32_t mapq = 0;
    bool high = false;
    if (!declined && nk) {
        const float s0 = lane_of(p_score, 0), s1 = lane_of(p_score, nk >= 2 ? 1u : 0u);
        if (nk == 1) mapq = 60; // rmap.cpp:67
        else {                  // rmap.cpp:74-86
            const float q = __fdiv_rn(s1, s0), p = 40.0f * (1.0f - q);
            if (!finite(q) || !(p >= -2147483648.0f && p < 2147483648.0f)) declined = true;
            else { const int v = (int)p; mapq = v > 60 ? 60u : v < 0 ? 0u : (uint32_t)v; }
        }
        if (!declined && na0 != 0) { // rmap.cpp:597-598
            if (nk >= 2) {
                const float q = __fdiv_rn(s0, s1);
                if (!finite(q)) declined = true;
                else if (q >= a.opt.min_bestmap_ratio) high = true; // rmap.cpp:604, 651
                else {
                    float mean = 0.0f;
                    for (uint32_t k = 0; k < nk; k++) mean += lane_of(p_score, k); // serial, in primary order
                    mean = __fdiv_rn(mean, (float)nk);
                    high = s0 >= a.opt.min_meanmap_ratio * mean; // rmap.cpp:615, 658
                }
            } else high = na0 >= a.opt.min_chain_anchor; // rmap.cpp:620, 659
        }
    }
    if (declined) { nk = 0; mapq = 0; high = false; }
    if (lane < nk) a.primary[c0 + lane] = p_idx;
    if (lane == 0) a.out[r] = rawdtw_round_out_t{nk, mapq, (high ? RAWDTW_ROUND_HIGH : 0u) | (declined ? RAWDTW_ROUND_DECLINED : 0u)};
}

using capi::carve;
// The workspace, described once: lay(0) gives the bytes it needs, lay(the block's base) the pointers.  The inputs' regions are there for
// either form (a batch's round end leaves those it reads in place unused); out and primary lie one behind the other and come home in one copy.
struct RoundEndLayout {
    uint64_t n_reads, n_chains;
    uint64_t *coff; float *score; uint8_t *keep; rawdtw_chain_rec_t *recs;
    rawdtw_round_out_t *out; uint32_t *primary;
    size_t home_bytes; // from out to primary's end

    size_t lay(void *base)
    {
        uintptr_t p = reinterpret_cast<uintptr_t>(base);
        coff = carve<uint64_t>(p, n_reads + 1); score = carve<float>(p, n_chains); keep = carve<uint8_t>(p, n_chains); recs = carve<rawdtw_chain_rec_t>(p, n_chains);
        out = carve<rawdtw_round_out_t>(p, n_reads); primary = carve<uint32_t>(p, n_chains);
        home_bytes = (size_t)(reinterpret_cast<uintptr_t>(primary) - reinterpret_cast<uintptr_t>(out)) + (size_t)n_chains * 4;
        return (size_t)(p - reinterpret_cast<uintptr_t>(base));
    }
};

} // namespace
} // namespace rawdtw

using namespace rawdtw;
using namespace rawdtw::capi;

struct rawdtw_round_end_ws {
    WsBlocks w;
    // a round end begun and not fetched
    bool pending = false;
    uint64_t n_reads = 0, n_chains = 0;
    rawdtw_select_opt_t opt{};
    const rawdtw_batch *batch = nullptr; // (null: rawdtw_round_end's own)
    bool batch_was_stream = false;
    const rawdtw_chain_rec_t *d_recs = nullptr;
    const rawdtw_round_out_t *d_out = nullptr; // out and primary in the workspace, for what is enqueued behind the launch (rawdtw_keep.hip)
    const uint32_t *d_primary = nullptr;
    uint64_t serial = 0;                       // launches so far
    size_t home_at = 0, home_bytes = 0, primary_at = 0; // where out lies in the block, what comes home, primary's place in it
    float kernel_ms = 0.0f;
};

namespace {

// where the arrays the kernel reads are: `on_device` the three of a batch in device memory, else host arrays that go up; recs on its own
struct RoundEndIn {
    const uint64_t *chain_off; const float *score; const uint8_t *keep; bool on_device;
    const rawdtw_chain_rec_t *recs; bool recs_on_device;
};

// the one enqueue: workspace, uploads, the launch, the results' copy into the page-locked block, the event behind it
int round_end_begin(rawdtw_ctx *ctx, const rawdtw_select_opt_t *opt, uint64_t n_reads, uint64_t n_chains, const RoundEndIn &in, const rawdtw_batch *batch)
{
    if (n_reads == 0 || n_reads > 0xffffffffull * kReWaves) return fail(ctx, RAWDTW_ERR_INVALID, "no reads, or too many");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->round_end_ws) ctx->round_end_ws = new (std::nothrow) rawdtw_round_end_ws;
    if (!ctx->round_end_ws) return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    rawdtw_round_end_ws &ws = *ctx->round_end_ws;
    RoundEndLayout L{n_reads, n_chains};
    const size_t need = L.lay(nullptr);
    if (const int st = blocks_reserve(ctx, ws.w, need, L.home_bytes + 256, "round-end workspace allocation failed")) return st;
    (void)L.lay(ws.w.dev);
    hipStream_t s = ctx->stream;
    if (!in.on_device) {
        HIP_TRY(ctx, hipMemcpyAsync(L.coff, in.chain_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, s));
        if (n_chains) HIP_TRY(ctx, hipMemcpyAsync(L.score, in.score, n_chains * 4, hipMemcpyHostToDevice, s));
        if (n_chains && in.keep) HIP_TRY(ctx, hipMemcpyAsync(L.keep, in.keep, n_chains, hipMemcpyHostToDevice, s));
    }
    if (!in.recs_on_device && n_chains) HIP_TRY(ctx, hipMemcpyAsync(L.recs, in.recs, n_chains * sizeof(rawdtw_chain_rec_t), hipMemcpyHostToDevice, s));
    RoundEndArgs a{in.on_device ? in.chain_off : L.coff, in.recs_on_device ? in.recs : L.recs, in.on_device ? in.score : L.score,
                   in.on_device ? in.keep : L.keep, n_reads, n_chains, *opt, L.out, L.primary};
    HIP_TRY(ctx, hipEventRecord(ws.w.ev0, s));
    hipLaunchKernelGGL(k_round_end, dim3((uint32_t)((n_reads + kReWaves - 1) / kReWaves)), dim3(64 * kReWaves), 0, s, a);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ws.w.ev1, s));
    HIP_TRY(ctx, hipMemcpyAsync(ws.w.pin, L.out, L.home_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(ws.w.done, s));
    ws.pending = true; ws.n_reads = n_reads; ws.n_chains = n_chains; ws.opt = *opt; ws.batch = batch;
    ws.batch_was_stream = batch && batch->stream;
    ws.d_recs = a.recs; ws.d_out = L.out; ws.d_primary = L.primary; ws.serial++;
    ws.home_bytes = L.home_bytes;
    ws.primary_at = (size_t)(reinterpret_cast<uintptr_t>(L.primary) - reinterpret_cast<uintptr_t>(L.out));
    return RAWDTW_OK;
}

int round_end_fetch(rawdtw_ctx *ctx, rawdtw_round_out_t *out, uint32_t *primary)
{
    rawdtw_round_end_ws &ws = *ctx->round_end_ws;
    ws.pending = false;
    HIP_TRY(ctx, hipEventSynchronize(ws.w.done));
    (void)hipEventElapsedTime(&ws.kernel_ms, ws.w.ev0, ws.w.ev1);
    const char *h = reinterpret_cast<const char *>(ws.w.pin);
    memcpy(out, h, ws.n_reads * sizeof(rawdtw_round_out_t));
    if (ws.n_chains) memcpy(primary, h + ws.primary_at, ws.n_chains * 4);
    return RAWDTW_OK;
}

bool round_end_busy(rawdtw_ctx *ctx) { return ctx->round_end_ws && ctx->round_end_ws->pending; }

} // namespace

extern "C" {

int rawdtw_round_end(rawdtw_ctx *ctx, const rawdtw_select_opt_t *opt, uint64_t n_reads, const uint64_t *chain_off, const rawdtw_chain_rec_t *recs,
                     const float *score, const uint8_t *keep, rawdtw_round_out_t *out, uint32_t *primary)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!opt || !chain_off || !out) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (round_end_busy(ctx)) return fail(ctx, RAWDTW_ERR_INVALID, "a round end is begun on this context and not fetched");
    if (n_reads && chain_off[0] != 0) return fail(ctx, RAWDTW_ERR_INVALID, "offsets do not start at 0");
    for (uint64_t r = 0; r < n_reads; r++)
        if (chain_off[r + 1] < chain_off[r]) return fail(ctx, RAWDTW_ERR_INVALID, "offsets do not ascend");
    if (n_reads == 0) return RAWDTW_OK; // (as rawdtw_round_end_host: nothing to do, nothing launched)
    const uint64_t nc = chain_off[n_reads];
    if (nc && (!recs || !score || !primary || (opt->evaluate_chains && !keep))) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    const RoundEndIn in{chain_off, score, keep, false, recs, false};
    const int st = round_end_begin(ctx, opt, n_reads, nc, in, nullptr);
    return st == RAWDTW_OK ? round_end_fetch(ctx, out, primary) : st;
}

int rawdtw_batch_round_end_begin(rawdtw_ctx *ctx, rawdtw_batch *batch, const rawdtw_select_opt_t *opt, const rawdtw_chain_rec_t *recs, int recs_on_device)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!batch || batch->ctx != ctx || batch_dead(batch)) return fail(ctx, RAWDTW_ERR_INVALID, "batch does not belong to this context");
    if (!opt || (!recs && batch->n_chains)) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (round_end_busy(ctx)) return fail(ctx, RAWDTW_ERR_INVALID, "a round end is begun on this context and not fetched");
    const RoundEndIn in{batch->d_chain_off, batch->d_score, batch->d_keep, true, recs, recs_on_device != 0};
    return round_end_begin(ctx, opt, batch->n_reads, batch->n_chains, in, batch);
}

int rawdtw_batch_round_end_fetch(rawdtw_ctx *ctx, rawdtw_batch *batch, rawdtw_round_out_t *out, uint32_t *primary)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!round_end_busy(ctx) || !batch || ctx->round_end_ws->batch != batch) return fail(ctx, RAWDTW_ERR_INVALID, "no round end begun for this batch");
    if (!out || (!primary && batch->n_chains)) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    rawdtw_round_end_ws &ws = *ctx->round_end_ws;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the scores the kernel read are the batch's only if the device-planned path did not decline it: else it is scored again through the
    // job list (by rawdtw_batch_fetch before this call, or here) and the round end runs again, on those scores, with the records where they are
    bool redone = false;
    int st = batch_settle(ctx, batch, &redone);
    if (st != RAWDTW_OK) { ws.pending = false; return st; }
    if (redone || (ws.batch_was_stream && !batch->stream)) {
        if (!batch->plan) { ws.pending = false; return fail(ctx, RAWDTW_ERR_INVALID, "the batch has no scores (its fetch failed)"); }
        const RoundEndIn in{batch->d_chain_off, batch->d_score, batch->d_keep, true, ws.d_recs, true};
        const rawdtw_select_opt_t opt = ws.opt;
        st = round_end_begin(ctx, &opt, batch->n_reads, batch->n_chains, in, batch);
        if (st != RAWDTW_OK) { ws.pending = false; return st; }
    }
    return round_end_fetch(ctx, out, primary);
}

} // extern "C"

namespace rawdtw { namespace capi {
void round_end_ws_free(rawdtw_ctx *ctx)
{
    if (!ctx || !ctx->round_end_ws) return;
    blocks_release(ctx->round_end_ws->w);
    delete ctx->round_end_ws;
    ctx->round_end_ws = nullptr;
}
// a batch on its way out: a round end begun for it and not fetched is waited for and dropped (the arrays it reads go with the batch)
void round_end_forget(rawdtw_ctx *ctx, const rawdtw_batch *b)
{
    if (!ctx || !ctx->round_end_ws || !ctx->round_end_ws->pending || ctx->round_end_ws->batch != b) return;
    (void)hipEventSynchronize(ctx->round_end_ws->w.done);
    ctx->round_end_ws->pending = false;
    ctx->round_end_ws->batch = nullptr;
}
bool round_end_view(const rawdtw_ctx *ctx, RoundEndView *v)
{
    if (!ctx || !ctx->round_end_ws || !ctx->round_end_ws->serial) return false;
    const rawdtw_round_end_ws &ws = *ctx->round_end_ws;
    v->pending = ws.pending; v->batch = ws.batch; v->n_reads = ws.n_reads; v->n_chains = ws.n_chains; v->serial = ws.serial;
    v->d_out = ws.d_out; v->d_primary = ws.d_primary; v->d_recs = ws.d_recs;
    return true;
}
int64_t round_end_kernel_us(const rawdtw_ctx *ctx) { return ctx->round_end_ws ? (int64_t)std::lround(ctx->round_end_ws->kernel_ms * 1000.0f) : 0; }
} }
