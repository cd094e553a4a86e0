// rawdtw_keep.hip -- the kept chains: a round's primary chains stay on the device as the next round's previous seeds.
//
//   src/rmap.cpp:344-357   gen_chains re-seeds a round with the anchors of the chains the read kept from the round before
// as the mapper's write_seeds restates it over rd.chains, and rawdtw_round_keep_host (rawdtw_host.cpp) over a round's flat arrays, which
// the tests compare this with byte for byte.
//
// THE STORE (rawdtw_keep_layout.h): n_slots x 2 halves of N seeds and a count each, one device block a context, grow-only.  A round writes
// the half a read is not seeded from; which half a read is seeded from is the caller's knowledge (the mapper switches in its commit block
// only), so a failed round leaves the caller as it was.  The context mirrors every half's count on the host; rawdtw_chain.hip's resident
// begin checks a read's stretch against the mirror before anything is enqueued.
//
// A WAVE A READ.  Lane p < n_primary loads its chain's n_anchors and where its anchors start; a prefix sum over the wave gives each
// chain's place in the half and the total.  A read that is declined, has no destination or whose total is above N writes the count
// RAWDTW_NOT_KEPT and no seed.  Else all 64 lanes take the primary chains one after the other, best first, and copy each chain's anchors in
// the order they lie as {key, target, query}: 64 consecutive 12-byte stores a step, all inside the read's own half.  No LDS.
//
// ONE ENQUEUE.  rawdtw_round_keep (host arrays, for tests) and rawdtw_batch_round_end_keep (the arrays where the round left them) both go
// through keep_enqueue: one launch, the counts' copy into the page-locked block, the event behind it.
#include "rawdtw_capi.h"
#include "rawdtw_keep_layout.h"

#include <cmath>
#include <cstring>

namespace rawdtw {
namespace {

constexpr uint32_t kKeepWaves = 4; // reads a workgroup

struct KeepArgs {
    const uint64_t *chain_off;
    const rawdtw_chain_rec_t *recs;
    const uint64_t *anchor_off;
    const rawdtw_anchor_t *anchors;
    const rawdtw_round_out_t *out;
    const uint32_t *primary;
    const uint32_t *dst;
    uint64_t n_reads;
    keep::Layout L;
    char *store;
    uint32_t *kept_count;
};

__device__ __forceinline__ uint32_t uni(const uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

__global__ __launch_bounds__(64 * kKeepWaves) void k_keep_primary(const KeepArgs a)
{
    const uint32_t lane = threadIdx.x & 63u, w = uni(threadIdx.x >> 6);
    const uint64_t r = (uint64_t)blockIdx.x * kKeepWaves + w;
    if (r >= a.n_reads) return; // (whole waves)
    const uint32_t addr = a.dst[r];
    const bool has_dst = addr != RAWDTW_NO_KEEP && addr < a.L.halves(); // (the host has checked the addresses: nothing is written outside the store)
    const uint64_t c0 = a.chain_off[r], c1 = a.chain_off[r + 1];
    const rawdtw_round_out_t o = a.out[r];
    const uint32_t cap = (uint32_t)a.L.n_seeds;
    const uint64_t n_chains = c1 > c0 ? c1 - c0 : 0;
    uint32_t np = o.n_primary < 64u ? o.n_primary : 64u;
    if (np > n_chains) np = (uint32_t)n_chains;
    bool kept = has_dst && !(o.flags & RAWDTW_ROUND_DECLINED) && np == o.n_primary;

    // counting: lane p's chain, its anchors, its place in the half.  A chain's count is taken as at most cap + 1: the sum of 64 of them
    // stays below 2^32 and is above cap exactly when the true total is
    uint32_t na = 0;
    uint64_t a0 = 0;
    uint32_t key = 0;
    if (lane < np) {
        const uint32_t idx = a.primary[c0 + lane];
        if (idx < n_chains) {
            const rawdtw_chain_rec_t rec = a.recs[c0 + idx];
            na = min(rec.n_anchors, cap + 1u); key = rec.key; a0 = a.anchor_off[c0 + idx];
        } else na = cap + 1u; // (an index outside the read: nothing of it is kept)
    }
    uint32_t incl = na;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= (uint32_t)d) incl += t;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63);
    const uint32_t at = incl - na;
    if (total > cap) kept = false;

    if (lane == 0) {
        a.kept_count[r] = kept ? total : RAWDTW_NOT_KEPT;
        if (has_dst) *reinterpret_cast<uint32_t *>(a.store + a.L.count_at(addr)) = kept ? total : RAWDTW_NOT_KEPT;
    }
    if (!kept) return;
    rawdtw_seed_t *half = reinterpret_cast<rawdtw_seed_t *>(a.store + a.L.seeds_at(addr));
    for (uint32_t p = 0; p < np; p++) { // best first; at + k < total <= N: inside the half
        const uint32_t pn = (uint32_t)__shfl((int)na, (int)p), pat = (uint32_t)__shfl((int)at, (int)p), pkey = (uint32_t)__shfl((int)key, (int)p);
        const uint64_t pa0 = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(a0 >> 32), (int)p) << 32) | (uint32_t)__shfl((int)(uint32_t)a0, (int)p);
        for (uint32_t k = lane; k < pn; k += 64) {
            const rawdtw_anchor_t an = a.anchors[pa0 + k];
            half[pat + k] = rawdtw_seed_t{pkey, an.target_position, an.query_position};
        }
    }
}

using capi::carve;
// rawdtw_round_keep's workspace, described once: lay(0) gives the bytes it needs, lay(the block's base) the pointers.  The batch form uses
// dst and kept alone (everything else lies where the round left it).
struct KeepWsLayout {
    uint64_t n_reads, n_chains, n_anchors;
    uint64_t *coff, *aoff; rawdtw_chain_rec_t *recs; rawdtw_anchor_t *anch; rawdtw_round_out_t *out; uint32_t *primary, *dst, *kept;

    size_t lay(void *base)
    {
        uintptr_t p = reinterpret_cast<uintptr_t>(base);
        dst = carve<uint32_t>(p, n_reads); kept = carve<uint32_t>(p, n_reads);
        coff = carve<uint64_t>(p, n_reads + 1); aoff = carve<uint64_t>(p, n_chains + 1); recs = carve<rawdtw_chain_rec_t>(p, n_chains);
        anch = carve<rawdtw_anchor_t>(p, n_anchors); out = carve<rawdtw_round_out_t>(p, n_reads); primary = carve<uint32_t>(p, n_chains);
        return (size_t)(p - reinterpret_cast<uintptr_t>(base));
    }
};

} // namespace
} // namespace rawdtw

using namespace rawdtw;
using namespace rawdtw::capi;

struct rawdtw_keep_ws {
    // the store
    char *store = nullptr;
    keep::Layout L;
    std::vector<uint32_t> mirror; // per half: its count as the last fetched keep left it (RAWDTW_NOT_KEPT: not kept, never written, or in flight)
    // the launch's workspace, and a keep enqueued and not fetched
    WsBlocks w;
    bool pending = false;
    const rawdtw_batch *batch = nullptr; // (null: rawdtw_round_keep's own)
    uint64_t n_reads = 0;
    uint64_t end_serial = 0;             // the round end it ran behind (RoundEndView::serial)
    std::vector<uint32_t> dst;
    std::vector<uint8_t> seen;           // (scratch of the address check)
    float kernel_ms = 0.0f;
};

namespace {

rawdtw_keep_ws *keep_ws(rawdtw_ctx *ctx)
{
    if (!ctx->keep_ws) ctx->keep_ws = new (std::nothrow) rawdtw_keep_ws;
    return ctx->keep_ws;
}

// every dst is RAWDTW_NO_KEEP or an address of the store, none twice
int check_dst(rawdtw_ctx *ctx, rawdtw_keep_ws &ws, uint64_t n_reads, const uint32_t *dst)
{
    if (!ws.store) return fail(ctx, RAWDTW_ERR_INVALID, "no store of kept chains on this context (rawdtw_chain_keep_reserve)");
    try { ws.seen.assign((size_t)ws.L.halves(), 0); ws.dst.assign(dst, dst + n_reads); } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    for (uint64_t r = 0; r < n_reads; r++) {
        if (dst[r] == RAWDTW_NO_KEEP) continue;
        if (dst[r] >= ws.L.halves()) return fail(ctx, RAWDTW_ERR_INVALID, "a destination is outside the store of kept chains");
        if (ws.seen[dst[r]]) return fail(ctx, RAWDTW_ERR_INVALID, "two reads have the same destination in the store of kept chains");
        ws.seen[dst[r]] = 1;
    }
    return RAWDTW_OK;
}

// the one enqueue: the launch on arrays that are in device memory (dst among them), the counts' copy home, the event behind it
int keep_enqueue(rawdtw_ctx *ctx, rawdtw_keep_ws &ws, KeepArgs a)
{
    hipStream_t s = ctx->stream;
    a.L = ws.L; a.store = ws.store;
    HIP_TRY(ctx, hipEventRecord(ws.w.ev0, s));
    hipLaunchKernelGGL(k_keep_primary, dim3((uint32_t)((a.n_reads + kKeepWaves - 1) / kKeepWaves)), dim3(64 * kKeepWaves), 0, s, a);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ws.w.ev1, s));
    HIP_TRY(ctx, hipMemcpyAsync(ws.w.pin, a.kept_count, a.n_reads * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(ws.w.done, s));
    // a half written is void in the mirror until the counts are home
    for (uint64_t r = 0; r < a.n_reads; r++)
        if (ws.dst[r] != RAWDTW_NO_KEEP) ws.mirror[ws.dst[r]] = RAWDTW_NOT_KEPT;
    return RAWDTW_OK;
}

int keep_collect(rawdtw_ctx *ctx, rawdtw_keep_ws &ws, uint32_t *kept_count)
{
    HIP_TRY(ctx, hipEventSynchronize(ws.w.done));
    (void)hipEventElapsedTime(&ws.kernel_ms, ws.w.ev0, ws.w.ev1);
    const uint32_t *h = reinterpret_cast<const uint32_t *>(ws.w.pin);
    memcpy(kept_count, h, ws.n_reads * 4);
    for (uint64_t r = 0; r < ws.n_reads; r++)
        if (ws.dst[r] != RAWDTW_NO_KEEP) ws.mirror[ws.dst[r]] = h[r];
    return RAWDTW_OK;
}

// the batch form's launch: everything but dst and the counts lies where the round left it
int keep_batch_enqueue(rawdtw_ctx *ctx, rawdtw_keep_ws &ws, const RoundEndView &ev, const ChainKeptView &cv, const rawdtw_batch *batch, bool upload_dst)
{
    KeepWsLayout L{ws.n_reads, 0, 0};
    (void)L.lay(ws.w.dev);
    if (upload_dst) HIP_TRY(ctx, hipMemcpyAsync(L.dst, ws.dst.data(), ws.n_reads * 4, hipMemcpyHostToDevice, ctx->stream));
    KeepArgs a{batch->d_chain_off, cv.d_recs, cv.d_aoff, cv.d_anch, ev.d_out, ev.d_primary, L.dst, ws.n_reads, keep::Layout{}, nullptr, L.kept};
    return keep_enqueue(ctx, ws, a);
}

} // namespace

extern "C" {

int rawdtw_chain_keep_reserve(rawdtw_ctx *ctx, uint64_t n_slots, uint64_t seeds_per_half)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (n_slots == 0 || n_slots > keep::kMaxSlots || seeds_per_half == 0 || seeds_per_half > keep::kMaxSeeds)
        return fail(ctx, RAWDTW_ERR_INVALID, "a store of kept chains has 1 .. 2^30 slots of 1 .. 2^20 seeds a half");
    rawdtw_keep_ws *ws = keep_ws(ctx);
    if (!ws) return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    if (ws->pending) return fail(ctx, RAWDTW_ERR_INVALID, "a keep is enqueued on this context and not fetched");
    if (ws->store && ws->L.n_slots >= n_slots && ws->L.n_seeds >= seeds_per_half) return RAWDTW_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const keep::Layout L = keep::layout(std::max(n_slots, ws->L.n_slots), std::max(seeds_per_half, ws->L.n_seeds));
    std::vector<uint32_t> mirror;
    try { mirror.assign((size_t)L.halves(), RAWDTW_NOT_KEPT); } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    void *d = nullptr;
    if (hipMalloc(&d, L.need) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, RAWDTW_ERR_OOM, "allocation of the store of kept chains failed"); }
    // every count RAWDTW_NOT_KEPT; on the context's stream, where everything that reads or writes the store is enqueued
    const hipError_t e = hipMemsetAsync(d, 0xff, L.counts_bytes, ctx->stream);
    if (e != hipSuccess) { (void)hipFree(d); return hip_fail(ctx, e, "hipMemsetAsync"); }
    if (ws->store) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ws->store); } // (a launch that reads the old block may be in flight)
    ws->store = static_cast<char *>(d); ws->L = L; ws->mirror.swap(mirror);
    return RAWDTW_OK;
}

int rawdtw_round_keep(rawdtw_ctx *ctx, uint64_t n_reads, const uint64_t *chain_off, const rawdtw_chain_rec_t *recs, const uint64_t *anchor_off,
                      const rawdtw_anchor_t *anchors, const rawdtw_round_out_t *out, const uint32_t *primary, const uint32_t *dst, uint32_t *kept_count)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!chain_off || !out || !dst || !kept_count) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n_reads == 0) return RAWDTW_OK;
    if (n_reads > 0xffffffffull) return fail(ctx, RAWDTW_ERR_INVALID, "too many reads");
    if (chain_off[0] != 0) return fail(ctx, RAWDTW_ERR_INVALID, "offsets do not start at 0");
    const uint64_t nc = chain_off[n_reads];
    if (nc && (!recs || !anchor_off || !primary)) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    for (uint64_t r = 0; r < n_reads; r++) {
        if (chain_off[r + 1] < chain_off[r] || chain_off[r + 1] > nc) return fail(ctx, RAWDTW_ERR_INVALID, "offsets do not ascend");
        const uint64_t c0 = chain_off[r], n = chain_off[r + 1] - c0;
        if (out[r].n_primary > n || out[r].n_primary > 64) return fail(ctx, RAWDTW_ERR_INVALID, "a read has more primary chains than chains, or than 64");
        for (uint32_t p = 0; p < out[r].n_primary; p++)
            if (primary[c0 + p] >= n) return fail(ctx, RAWDTW_ERR_INVALID, "a primary index is outside its read");
    }
    for (uint64_t c = 0; c < nc; c++)
        if (anchor_off[c + 1] < anchor_off[c] || anchor_off[c + 1] - anchor_off[c] != recs[c].n_anchors)
            return fail(ctx, RAWDTW_ERR_INVALID, "a chain's anchor_off stretch is not its n_anchors");
    const uint64_t na = nc ? anchor_off[nc] : 0;
    if (na && !anchors) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    rawdtw_keep_ws *wsp = keep_ws(ctx);
    if (!wsp) return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    rawdtw_keep_ws &ws = *wsp;
    if (ws.pending) return fail(ctx, RAWDTW_ERR_INVALID, "a keep is enqueued on this context and not fetched");
    if (const int st = check_dst(ctx, ws, n_reads, dst)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    KeepWsLayout L{n_reads, nc, na};
    const size_t need = L.lay(nullptr);
    if (const int st = blocks_reserve(ctx, ws.w, need, n_reads * 4 + 256, "keep workspace allocation failed")) return st;
    (void)L.lay(ws.w.dev);
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(L.dst, dst, n_reads * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(L.coff, chain_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(L.out, out, n_reads * sizeof(rawdtw_round_out_t), hipMemcpyHostToDevice, s));
    if (nc) {
        HIP_TRY(ctx, hipMemcpyAsync(L.aoff, anchor_off, (nc + 1) * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(L.recs, recs, nc * sizeof(rawdtw_chain_rec_t), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(L.primary, primary, nc * 4, hipMemcpyHostToDevice, s));
    }
    if (na) HIP_TRY(ctx, hipMemcpyAsync(L.anch, anchors, na * sizeof(rawdtw_anchor_t), hipMemcpyHostToDevice, s));
    ws.n_reads = n_reads; ws.batch = nullptr;
    const KeepArgs a{L.coff, L.recs, L.aoff, L.anch, L.out, L.primary, L.dst, n_reads, keep::Layout{}, nullptr, L.kept};
    int st = keep_enqueue(ctx, ws, a);
    // (the uploads read the caller's pageable arrays: the wait below is behind them too)
    if (st == RAWDTW_OK) st = keep_collect(ctx, ws, kept_count);
    else (void)hipStreamSynchronize(s);
    return st;
}

int rawdtw_batch_round_end_keep(rawdtw_ctx *ctx, rawdtw_batch *batch, const uint32_t *dst)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!batch || !dst) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    RoundEndView ev;
    if (!round_end_view(ctx, &ev) || !ev.pending || ev.batch != batch) return fail(ctx, RAWDTW_ERR_INVALID, "no round end begun for this batch");
    ChainKeptView cv;
    if (!chain_kept_view(ctx, &cv) || cv.d_recs != ev.d_recs)
        return fail(ctx, RAWDTW_ERR_INVALID, "the round end's records are not the context's ended chaining round's");
    if (!ctx->keep_ws || !ctx->keep_ws->store) return fail(ctx, RAWDTW_ERR_INVALID, "no store of kept chains on this context (rawdtw_chain_keep_reserve)");
    rawdtw_keep_ws &ws = *ctx->keep_ws;
    if (ws.pending) return fail(ctx, RAWDTW_ERR_INVALID, "a keep is enqueued on this context and not fetched");
    if (const int st = check_dst(ctx, ws, ev.n_reads, dst)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    KeepWsLayout L{ev.n_reads, 0, 0};
    if (const int st = blocks_reserve(ctx, ws.w, L.lay(nullptr), ev.n_reads * 4 + 256, "keep workspace allocation failed")) return st;
    ws.n_reads = ev.n_reads;
    const int st = keep_batch_enqueue(ctx, ws, ev, cv, batch, true);
    if (st != RAWDTW_OK) return st;
    ws.pending = true; ws.batch = batch; ws.end_serial = ev.serial;
    return RAWDTW_OK;
}

int rawdtw_batch_round_keep_fetch(rawdtw_ctx *ctx, rawdtw_batch *batch, uint32_t *kept_count)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!ctx->keep_ws || !ctx->keep_ws->pending || !batch || ctx->keep_ws->batch != batch) return fail(ctx, RAWDTW_ERR_INVALID, "no keep enqueued for this batch");
    if (!kept_count) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    rawdtw_keep_ws &ws = *ctx->keep_ws;
    RoundEndView ev;
    if (!round_end_view(ctx, &ev) || ev.pending || ev.batch != batch)
        return fail(ctx, RAWDTW_ERR_INVALID, "the batch's round end is not fetched yet (rawdtw_batch_round_end_fetch comes first)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ws.pending = false;
    if (ev.serial != ws.end_serial) { // the round end ran again at its fetch, on the batch's scores from the job list: so does the keep, behind it
        ChainKeptView cv;
        if (!chain_kept_view(ctx, &cv) || cv.d_recs != ev.d_recs) return fail(ctx, RAWDTW_ERR_INVALID, "the context's chaining round has changed since the keep was enqueued");
        if (const int st = keep_batch_enqueue(ctx, ws, ev, cv, batch, false)) return st;
    }
    return keep_collect(ctx, ws, kept_count);
}

int rawdtw_chain_kept_fetch(rawdtw_ctx *ctx, uint32_t addr, rawdtw_seed_t *seeds, uint32_t cap, uint32_t *n)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!n || (cap && !seeds)) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (!ctx->keep_ws || !ctx->keep_ws->store) return fail(ctx, RAWDTW_ERR_INVALID, "no store of kept chains on this context (rawdtw_chain_keep_reserve)");
    const rawdtw_keep_ws &ws = *ctx->keep_ws;
    if (addr >= ws.L.halves()) return fail(ctx, RAWDTW_ERR_INVALID, "the address is outside the store of kept chains");
    if (cap > ws.L.n_seeds) return fail(ctx, RAWDTW_ERR_RANGE, "more seeds asked for than a half holds");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(n, ws.store + ws.L.count_at(addr), 4, hipMemcpyDeviceToHost, ctx->stream));
    if (cap) HIP_TRY(ctx, hipMemcpyAsync(seeds, ws.store + ws.L.seeds_at(addr), (size_t)cap * sizeof(rawdtw_seed_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RAWDTW_OK;
}

} // extern "C"

namespace rawdtw { namespace capi {
void keep_ws_free(rawdtw_ctx *ctx)
{
    if (!ctx || !ctx->keep_ws) return;
    if (ctx->keep_ws->store) (void)hipFree(ctx->keep_ws->store);
    blocks_release(ctx->keep_ws->w);
    delete ctx->keep_ws;
    ctx->keep_ws = nullptr;
}
// a batch on its way out: a keep enqueued for it and not fetched is waited for and dropped (it reads the batch's chain offsets)
void keep_forget(rawdtw_ctx *ctx, const rawdtw_batch *b)
{
    if (!ctx || !ctx->keep_ws || !ctx->keep_ws->pending || ctx->keep_ws->batch != b) return;
    (void)hipEventSynchronize(ctx->keep_ws->w.done);
    ctx->keep_ws->pending = false;
    ctx->keep_ws->batch = nullptr;
}
bool keep_store_view(const rawdtw_ctx *ctx, KeepStoreView *v)
{
    if (!ctx || !ctx->keep_ws || !ctx->keep_ws->store) return false;
    v->store = ctx->keep_ws->store; v->L = ctx->keep_ws->L; v->mirror = ctx->keep_ws->mirror.data();
    return true;
}
int64_t round_keep_kernel_us(const rawdtw_ctx *ctx) { return ctx->keep_ws ? (int64_t)std::lround(ctx->keep_ws->kernel_ms * 1000.0f) : 0; }
} }
