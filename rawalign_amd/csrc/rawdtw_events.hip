// rawdtw_events.hip -- event detection (detect_events, src/revent.c:190-210) for a whole chunk round on the device, bit for bit
// equal to the host restatement (rawdtw_events_host.cpp) and so to the reference, in the plain and the contracted form.
//
// Three recurrences are serial per chunk (the prefix sums, the peak state machine, the two double sums of the normalisation);
// everything else is parallel across positions or events.  Five launches:
//   k_ev_prefix   a lane per chunk, 64 chunks a wave: samples staged through LDS in 64 x 64 tiles (coalesced loads), each lane
//                 walks its own row in sample order, the prefix sums go out through LDS again (coalesced stores)
//   k_ev_tstat    a thread per position over the whole batch, both windows: the bulk of the arithmetic (five correctly
//                 rounded fp32 divisions, one f64 sqrt and one f64 division per position and window)
//   k_ev_peaks    a lane per chunk: the two-detector state machine over LDS tiles of both t-statistics; peaks into the chunk's
//                 own s_len slots, then the chunk's event count
//   k_ev_scan     one workgroup: exclusive scan of the counts -> event_off and the total
//   k_ev_events   a wave per chunk: segment means in parallel, the double sums on one lane in emission order, normalisation in
//                 parallel, written at event_off -- into device memory, or straight into the caller's page-locked array
// The raw entry (rawdtw_detect_raw_begin) puts three launches in front, which turn windows of int16 DAC samples into the same dense
// pA chunks (ri_read_sig, src/rsig.cpp:216-224: convert, drop the outliers, keep the order):
//   k_raw_count   a wave per window: 16 bytes = 8 samples a lane and load, the kept samples counted -> s_len
//   k_ev_scan     the same scan, over s_len -> the chunks' sample offsets and the sample total, which stay on the device
//   k_raw_compact a wave per window: the same conversion, the kept samples ranked across the wave, gathered in LDS and written
//                 out lane by lane (coalesced) at the chunk's offset
// after which EvArgs.off means what it always means; k_ev_tstat, which takes the sample total from the host, reads it from device
// memory instead (EvArgs.n_dev) under a grid sized by the raw total.
// A RESIDENT detection (rawdtw_detect_resident_begin / _raw_resident_begin) runs the same launches and writes chunk k's normalised
// events into the context's event arena at dst_start[k] instead, where the seeding and the DTW read them: no event goes home.
//   k_ev_room     one workgroup behind k_ev_scan: a chunk with more events than its room, or a total above events_cap, raises the
//                 flag word; k_ev_events<true> then writes nothing anywhere (all or nothing, decided before the first store)
// A batch lasts as long as its longest chunk's serial chain: ~4 000 steps for the mapper's chunks; a whole read passed as one
// chunk works but costs its full length.
//
// Exactness: the library is built with -ffp-contract=off -fno-fast-math (and the pragma below says it again for this file);
// the contracted form names its fused operations (__fmaf_rn, __fma_rn), fp32 division is __fdiv_rn, and f64 `/` and sqrt
// lower to correctly rounded sequences on gfx950.  Denormals are not flushed.
//
// The host half (from DetectWs down): four begins share begin_checks and detect_enqueue, two ends share detect_end.  Where what lies in
// the workspace's device block and page-locked block, and the names of tot's words, is rawdtw_events_layout.h.
#include "rawdtw_capi.h"
#include "rawdtw_events.h"
#include "rawdtw_events_layout.h"

#include <algorithm>
#include <cfloat>

#pragma clang fp contract(off)

namespace rawdtw {
namespace {

constexpr uint32_t kW = 64;       // chunks a wave, and samples a tile
constexpr uint32_t kPad = kW + 1; // LDS row stride: a lane's row walk and the wave's column loads both hit 64 banks
constexpr uint32_t kEvLds = 2048; // k_ev_events: a chunk's events up to this many are summed out of LDS

struct EvArgs {
    const uint64_t *off; // n + 1 sample offsets, rebased to the uploaded samples (off[0] = 0)
    const float *sig;
    float *ps, *pss;     // chunk k: s_len + 1 entries from off[k] + k
    float *t1, *t2;      // chunk k: s_len entries from off[k]
    uint32_t *peaks;     // chunk k: s_len slots from off[k]
    uint32_t *npk, *nev; // per chunk: peaks emitted, events
    uint64_t *eoff;      // n + 1
    uint64_t *tot;       // [0] the total of events
    float *ev;           // the events, at eoff (device; n_samples entries)
    uint32_t n;
    uint64_t n_samples;
    const uint64_t *n_dev; // the raw entry: the kept samples' total, known to the device alone (n_samples then bounds it)
    const uint64_t *dst;   // a resident detection: per chunk, where its events go in the event arena; else null
    const uint64_t *flag;  // ... and its flag word (k_ev_room); else null
    rawdtw_event_opt_t opt;
};

__device__ __forceinline__ uint32_t wave_max(uint32_t x)
{
    for (int o = 32; o; o >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, o));
    return x;
}

// lane c's chunk start and length, as every lane sees them
__device__ __forceinline__ uint64_t lane_u64(uint64_t x, int c)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, c), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), c);
    return ((uint64_t)hi << 32) | lo;
}

// one 64 x 64 tile of a per-sample array into LDS (row c = chunk c, column = sample t0 + lane): all 64 loads are issued before
// the first LDS store, so a tile costs one memory latency rather than 64
__device__ __forceinline__ void load_tile(const float *src, uint64_t b, uint32_t len, uint32_t t0, float *tile)
{
    const uint32_t i = t0 + threadIdx.x;
    float v[kW];
#pragma unroll
    for (int c = 0; c < (int)kW; c++) {
        const uint64_t bc = lane_u64(b, c);
        const uint32_t lc = (uint32_t)__shfl((int)len, c);
        v[c] = i < lc ? src[bc + i] : 0.0f;
    }
#pragma unroll
    for (int c = 0; c < (int)kW; c++) tile[c * kPad + threadIdx.x] = v[c];
}

// revent.c:22-32
__global__ __launch_bounds__(64) void k_ev_prefix(EvArgs a)
{
    __shared__ float tx[kW * kPad], tp[kW * kPad], tq[kW * kPad];
    __shared__ uint64_t sb[kW];
    __shared__ uint32_t sl[kW];
    const uint32_t lane = threadIdx.x, c0 = blockIdx.x * kW, me = c0 + lane, nc = min(kW, a.n - c0);
    uint64_t b = 0;
    uint32_t len = 0;
    if (lane < nc) { b = a.off[me]; len = (uint32_t)(a.off[me + 1] - b); }
    sb[lane] = b; sl[lane] = len;
    const uint32_t most = wave_max(len);
    if (lane < nc) { a.ps[b + me] = 0.0f; a.pss[b + me] = 0.0f; }
    const bool fused = a.opt.contracted != 0;
    float s = 0.0f, q = 0.0f;
    __syncthreads();
    for (uint32_t t0 = 0; t0 < most; t0 += kW) {
        const uint32_t i = t0 + lane;
        load_tile(a.sig, b, len, t0, tx);
        __syncthreads();
        const uint32_t lim = len > t0 ? min(kW, len - t0) : 0u;
        for (uint32_t j = 0; j < lim; j++) {
            const float x = tx[lane * kPad + j];
            s = s + x;
            q = fused ? __fmaf_rn(x, x, q) : q + x * x;
            tp[lane * kPad + j] = s;
            tq[lane * kPad + j] = q;
        }
        __syncthreads();
        for (uint32_t c = 0; c < nc; c++)
            if (i < sl[c]) {
                const uint64_t d = sb[c] + c0 + c + 1 + i;
                a.ps[d] = tp[c * kPad + lane];
                a.pss[d] = tq[c * kPad + lane];
            }
        __syncthreads();
    }
}

// the largest k in [lo, hi] with off[k] <= j
__device__ __forceinline__ uint32_t chunk_of(const uint64_t *off, uint32_t lo, uint32_t hi, uint64_t j)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= j) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// revent.c:46-70 at position i of a chunk of n samples (P, Q: its prefix sums)
__device__ __forceinline__ float tstat_at(const float *P, const float *Q, uint32_t n, uint32_t i, uint32_t w, bool fused)
{
    if (n < 2 * w || w < 2 || i < w || i > n - w) return 0.0f;
    float s1 = P[i], q1 = Q[i];
    if (i > w) {
        s1 = s1 - P[i - w];
        q1 = q1 - Q[i - w];
    }
    const float s2 = P[i + w] - P[i], q2 = Q[i + w] - Q[i];
    const float wf = (float)w;
    const float m1 = __fdiv_rn(s1, wf), m2 = __fdiv_rn(s2, wf);
    float cv = fused ? __fmaf_rn(-m2, m2, __fmaf_rn(-m1, m1, __fdiv_rn(q1, wf)) + __fdiv_rn(q2, wf))
                     : __fdiv_rn(q1, wf) - m1 * m1 + __fdiv_rn(q2, wf) - m2 * m2;
    cv = fmaxf(cv, FLT_MIN);
    return (float)(fabs((double)(m2 - m1)) / sqrt((double)__fdiv_rn(cv, wf)));
}

__global__ __launch_bounds__(256) void k_ev_tstat(EvArgs a)
{
    __shared__ uint32_t kr[2];
    const uint64_t j0 = (uint64_t)blockIdx.x * 256, j = j0 + threadIdx.x;
    const uint64_t n_samples = a.n_dev ? a.n_dev[0] : a.n_samples;
    if (j0 >= n_samples) return; // (the whole workgroup: only the raw entry's grid reaches past the total)
    if (threadIdx.x == 0) kr[0] = chunk_of(a.off, 0, a.n - 1, j0);
    if (threadIdx.x == 1) kr[1] = chunk_of(a.off, 0, a.n - 1, min(j0 + 255, n_samples - 1));
    __syncthreads();
    if (j >= n_samples) return;
    const uint32_t k = chunk_of(a.off, kr[0], kr[1], j);
    const uint64_t b = a.off[k];
    const uint32_t len = (uint32_t)(a.off[k + 1] - b), i = (uint32_t)(j - b);
    const float *P = a.ps + b + k, *Q = a.pss + b + k;
    const bool fused = a.opt.contracted != 0;
    a.t1[j] = tstat_at(P, Q, len, i, a.opt.window_length1, fused);
    a.t2[j] = tstat_at(P, Q, len, i, a.opt.window_length2, fused);
}

struct Det {
    float pv;     // peak_value
    int pp;       // peak_pos
    uint32_t mt;  // masked_to
    bool valid;
};

// revent.c:77-138.  Peaks: at most s_len - 1 a chunk (a detector emits from step 2 on, at most once every window_length / 2 + 2
// >= 2 steps), so the chunk's s_len slots always suffice; the guard below only keeps a broken invariant inside the chunk.
__global__ __launch_bounds__(64) void k_ev_peaks(EvArgs a)
{
    __shared__ float ta[kW * kPad], tb[kW * kPad];
    const uint32_t lane = threadIdx.x, c0 = blockIdx.x * kW, me = c0 + lane, nc = min(kW, a.n - c0);
    uint64_t b = 0;
    uint32_t len = 0;
    if (lane < nc) { b = a.off[me]; len = (uint32_t)(a.off[me + 1] - b); }
    const uint32_t most = wave_max(len);
    const float th[2] = {a.opt.threshold1, a.opt.threshold2}, ph = a.opt.peak_height;
    const uint32_t wl[2] = {a.opt.window_length1, a.opt.window_length2};
    Det d[2] = {{FLT_MAX, -1, 0u, false}, {FLT_MAX, -1, 0u, false}};
    uint32_t cur = 0, inside = 0;
    uint32_t *pk = a.peaks + b;
    __syncthreads();
    for (uint32_t t0 = 0; t0 < most; t0 += kW) {
        load_tile(a.t1, b, len, t0, ta);
        load_tile(a.t2, b, len, t0, tb);
        __syncthreads();
        const uint32_t lim = len > t0 ? min(kW, len - t0) : 0u;
        for (uint32_t j = 0; j < lim; j++) {
            const uint32_t i = t0 + j;
            const float x[2] = {ta[lane * kPad + j], tb[lane * kPad + j]};
#pragma unroll
            for (int k = 0; k < 2; k++) {
                Det &D = d[k];
                if (D.mt >= i) continue;
                const float v = x[k];
                if (D.pp == -1) {
                    if (v < D.pv) D.pv = v;
                    else if (v - D.pv > ph) { D.pv = v; D.pp = (int)i; }
                } else {
                    if (v > D.pv) { D.pv = v; D.pp = (int)i; }
                    if (k == 0 && D.pv > th[0]) d[1] = Det{FLT_MAX, -1, (uint32_t)D.pp + wl[0], false};
                    if (D.pv - v > ph && D.pv > th[k]) D.valid = true;
                    if (D.valid && (i - (uint32_t)D.pp) > wl[k] / 2) {
                        const uint32_t p = (uint32_t)D.pp;
                        if (cur < len) pk[cur] = p;
                        if (cur >= 1 && p > 0 && p < len) inside++; // revent.c:145-147
                        cur++;
                        D.pp = -1;
                        D.pv = v;
                        D.valid = false;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (lane < nc) {
        a.npk[me] = min(cur, len);
        a.nev[me] = cur ? min(1 + inside, len) : 0; // revent.c:206: no peak, no events (the min: see above)
    }
}

// exclusive scan of the event counts
__global__ __launch_bounds__(1024) void k_ev_scan(const uint32_t *nev, uint32_t n, uint64_t *eoff, uint64_t *tot, uint64_t *h_eoff)
{
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (n + 1023ull) / 1024, lo = min((uint64_t)n, t * per), hi = min((uint64_t)n, lo + per);
    uint64_t s = 0;
    for (uint64_t k = lo; k < hi; k++) s += nev[k];
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = part[t] - s;
    for (uint64_t k = lo; k < hi; k++) {
        eoff[k] = run;
        if (h_eoff) h_eoff[k] = run;
        run += nev[k];
    }
    if (t == 1023) {
        eoff[n] = part[1023];
        if (h_eoff) h_eoff[n] = part[1023];
        tot[0] = part[1023];
    }
}

// A resident detection's go or no-go, before a single event is written: bit 0 a chunk has more events than its room in the arena,
// bit 1 the round's total is above the caller's events_cap.
__global__ __launch_bounds__(1024) void k_ev_room(const uint32_t *nev, const uint32_t *room, uint32_t n, const uint64_t *tot, uint64_t cap, uint64_t *flag)
{
    int over = 0;
    for (uint32_t k = threadIdx.x; k < n; k += 1024) over |= nev[k] > room[k] ? 1 : 0;
    over = __syncthreads_or(over);
    if (threadIdx.x == 0) flag[0] = (over ? 1u : 0u) | (tot[0] > cap ? 2u : 0u);
}

// revent.c:140-188.  Nothing is written unless the whole round's events fit below `bound` (the caller's events_cap, and the
// device array's size).  kArena (a resident detection): nothing is written either when k_ev_room raised the flag, and the
// normalised events go to out + a.dst[k] (the event arena; the host checked dst + room against its size, k_ev_room the count
// against the room); the raw means still go to the workspace.
template <bool kArena> __global__ __launch_bounds__(64) void k_ev_events(EvArgs a, uint64_t bound, float *out)
{
    __shared__ double stat[2];
    __shared__ float se[kEvLds]; // the chunk's events for the serial sums, when they fit
    if (a.tot[0] > bound) return;
    if (kArena && a.flag[0]) return;
    const uint32_t k = blockIdx.x, lane = threadIdx.x, nev = a.nev[k];
    if (!nev) return;
    const uint64_t b = a.off[k], eo = a.eoff[k];
    const uint32_t len = (uint32_t)(a.off[k + 1] - b);
    const float *P = a.ps + b + k;
    const uint32_t *pk = a.peaks + b;
    float *ev = a.ev + eo;
    for (uint32_t p = lane; p < nev; p += kW) {
        const uint32_t l = p ? pk[p - 1] : 0u, e = p + 1 < nev ? pk[p] : len;
        const float l_ps = p ? P[l] : 0.0f, l_peak = p ? (float)l : 0.0f;
        const float x = __fdiv_rn(P[e] - l_ps, (float)e - l_peak);
        ev[p] = x;
        if (nev <= kEvLds) se[p] = x;
    }
    __syncthreads();
    if (lane == 0) {
        const float *src = nev <= kEvLds ? se : ev;
        double sum = 0, sum2 = 0;
        for (uint32_t p = 0; p < nev; p++) {
            const float e = src[p];
            sum += (double)e;
            sum2 += (double)(e * e); // (the float product, widened)
        }
        const double mean = sum / (double)nev, m2 = sum2 / (double)nev;
        stat[0] = mean;
        stat[1] = sqrt(a.opt.contracted ? __fma_rn(-mean, mean, m2) : m2 - mean * mean);
    }
    __syncthreads();
    const double mean = stat[0], sd = stat[1];
    float *dst = kArena ? out + a.dst[k] : (out ? out : a.ev) + eo;
    for (uint32_t p = lane; p < nev; p += kW) dst[p] = (float)(((double)ev[p] - mean) / sd);
}

// ---- raw int16 samples in: ri_read_sig's conversion and filter (src/rsig.cpp:216-224) ----

struct RawArgs {
    const uint64_t *roff;         // n + 1 raw offsets, rebased to the uploaded samples (roff[0] = 0)
    const int16_t *raw;           // 16-byte aligned, readable up to the next multiple of 8 samples past roff[n]
    const rawdtw_channel_t *chan; // one a window
    uint32_t *cnt;                // per window: the kept samples (s_len)
    uint32_t *h_cnt;              // the caller's page-locked s_len, or null
    const uint64_t *off;          // n + 1 sample offsets of the kept samples (k_ev_scan over cnt)
    float *sig;                   // the kept pA samples, dense
};

// the 8 samples of the aligned group g (raw[8g .. 8g + 8)) to pA; bit j of the result: sample 8g + j lies in [s, e) and is kept.
// The three operations of rsig.cpp:216-224 and no other: the scale's division is the caller's.
__device__ __forceinline__ uint32_t convert8(const uint4 v, uint64_t g, uint64_t s, uint64_t e, float offset, float scale, float *pa)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t keep = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int16_t r = (int16_t)(w[j >> 1] >> (16 * (j & 1)));
        const float x = __fmul_rn(__fadd_rn((float)r, offset), scale);
        const uint64_t i = g * 8 + j;
        pa[j] = x;
        if (i >= s && i < e && x > 30.0f && x < 200.0f) keep |= 1u << j;
    }
    return keep;
}

// group g of a window that ends at e; a lane whose group lies past the end loads nothing
__device__ __forceinline__ uint4 load8(const int16_t *raw, uint64_t g, uint64_t e)
{
    return g * 8 < e ? *reinterpret_cast<const uint4 *>(raw + g * 8) : make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(64) void k_raw_count(RawArgs a)
{
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    const uint64_t s = a.roff[k], e = a.roff[k + 1];
    const rawdtw_channel_t ch = a.chan[k];
    const float scale = __fdiv_rn(ch.range, ch.digitisation);
    uint32_t c = 0;
    for (uint64_t g = s / 8 + lane; g * 8 < e; g += kW) {
        float pa[8];
        c += (uint32_t)__popc(convert8(load8(a.raw, g, e), g, s, e, ch.offset, scale, pa));
    }
    for (int o = 32; o; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
    if (lane == 0) {
        a.cnt[k] = c;
        if (a.h_cnt) a.h_cnt[k] = c;
    }
}

__global__ __launch_bounds__(64) void k_raw_compact(RawArgs a)
{
    __shared__ float out[kW * 8];
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    const uint64_t s = a.roff[k], e = a.roff[k + 1], b = a.off[k];
    const uint32_t len = (uint32_t)(a.off[k + 1] - b); // what k_raw_count counted: nothing is written past it
    const rawdtw_channel_t ch = a.chan[k];
    const float scale = __fdiv_rn(ch.range, ch.digitisation);
    float *dst = a.sig + b;
    uint32_t run = 0;
    uint4 cur = load8(a.raw, s / 8 + lane, e);
    for (uint64_t g0 = s / 8; g0 * 8 < e; g0 += kW) { // (the same trip count in every lane)
        const uint64_t g = g0 + lane;
        const uint4 nxt = load8(a.raw, g + kW, e); // the next piece is on its way while this one is ranked
        float pa[8];
        const uint32_t keep = g * 8 < e ? convert8(cur, g, s, e, ch.offset, scale, pa) : 0u;
        const uint32_t c = (uint32_t)__popc(keep);
        uint32_t incl = c; // kept samples of lanes 0 .. lane
#pragma unroll
        for (int o = 1; o < (int)kW; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
            if (lane >= (uint32_t)o) incl += t;
        }
        const uint32_t tot = (uint32_t)__shfl((int)incl, kW - 1);
        uint32_t p = incl - c;
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (keep >> j & 1) out[p++] = pa[j];
        __syncthreads();
        for (uint32_t i = lane; i < tot && run + i < len; i += kW) dst[run + i] = out[i];
        __syncthreads();
        run += tot;
        cur = nxt;
    }
}

struct DetectWs : capi::WsBlocks { // (the detection's own blocks: where what lies, rawdtw_events_layout.h)
    events::Layout at; // of the detection begun last
    // a detection begun and not ended
    bool pending = false, enqueued = false; // enqueued: it has work on the stream (else: no chunk, or no sample)
    bool raw = false, arena = false;        // the raw entries; a resident detection
    uint32_t n = 0;
    uint64_t n_samples = 0, cap = 0;
    // a plain detection: the caller's arrays, and which of them the device wrote itself
    bool direct_off = false, direct_ev = false, direct_slen = false;
    uint64_t *h_eoff = nullptr;
    float *h_ev = nullptr;
    uint32_t *h_slen = nullptr; // (the raw entry)
};

// the layout's consumers: a region of the device block, and of the pinned block
template <typename T> T *dev(const DetectWs &w, const events::Region &r) { return reinterpret_cast<T *>(static_cast<char *>(w.dev) + r.at); }
template <typename T> T *pinned(const DetectWs &w, const events::Region &r) { return reinterpret_cast<T *>(reinterpret_cast<char *>(w.pin) + r.at); }

// what a detection reads: pA chunks (sig), or raw windows with a channel each
struct Input {
    const float *sig = nullptr;
    const int16_t *raw = nullptr;
    const rawdtw_channel_t *chan = nullptr;
    uint32_t *s_len = nullptr;
    // a resident detection: the chunks' places and room in the context's event arena
    bool arena = false;
    const uint64_t *dst_start = nullptr;
    const uint32_t *room = nullptr;
};

} // namespace
} // namespace rawdtw

using namespace rawdtw;
using namespace rawdtw::capi;

struct rawdtw_detect_ws { DetectWs w; };

namespace {

// What the four begins refuse alike, in this order; the options resolved into *o.  null_arg: one of the entry's own arguments is null.
// The offsets' rule (check) and its sentence are the entry's.
int begin_checks(rawdtw_ctx *ctx, bool null_arg, bool arena, const rawdtw_event_opt_t *opt, rawdtw_event_opt_t *o,
                 int (*check)(uint32_t, const uint64_t *), uint32_t n_chunks, const uint64_t *off, const char *bad_offsets)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (null_arg) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (arena && !ctx->d_ev) return fail(ctx, RAWDTW_ERR_INVALID, "no event arena on this context (rawdtw_events_reserve, rawdtw_set_events_device)");
    if (ctx->detect_ws && ctx->detect_ws->w.pending) return fail(ctx, RAWDTW_ERR_INVALID, "a detection is begun on this context and not ended");
    if (events::resolve_opt(opt, o) != RAWDTW_OK) return fail(ctx, RAWDTW_ERR_INVALID, "a window length above 65535");
    if (check(n_chunks, off) != RAWDTW_OK) return fail(ctx, RAWDTW_ERR_INVALID, bad_offsets);
    return RAWDTW_OK;
}

const char *const kBadRawOffsets = "a window of 2^32 raw samples or more, or offsets that descend";

// everything after the entry's own checks: the workspace, the upload and the launches.  off: the caller's n + 1 offsets (of
// samples, or of raw samples), N = off[n] - off[0].
int detect_enqueue(rawdtw_ctx *ctx, const rawdtw_event_opt_t &o, uint32_t n_chunks, const uint64_t *off, const Input &in,
                   uint64_t *event_off, float *events, uint64_t events_cap)
{
    if (n_chunks >= 0x7fffffffu) return fail(ctx, RAWDTW_ERR_INVALID, "2^31 chunks or more");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool is_raw = in.raw != nullptr, arena = in.arena;
    const uint64_t n = n_chunks, N = off[n] - off[0];
    if (!ctx->detect_ws) ctx->detect_ws = new (std::nothrow) rawdtw_detect_ws;
    if (!ctx->detect_ws) return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    DetectWs &w = ctx->detect_ws->w;
    const events::Layout L = events::layout(is_raw, arena, n, N);
    if (const int st = blocks_reserve(ctx, w, L.need, L.pin_need, "detection workspace allocation failed")) return st;
    w.at = L;
    w.pending = true; w.n = n_chunks; w.n_samples = N; w.cap = events_cap;
    w.h_eoff = event_off; w.h_ev = events; w.h_slen = in.s_len;
    w.direct_off = w.direct_ev = w.direct_slen = false;
    w.arena = arena; w.enqueued = false; w.raw = is_raw;
    uint64_t *const h_off = pinned<uint64_t>(w, L.p_off), *const h_dst = pinned<uint64_t>(w, L.p_dst);
    uint32_t *const h_room = pinned<uint32_t>(w, L.p_room);
    for (uint64_t k = 0; k <= n; k++) h_off[k] = off[k] - off[0];
    if (arena) // the tables are checked in the very copy that goes up
        for (uint64_t k = 0; k < n; k++) {
            h_dst[k] = in.dst_start[k]; h_room[k] = in.room[k];
            if (h_dst[k] > ctx->n_ev || ctx->n_ev - h_dst[k] < h_room[k]) {
                w.pending = false;
                return fail(ctx, RAWDTW_ERR_RANGE, "a chunk's stretch (dst_start + room) is beyond the context's event arena");
            }
        }
    if (n == 0 || N == 0) return RAWDTW_OK; // (N == 0: every raw window is empty; the end fills the zeros)
    EvArgs a{};
    uint64_t *const d_off = dev<uint64_t>(w, L.off), *const d_dst = dev<uint64_t>(w, L.dst);
    float *const d_sig = dev<float>(w, L.sig);
    uint32_t *const d_room = dev<uint32_t>(w, L.room);
    a.off = d_off; a.sig = d_sig; a.ps = dev<float>(w, L.ps); a.pss = dev<float>(w, L.pss);
    a.t1 = dev<float>(w, L.t1); a.t2 = dev<float>(w, L.t2); a.peaks = dev<uint32_t>(w, L.peaks);
    a.npk = dev<uint32_t>(w, L.npk); a.nev = dev<uint32_t>(w, L.nev);
    a.eoff = dev<uint64_t>(w, L.eoff); a.tot = dev<uint64_t>(w, L.tot); a.ev = dev<float>(w, L.ev);
    a.n = n_chunks; a.n_samples = N; a.opt = o;
    a.n_dev = is_raw ? a.tot + events::kTotSamples : nullptr;
    if (arena) { a.dst = d_dst; a.flag = a.tot + events::kTotFlag; }
    uint64_t *dv_eoff = arena ? nullptr : static_cast<uint64_t *>(device_view(event_off, (n + 1) * 8));
    float *dv_ev = arena ? nullptr : static_cast<float *>(device_view(events, events_cap * 4));
    w.direct_off = dv_eoff != nullptr; w.direct_ev = dv_ev != nullptr;
    hipStream_t s = ctx->stream;
    auto undo = [&](int st) { w.pending = false; return st; };
    if (arena && (hipMemcpyAsync(d_dst, h_dst, n * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
                  hipMemcpyAsync(d_room, h_room, n * 4, hipMemcpyHostToDevice, s) != hipSuccess))
        return undo(hip_fail(ctx, hipGetLastError(), "detection upload"));
    const uint32_t waves = (uint32_t)((n + kW - 1) / kW);
    RawArgs r{};
    if (is_raw) {
        r.roff = dev<uint64_t>(w, L.roff); r.raw = dev<int16_t>(w, L.raw); r.chan = dev<rawdtw_channel_t>(w, L.chan);
        r.cnt = dev<uint32_t>(w, L.slen); r.off = d_off; r.sig = d_sig;
        r.h_cnt = arena ? nullptr : static_cast<uint32_t *>(device_view(in.s_len, n * 4));
        w.direct_slen = r.h_cnt != nullptr;
        if (hipMemcpyAsync(dev<uint64_t>(w, L.roff), h_off, (n + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(dev<rawdtw_channel_t>(w, L.chan), in.chan, n * sizeof(rawdtw_channel_t), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(dev<int16_t>(w, L.raw), in.raw + off[0], N * 2, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipEventRecord(w.ev0, s) != hipSuccess)
            return undo(hip_fail(ctx, hipGetLastError(), "detection upload"));
        hipLaunchKernelGGL(k_raw_count, dim3(n_chunks), dim3(kW), 0, s, r);
        hipLaunchKernelGGL(k_ev_scan, dim3(1), dim3(1024), 0, s, r.cnt, n_chunks, d_off, a.tot + events::kTotSamples, (uint64_t *)nullptr);
        hipLaunchKernelGGL(k_raw_compact, dim3(n_chunks), dim3(kW), 0, s, r);
    } else if (hipMemcpyAsync(d_off, h_off, (n + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
               hipMemcpyAsync(d_sig, in.sig + off[0], N * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
               hipEventRecord(w.ev0, s) != hipSuccess)
        return undo(hip_fail(ctx, hipGetLastError(), "detection upload"));
    hipLaunchKernelGGL(k_ev_prefix, dim3(waves), dim3(kW), 0, s, a);
    hipLaunchKernelGGL(k_ev_tstat, dim3((uint32_t)((N + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_ev_peaks, dim3(waves), dim3(kW), 0, s, a);
    hipLaunchKernelGGL(k_ev_scan, dim3(1), dim3(1024), 0, s, a.nev, n_chunks, a.eoff, a.tot + events::kTotEvents, dv_eoff);
    if (arena) {
        hipLaunchKernelGGL(k_ev_room, dim3(1), dim3(1024), 0, s, a.nev, d_room, n_chunks, a.tot + events::kTotEvents, events_cap, a.tot + events::kTotFlag);
        hipLaunchKernelGGL(k_ev_events<true>, dim3(n_chunks), dim3(kW), 0, s, a, N, ctx->d_ev);
    } else
        hipLaunchKernelGGL(k_ev_events<false>, dim3(n_chunks), dim3(kW), 0, s, a, std::min<uint64_t>(events_cap, N), dv_ev);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(w.ev1, s);
    if (e == hipSuccess) e = hipMemcpyAsync(pinned<uint64_t>(w, L.p_tot), a.tot + events::kTotEvents, 8, hipMemcpyDeviceToHost, s);
    if (arena) { // the flag, the counts and the raw entry's s_len: all that comes home
        if (e == hipSuccess) e = hipMemcpyAsync(pinned<uint64_t>(w, L.p_flag), a.tot + events::kTotFlag, 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(pinned<uint32_t>(w, L.p_nev), a.nev, n * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && is_raw) e = hipMemcpyAsync(pinned<uint32_t>(w, L.p_cnt), r.cnt, n * 4, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipEventRecord(w.done, s);
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "detection launches"));
    w.enqueued = true;
    return RAWDTW_OK;
}

// a resident end's arrays (null: the plain end, whose arrays the begin took)
struct ResidentOut {
    uint32_t *s_len, *ev_len;
    uint64_t *total;
};

// Both ends: the detection begun is of the end's kind, is ended, filled with zeros when nothing was enqueued, else waited for and
// timed; then what came home goes to the caller's arrays.
int detect_end(rawdtw_ctx *ctx, const ResidentOut *res, float *kernel_ms)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    DetectWs *const wp = ctx->detect_ws ? &ctx->detect_ws->w : nullptr;
    if (!wp || !wp->pending || (res && !wp->arena))
        return fail(ctx, RAWDTW_ERR_INVALID, res ? "no resident detection begun on this context" : "no detection begun on this context");
    if (!res && wp->arena) return fail(ctx, RAWDTW_ERR_INVALID, "the detection begun on this context is a resident one (rawdtw_detect_resident_end)");
    DetectWs &w = *wp;
    if (res && (!res->total || (w.n && !res->ev_len))) return fail(ctx, RAWDTW_ERR_INVALID, "null argument"); // (the detection stays begun)
    const uint64_t n = w.n;
    uint32_t *const s_len = res ? res->s_len : w.h_slen;
    w.pending = false;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (res) *res->total = 0;
    if (!w.enqueued) { // no chunk, or no sample
        if (res) std::fill_n(res->ev_len, n, 0u);
        else std::fill_n(w.h_eoff, n + 1, (uint64_t)0);
        if (s_len) std::fill_n(s_len, n, 0u);
        return RAWDTW_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(w.done)); // (the detection's own work: what the caller enqueued behind it, a seeding for one, goes on)
    if (kernel_ms) HIP_TRY(ctx, hipEventElapsedTime(kernel_ms, w.ev0, w.ev1));
    const uint64_t tot = *pinned<uint64_t>(w, w.at.p_tot);
    if (res) {
        const uint64_t *const h_off = pinned<uint64_t>(w, w.at.p_off), flag = *pinned<uint64_t>(w, w.at.p_flag);
        const uint32_t *const h_nev = pinned<uint32_t>(w, w.at.p_nev), *const h_cnt = pinned<uint32_t>(w, w.at.p_cnt);
        for (uint64_t k = 0; k < n; k++) {
            res->ev_len[k] = h_nev[k];
            if (s_len) s_len[k] = w.raw ? h_cnt[k] : (uint32_t)(h_off[k + 1] - h_off[k]);
        }
        *res->total = tot;
        if (flag & 1) return fail(ctx, RAWDTW_ERR_RANGE, "a chunk has more events than its room in the event arena (ev_len and the total are filled, nothing was written)");
        if (flag & 2) return fail(ctx, RAWDTW_ERR_RANGE, "events_cap is below the round's events (ev_len and the total are filled, nothing was written)");
        return RAWDTW_OK;
    }
    hipStream_t s = ctx->stream;
    if (!w.direct_off) {
        HIP_TRY(ctx, hipMemcpyAsync(w.h_eoff, dev<uint64_t>(w, w.at.eoff), (n + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    if (s_len && !w.direct_slen) {
        HIP_TRY(ctx, hipMemcpyAsync(s_len, dev<uint32_t>(w, w.at.slen), n * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    if (tot > w.cap) return fail(ctx, RAWDTW_ERR_RANGE, "events_cap is below the round's events (event_off is filled)");
    if (tot > w.n_samples) return fail(ctx, RAWDTW_ERR_DEVICE, "more events than samples");
    if (!w.direct_ev && tot) {
        HIP_TRY(ctx, hipMemcpyAsync(w.h_ev, dev<float>(w, w.at.ev), tot * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    return RAWDTW_OK;
}

} // namespace

extern "C" {

int rawdtw_detect_begin(rawdtw_ctx *ctx, const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *sig_off, const float *sig,
                        uint64_t *event_off, float *events, uint64_t events_cap)
{
    rawdtw_event_opt_t o;
    if (const int st = begin_checks(ctx, !sig_off || !event_off || (n_chunks && (!sig || !events)), false, opt, &o, events::check_offsets, n_chunks, sig_off,
                                    "an empty chunk (revent.c:24 asserts), a chunk of 2^32 samples or more, or offsets that descend"))
        return st;
    Input in;
    in.sig = sig;
    return detect_enqueue(ctx, o, n_chunks, sig_off, in, event_off, events, events_cap);
}

int rawdtw_detect_raw_begin(rawdtw_ctx *ctx, const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *raw_off, const int16_t *raw,
                            const rawdtw_channel_t *chan, uint32_t *s_len, uint64_t *event_off, float *events, uint64_t events_cap)
{
    rawdtw_event_opt_t o;
    if (const int st = begin_checks(ctx, !raw_off || !event_off || (n_chunks && (!raw || !chan || !s_len || !events)), false, opt, &o,
                                    events::check_raw_offsets, n_chunks, raw_off, kBadRawOffsets))
        return st;
    Input in;
    in.raw = raw; in.chan = chan; in.s_len = s_len;
    return detect_enqueue(ctx, o, n_chunks, raw_off, in, event_off, events, events_cap);
}

int rawdtw_detect_resident_begin(rawdtw_ctx *ctx, const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *sig_off, const float *sig,
                                 const uint64_t *dst_start, const uint32_t *room, uint64_t events_cap)
{
    rawdtw_event_opt_t o; // (an empty chunk is a read's all-outlier window: no events, as the raw entry has it)
    if (const int st = begin_checks(ctx, !sig_off || (n_chunks && (!sig || !dst_start || !room)), true, opt, &o, events::check_raw_offsets, n_chunks, sig_off,
                                    "a chunk of 2^32 samples or more, or offsets that descend"))
        return st;
    Input in;
    in.sig = sig; in.arena = true; in.dst_start = dst_start; in.room = room;
    return detect_enqueue(ctx, o, n_chunks, sig_off, in, nullptr, nullptr, events_cap);
}

int rawdtw_detect_raw_resident_begin(rawdtw_ctx *ctx, const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *raw_off, const int16_t *raw,
                                     const rawdtw_channel_t *chan, const uint64_t *dst_start, const uint32_t *room, uint64_t events_cap)
{
    rawdtw_event_opt_t o;
    if (const int st = begin_checks(ctx, !raw_off || (n_chunks && (!raw || !chan || !dst_start || !room)), true, opt, &o, events::check_raw_offsets, n_chunks,
                                    raw_off, kBadRawOffsets))
        return st;
    Input in;
    in.raw = raw; in.chan = chan; in.arena = true; in.dst_start = dst_start; in.room = room;
    return detect_enqueue(ctx, o, n_chunks, raw_off, in, nullptr, nullptr, events_cap);
}

int rawdtw_detect_resident_end(rawdtw_ctx *ctx, uint32_t *s_len, uint32_t *ev_len, uint64_t *total, float *kernel_ms)
{
    const ResidentOut res{s_len, ev_len, total};
    return detect_end(ctx, &res, kernel_ms);
}

int rawdtw_detect_end(rawdtw_ctx *ctx, float *kernel_ms) { return detect_end(ctx, nullptr, kernel_ms); }

} // extern "C"

namespace rawdtw { namespace capi {
bool detect_resident_view(const rawdtw_ctx *ctx, DetectView *v)
{
    const DetectWs *w = ctx && ctx->detect_ws ? &ctx->detect_ws->w : nullptr;
    if (!w || !w->pending || !w->arena) return false;
    *v = DetectView{w->enqueued, w->n, w->cap, w->n_samples, dev<uint64_t>(*w, w->at.eoff), dev<uint64_t>(*w, w->at.dst),
                    dev<uint64_t>(*w, w->at.tot) + events::kTotFlag};
    return true;
}

void detect_ws_free(rawdtw_ctx *ctx)
{
    if (!ctx || !ctx->detect_ws) return;
    blocks_release(ctx->detect_ws->w);
    delete ctx->detect_ws;
    ctx->detect_ws = nullptr;
}
} }
