// rawdtw_seed.hip -- seeding for a whole chunk round on the device: ri_sketch_reg (src/rsketch.c:223-274) and the lookup and hit
// loop of gen_chains (src/rmap.cpp:371-391), equal to the host restatement (rawdtw_seed_host.cpp) hit for hit and in its order.  The
// minimizer sketch (w > 0, ri_sketch_min, rsketch.c:146-221) is refused unless the context's "seed_minimizer" option is on; with it
// a fifth launch, k_seed_min, stands between the filter and the probe (below).
//
// One recurrence is serial per chunk: an event is compared with the last KEPT one.  Everything else is parallel.  Four launches:
//   k_seed_filter  a lane per chunk, 64 chunks a wave: events staged through LDS in 64 x 64 tiles (coalesced loads), each lane
//                  walks its own row and leaves every kept event's rank in its chunk; the tile then goes out row by row: a kept
//                  event's code and position land densely at the chunk's offset (stores nearly coalesced: ranks ascend)
//   k_seed_probe   a wave per chunk, a lane per kept event with e - 1 kept events in front of it: the last e codes packed, hashed
//                  (32-bit arithmetic, rawdtw_seed.h) and looked up in the table -- one 16-byte load a probe, uncoalesced by nature;
//                  what hides its latency is the number of independent probes in flight (every lane of every resident wave has
//                  one).  The element's hit count and its position-or-list word are stored; the wave sums the chunk's hits
//   k_seed_scan    one workgroup: exclusive scan of the chunks' hits -> hit_off and the total
//   k_seed_write   a wave per chunk, 64 elements a step: a wave scan of the counts places every element's hits; an element with
//                  up to kOwn hits is written by its own lane, a longer list by all 64 lanes together (no occurrence cap in the
//                  reference: a repeat gives one element thousands of positions, which one lane must not write alone).  One
//                  16-byte store a hit -- into device memory, or straight into the caller's page-locked array.  Nothing is
//                  written unless the round's total fits.
// With w > 0 ("seed_minimizer"): the filter has no RI_MASK_SIGNAL test (rsketch.c:172), and
//   k_seed_min     a wave per chunk: 64 e-mers a step are hashed by the lanes (e-mer m = the kept events m .. m + e - 1) into registers
//                  and an LDS ring of the last 512; the wave then walks them in order with the reference's window state (the minimum's
//                  hash and e-mer index, wave-uniform) and writes the chosen elements -- the hash, and the position of the e-mer's
//                  FIRST event -- densely at the chunk's offset, one slot an event at the most.  The probe then takes every element's
//                  hash as given; scan and write see the sketch's count and positions where they saw the kept events'.
// A RESIDENT seeding (rawdtw_seed_resident_begin) runs filter, probe and scan on events that are in the context's event arena already
// (a source start a chunk, apart from the dense workspace offset) and stops there: the hit counts go home, the per-element words
// stay in the workspace.  Two launches read them afterwards:
//   k_seed_write        on request (rawdtw_seed_resident_fetch): the 16-byte hits, as above
//   k_seed_write_chain  k_seed_write's shape, but what it lays down is the chaining's seed list (rmap.cpp:385-391 as the mapper's
//                       write_seeds restates it): 12-byte {sequence * 2 + strand, target, query + the chunk's start} records straight
//                       into rawdtw_chain.hip's workspace, behind the read's previous anchors -- the hits never exist in host memory
// A seeding DETECTED (rawdtw_seed_detected_begin) is a resident one enqueued straight behind a resident detection (rawdtw_events.hip)
// with no host step between: its dense offsets are the detection's event offsets, its source starts the detection's places in the
// arena, both copied on the device, and its workspace is sized by the detection's events_cap because no count has come home yet.
// Its launches are instantiations of their own (kGuard) that do nothing when the detection's flag word says it declined -- the
// offsets would then run past the workspace; the unguarded instantiations above never read that word.
// All three kinds are enqueued by one function, seed_enqueue, over one workspace layout (rawdtw_seed_layout.h).
#include "rawdtw_capi.h"
#include "rawdtw_seed.h"
#include "rawdtw_seed_layout.h"

#pragma clang fp contract(off)

namespace rawdtw {
namespace {

using seed::Slot;

constexpr uint32_t kW = 64;       // chunks a wave, and events a tile
constexpr uint32_t kPad = kW + 1; // LDS row stride (rawdtw_events.hip)
constexpr uint32_t kOwn = 4;      // hits an element's own lane writes
constexpr uint32_t kNone = ~0u;

struct SeedArgs {
    const uint64_t *off; // n + 1 event offsets, rebased to the uploaded events (off[0] = 0)
    const uint64_t *src; // resident: per chunk, where its events start in `ev` (the event arena); else unused (they start at off[k])
    const float *ev;
    uint32_t *code, *pos; // per chunk, dense from off[k]: the kept events' codes and positions
    uint32_t *kept;       // per chunk
    uint32_t *cnt;        // per kept event (at off[k] + rank): hits of the e-mer that ends there
    uint64_t *val;        // ... and the position (cnt == 1) or the list's start in the position array
    uint64_t *chits;      // per chunk: hits
    uint64_t *hoff;       // n + 1
    uint64_t *tot;        // [0] the total of hits
    const Slot *slots;
    const uint64_t *list;
    uint32_t log2_slots;
    uint32_t n, e, q, lq;
    const uint64_t *decl; // kGuard launches alone: the detection's flag word (non-zero: do nothing); never read by the others
};

__device__ __forceinline__ uint32_t wave_max(uint32_t x)
{
    for (int o = 32; o; o >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, o));
    return x;
}

__device__ __forceinline__ uint64_t lane_u64(uint64_t x, int c)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, c), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), c);
    return ((uint64_t)hi << 32) | lo;
}

// rsketch.c:242-247.  kSrc: the chunks' events are read from a.src[k] on (the event arena) rather than from the dense offset.
// kMask: the w == 0 rule (rsketch.c:243); without it ri_sketch_min's (rsketch.c:172), which keeps a masked value.
// kGuard: a detected seeding's instantiation (the whole workgroup leaves when the detection declined).
template <bool kSrc, bool kMask = true, bool kGuard = false> __global__ __launch_bounds__(64) void k_seed_filter(SeedArgs a)
{
    __shared__ float tx[kW * kPad];
    __shared__ uint32_t tr[kW * kPad];
    __shared__ uint64_t sb[kW];
    __shared__ uint32_t sl[kW];
    if (kGuard && a.decl[0]) return;
    const uint32_t lane = threadIdx.x, c0 = blockIdx.x * kW, me = c0 + lane, nc = min(kW, a.n - c0);
    uint64_t b = 0;
    uint32_t len = 0;
    if (lane < nc) { b = a.off[me]; len = (uint32_t)(a.off[me + 1] - b); }
    sb[lane] = b; sl[lane] = len;
    if (kSrc && lane < nc) b = a.src[me]; // (from here on b is where the lane's chunk is READ; the dense offsets are in sb)
    const uint32_t most = wave_max(len);
    float last = 0.0f;
    uint32_t rank = 0;
    __syncthreads();
    for (uint32_t t0 = 0; t0 < most; t0 += kW) {
        const uint32_t i = t0 + lane;
        {   // the tile: all 64 loads are issued before the first LDS store (one memory latency a tile)
            float v[kW];
#pragma unroll
            for (int c = 0; c < (int)kW; c++) {
                const uint64_t bc = lane_u64(b, c);
                const uint32_t lc = (uint32_t)__shfl((int)len, c);
                v[c] = i < lc ? a.ev[bc + i] : 0.0f;
            }
#pragma unroll
            for (int c = 0; c < (int)kW; c++) tx[c * kPad + lane] = v[c];
        }
        __syncthreads();
        const uint32_t lim = len > t0 ? min(kW, len - t0) : 0u;
        for (uint32_t j = 0; j < lim; j++) {
            const float x = tx[lane * kPad + j];
            const bool skip = kMask ? seed::skipped(x, last, t0 + j == 0) : seed::skipped_min(x, last, t0 + j == 0);
            tr[lane * kPad + j] = skip ? kNone : rank;
            // ev[l_sigpos] with l_sigpos = 0 until an event is kept (rsketch.c:233,243-245): a chunk whose event 0 is RI_MASK_SIGNAL
            // compares what follows with that value, not with nothing
            if (t0 + j == 0 || !skip) last = x;
            if (!skip) rank++;
        }
        __syncthreads();
        for (uint32_t c = 0; c < nc; c++)
            if (i < sl[c]) {
                const uint32_t r = tr[c * kPad + lane];
                if (r != kNone) { // r <= i < the chunk's length: inside the chunk's own stretch
                    a.code[sb[c] + r] = seed::code_of(__float_as_uint(tx[c * kPad + lane]), a.q, a.lq);
                    a.pos[sb[c] + r] = i;
                }
            }
        __syncthreads();
    }
    if (lane < nc) a.kept[me] = rank;
}

// ---- the minimizer sketch: ri_sketch_min's window (rsketch.c:193-219) over the filter's kept events ----
struct MinArgs {
    const uint64_t *off;                 // n + 1
    const uint32_t *code, *fpos, *fkept; // the filter's: per chunk dense from off[k], and the kept events a chunk
    uint32_t *hash, *pos, *count;        // the sketch: per chunk dense from off[k], and the elements a chunk
    uint64_t *over;                      // set when a chunk's sketch has more elements than the chunk has events
    uint32_t e, qb, w;
    const uint64_t *decl; // (as SeedArgs::decl)
};

constexpr uint32_t kRing = 512; // e-mer hashes kept in LDS: a window of up to 255 behind a step of 64

// The reference's buf[] at e-mer m is exactly the e-mers m - w + 1 .. m (slots below 0 are its empty UINT64_MAX entries, which lose
// every compare against a real one), so no ring of (x, y) is kept: the minimum is (hash, e-mer index), "buf_pos == min_pos" is "the
// minimum sits w e-mers back", and l = m + e.  x = hash << RI_HASH_SHIFT | span with one span: hashes compare as x does.  y differs
// exactly where the e-mer index does.
template <bool kGuard = false> __global__ __launch_bounds__(64) void k_seed_min(MinArgs a)
{
    __shared__ uint32_t ring[kRing];
    if (kGuard && a.decl[0]) return;
    const uint32_t k = blockIdx.x, lane = threadIdx.x, e = a.e, w = a.w;
    const uint64_t b = a.off[k];
    const uint32_t room = (uint32_t)(a.off[k + 1] - b), kept = a.fkept[k];
    const uint32_t M = kept >= e ? kept - e + 1 : 0; // e-mers
    const uint64_t mask_events = (1ull << (a.qb * e)) - 1;
    const uint64_t below = (1ull << lane) - 1;
    uint32_t out = 0;                // elements so far (wave-uniform, like the minimum)
    uint32_t mn_h = 0, mn_i = kNone; // kNone: no minimum yet (min.x == UINT64_MAX)
    auto push = [&](uint32_t h, uint32_t i) { // every store inside the chunk's own stretch of `room` slots
        if (lane == 0 && out < room) { a.hash[b + out] = h; a.pos[b + out] = a.fpos[b + i]; }
        out++;
    };
    // the e-mers lo .. hi whose hash is the minimum's, the minimum itself apart, oldest first (rsketch.c:195-198, 210-213)
    auto ties = [&](uint32_t lo, uint32_t hi) {
        for (uint32_t s0 = lo; s0 <= hi; s0 += kW) {
            const uint32_t i = s0 + lane;
            const bool f = i <= hi && i != mn_i && ring[i & (kRing - 1)] == mn_h;
            const unsigned long long bal = __ballot(f);
            const uint32_t at = out + (uint32_t)__popcll(bal & below);
            if (f && at < room) { a.hash[b + at] = mn_h; a.pos[b + at] = a.fpos[b + i]; }
            out += (uint32_t)__popcll(bal);
        }
    };
    for (uint32_t m0 = 0; m0 < M; m0 += kW) {
        uint32_t h = 0;
        if (m0 + lane < M) {
            uint64_t quant = 0;
            for (uint32_t j = 0; j < e; j++) quant = quant << a.qb | a.code[b + m0 + lane + j]; // (m + e - 1 < kept)
            h = seed::hash32((uint32_t)(quant & mask_events));
            ring[(m0 + lane) & (kRing - 1)] = h;
        }
        __syncthreads();
        const uint32_t lim = min(kW, M - m0);
        for (uint32_t j = 0; j < lim; j++) {
            const uint32_t m = m0 + j, hm = (uint32_t)__builtin_amdgcn_readlane((int)h, (int)j);
            if (m + 1 == w && mn_i != kNone) ties(0, m - 1); // the first window: the e-mers before this one
            if (mn_i == kNone || hm <= mn_h) { // a new minimum: the old one goes out
                if (m >= w && mn_i != kNone) push(mn_h, mn_i);
                mn_h = hm; mn_i = m;
            } else if (m - mn_i == w) { // the old minimum has left the window (so m >= w: every l >= w + e - 1 test holds)
                push(mn_h, mn_i);
                const uint32_t lo = m - w + 1; // >= 1
                uint64_t best = ~0ull;         // hash, then the NEWEST of equal ones (rsketch.c:206 ">="): ~index in the low half
                for (uint32_t s0 = lo; s0 <= m; s0 += kW) {
                    const uint32_t i = s0 + lane;
                    if (i <= m) best = min(best, (uint64_t)ring[i & (kRing - 1)] << 32 | (uint32_t)~i);
                }
                for (int o = 32; o; o >>= 1) best = min(best, lane_u64(best, (int)(lane ^ (uint32_t)o)));
                mn_h = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(best >> 32));
                mn_i = ~(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)best);
                ties(lo, m);
            }
        }
    }
    if (mn_i != kNone) push(mn_h, mn_i); // rsketch.c:218
    if (lane == 0) {
        a.count[k] = min(out, room);
        if (out > room) a.over[0] = 1;
    }
}

// rsketch.c:254-255, rawindex.cpp:256-273.  kGiven (w > 0): every element r < kept has its hash in a.code already (k_seed_min).
template <bool kGiven, bool kGuard = false> __global__ __launch_bounds__(64) void k_seed_probe(SeedArgs a)
{
    if (kGuard && a.decl[0]) return;
    const uint32_t k = blockIdx.x, lane = threadIdx.x, kept = a.kept[k], e = a.e, qb = a.lq + 2;
    const uint64_t b = a.off[k];
    const uint64_t mask_events = (1ull << (qb * e)) - 1;
    const uint32_t smask = (1u << a.log2_slots) - 1;
    uint64_t sum = 0;
    for (uint32_t r = lane; r < kept; r += kW) {
        uint32_t c = 0;
        uint64_t v = 0;
        if (kGiven || r + 1 >= e) {
            uint32_t h;
            if (kGiven) h = a.code[b + r];
            else {
                uint64_t quant = 0;
                for (uint32_t j = 0; j < e; j++) quant = quant << qb | a.code[b + r + 1 - e + j];
                h = seed::hash32((uint32_t)(quant & mask_events));
            }
            uint32_t at = seed::first_slot(h, a.log2_slots);
            for (uint32_t tries = 0; tries <= smask; tries++, at = (at + 1) & smask) { // (the table is at most half full: an empty slot ends it)
                const uint4 s = *reinterpret_cast<const uint4 *>(a.slots + at);
                if (s.y == 0) break;
                if (s.x == h) { c = s.y; v = (uint64_t)s.w << 32 | s.z; break; }
            }
        }
        a.cnt[b + r] = c;
        a.val[b + r] = v;
        sum += c;
    }
    for (int o = 32; o; o >>= 1) sum += lane_u64(sum, (int)(lane ^ (uint32_t)o));
    if (lane == 0) a.chits[k] = sum;
}

// exclusive scan of the chunks' hits (the shape of rawdtw_events.hip's k_ev_scan)
// (kGuard: `decl` is read, and the scan left out when it is set; without it `decl` is not looked at)
template <bool kGuard = false> __global__ __launch_bounds__(1024) void k_seed_scan(const uint64_t *cnt, uint32_t n, uint64_t *off, uint64_t *tot, uint64_t *h_off,
                                                                                   const uint64_t *decl)
{
    __shared__ uint64_t part[1024];
    if (kGuard && decl[0]) return;
    const uint32_t t = threadIdx.x;
    const uint64_t per = (n + 1023ull) / 1024, lo = min((uint64_t)n, t * per), hi = min((uint64_t)n, lo + per);
    uint64_t s = 0;
    for (uint64_t k = lo; k < hi; k++) s += cnt[k];
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
        off[k] = run;
        if (h_off) h_off[k] = run;
        run += cnt[k];
    }
    if (t == 1023) {
        off[n] = part[1023];
        if (h_off) h_off[n] = part[1023];
        tot[0] = part[1023];
    }
}

__device__ __forceinline__ uint4 hit_of(uint64_t y, uint32_t query)
{
    return make_uint4((uint32_t)(y >> 32), (uint32_t)(y & 1), (uint32_t)(y >> 1) & 0x7fffffffu, query); // rmap.cpp:387-388
}

// rmap.cpp:385-389.  Nothing is written unless the whole round's hits fit below `bound` (the caller's hits_cap, and the device
// array's size) and no chunk's sketch overflowed its stretch.
__global__ __launch_bounds__(64) void k_seed_write(SeedArgs a, uint64_t bound, uint4 *out)
{
    if (a.tot[0] > bound || a.tot[1]) return; // ([1]: k_seed_min's overflow flag, zero without it)
    const uint32_t k = blockIdx.x, lane = threadIdx.x, kept = a.kept[k];
    if (!a.chits[k]) return;
    const uint64_t b = a.off[k];
    uint4 *dst = out + a.hoff[k];
    uint64_t run = 0; // hits of the elements before this step
    for (uint32_t r0 = 0; r0 < kept; r0 += kW) { // (the same trip count in every lane)
        const uint32_t r = r0 + lane;
        const uint32_t c = r < kept ? a.cnt[b + r] : 0u;
        const uint64_t v = r < kept ? a.val[b + r] : 0ull;
        const uint32_t query = r < kept ? a.pos[b + r] : 0u;
        uint64_t incl = c; // (64 bits: 64 lists of up to 2^32 - 1 positions)
#pragma unroll
        for (int o = 1; o < (int)kW; o <<= 1) {
            const uint64_t t = lane_u64(incl, (int)((lane - (uint32_t)o) & (kW - 1)));
            if (lane >= (uint32_t)o) incl += t;
        }
        const uint64_t at = run + incl - c;
        if (c == 1) dst[at] = hit_of(v, query);
        else if (c <= kOwn)
            for (uint32_t s = 0; s < c; s++) dst[at + s] = hit_of(a.list[v + s], query);
        unsigned long long longs = __ballot(c > kOwn);
        while (longs) { // a long list: all 64 lanes, 64 consecutive 16-byte stores a step
            const int l = __ffsll(longs) - 1;
            longs &= longs - 1;
            const uint32_t lc = (uint32_t)__shfl((int)c, l), lquery = (uint32_t)__shfl((int)query, l);
            const uint64_t lv = lane_u64(v, l), lat = lane_u64(at, l);
            for (uint32_t s = lane; s < lc; s += kW) dst[lat + s] = hit_of(a.list[lv + s], lquery);
        }
        run += lane_u64(incl, kW - 1);
    }
}

// ---- the hits as the chaining's seed list ----
struct ChainDst {
    rawdtw_seed_t *seeds;          // the chaining workspace's seed list
    const uint64_t *seed_off;      // n + 1: read k's stretch
    const uint64_t *prev_off;      // n + 1: read k's previous anchors in `prev`, dense
    const rawdtw_seed_t *prev;
    const uint32_t *chunk_start;   // per read: reg->offset before this chunk (rmap.cpp:574)
    const uint8_t *sits_out;       // per read: the chunk is below min_events -- nothing is written (rmap.cpp:569-572)
    const uint32_t *prev_src;      // per read: RAWDTW_PREV_HOST, or the half of the kept chains' store its previous anchors lie in (null: all from `prev`)
    const char *store;             // the store (rawdtw_keep_layout.h)
    keep::Layout KL;
};

__device__ __forceinline__ rawdtw_seed_t seed_of(uint64_t y, uint32_t query)
{
    return rawdtw_seed_t{(uint32_t)(y >> 32) * 2u + (uint32_t)(y & 1), (uint32_t)(y >> 1) & 0x7fffffffu, query}; // rmap.cpp:387-391
}

// A wave a read: its previous anchors from the dense upload into the front of its stretch, then chunk k's hits behind them, placed as
// k_seed_write places them.  The host has checked seed_off[k + 1] - seed_off[k] == previous + hits against the counts this seeding
// sent home, so every store is inside the read's own stretch.
__global__ __launch_bounds__(64) void k_seed_write_chain(SeedArgs a, ChainDst d)
{
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (d.sits_out[k]) return;
    const uint64_t p0 = d.prev_off[k];
    uint32_t np = (uint32_t)(d.prev_off[k + 1] - p0);
    const rawdtw_seed_t *src = d.prev + p0;
    const uint64_t s0 = d.seed_off[k];
    rawdtw_seed_t *dst = d.seeds + s0;
    const uint32_t addr = d.prev_src ? d.prev_src[k] : RAWDTW_PREV_HOST;
    if (addr != RAWDTW_PREV_HOST) { // from the store: the half the keep launch of the round before wrote, earlier on this stream.  The host has
                                    // checked the stretch against its mirror of the count; the count is taken as at most a half and the stretch all the same
        np = (uint32_t)min(min((unsigned long long)*reinterpret_cast<const uint32_t *>(d.store + d.KL.count_at(addr)), (unsigned long long)d.KL.n_seeds),
                           (unsigned long long)(d.seed_off[k + 1] - s0));
        src = reinterpret_cast<const rawdtw_seed_t *>(d.store + d.KL.seeds_at(addr));
    }
    for (uint32_t i = lane; i < np; i += kW) dst[i] = src[i];
    if (!a.chits[k]) return;
    dst += np;
    const uint32_t kept = a.kept[k], start = d.chunk_start[k];
    const uint64_t b = a.off[k];
    uint64_t run = 0;
    for (uint32_t r0 = 0; r0 < kept; r0 += kW) { // (the same trip count in every lane)
        const uint32_t r = r0 + lane;
        const uint32_t c = r < kept ? a.cnt[b + r] : 0u;
        const uint64_t v = r < kept ? a.val[b + r] : 0ull;
        const uint32_t query = r < kept ? a.pos[b + r] + start : 0u;
        uint64_t incl = c;
#pragma unroll
        for (int o = 1; o < (int)kW; o <<= 1) {
            const uint64_t t = lane_u64(incl, (int)((lane - (uint32_t)o) & (kW - 1)));
            if (lane >= (uint32_t)o) incl += t;
        }
        const uint64_t at = run + incl - c;
        if (c == 1) dst[at] = seed_of(v, query);
        else if (c <= kOwn)
            for (uint32_t s = 0; s < c; s++) dst[at + s] = seed_of(a.list[v + s], query);
        unsigned long long longs = __ballot(c > kOwn);
        while (longs) { // a long list: all 64 lanes, 64 consecutive 12-byte stores a step
            const int l = __ffsll(longs) - 1;
            longs &= longs - 1;
            const uint32_t lc = (uint32_t)__shfl((int)c, l), lquery = (uint32_t)__shfl((int)query, l);
            const uint64_t lv = lane_u64(v, l), lat = lane_u64(at, l);
            for (uint32_t s = lane; s < lc; s += kW) dst[lat + s] = seed_of(a.list[lv + s], lquery);
        }
        run += lane_u64(incl, kW - 1);
    }
}

struct SeedWs : capi::WsBlocks { // (the seeding's own blocks: where what lies, rawdtw_seed_layout.h)
    // the table (rawdtw_seed_index_upload)
    uint64_t table_serial = 0; // the uploaded index's serial (0: none): the same index again is not uploaded twice
    Slot *d_slots = nullptr;
    uint64_t *d_list = nullptr;
    uint32_t log2_slots = 0;
    rawdtw_seed_pars_t pars{};
    bool has_table = false;
    void *d_hits = nullptr; // only for a caller whose hits are pageable
    size_t hits_bytes = 0;
    seed::Layout at; // of the seeding begun last
    // a seeding begun and not ended
    bool pending = false, direct_off = false, direct_hits = false;
    uint32_t n = 0;
    uint64_t n_events = 0, cap = 0;
    uint64_t *h_hoff = nullptr;
    rawdtw_seed_hit_t *h_hits = nullptr;
    const uint64_t *d_hoff = nullptr;
    // a resident seeding: begun (pending && resident), then ended and readable (ready) until the context's next seeding of either kind
    bool resident = false, ready = false;
    bool enqueued = false; // the resident seeding begun has work on the stream (its events are recorded)
    SeedArgs ra{};         // the launches' arguments: where the retained words are
    uint64_t r_total = 0;
};

// the layout's one consumer: a region of the device block, and of the pinned block (8-byte words)
template <typename T> T *dev(const SeedWs &w, const seed::Region &r) { return reinterpret_cast<T *>(static_cast<char *>(w.dev) + r.at); }
uint64_t *pinned(const SeedWs &w, const seed::Region &r) { return reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(w.pin) + r.at); }

// filter -> (min) -> probe -> scan on `a`.  With w > 0 the filter's output goes to `mn`'s inputs and `a` is re-pointed at the sketch: the
// launches behind (and whoever keeps `a`) see the sketch's elements where they saw the kept events.
template <bool kSrc, bool kGuard = false> void launch_seeding(SeedArgs &a, MinArgs mn, uint32_t w, hipStream_t s, uint64_t *dv_hoff)
{
    const dim3 tiles((a.n + kW - 1) / kW), chunks(a.n), wave(kW);
    if (w == 0) {
        hipLaunchKernelGGL((k_seed_filter<kSrc, true, kGuard>), tiles, wave, 0, s, a);
        hipLaunchKernelGGL((k_seed_probe<false, kGuard>), chunks, wave, 0, s, a);
    } else {
        SeedArgs f = a;
        f.code = const_cast<uint32_t *>(mn.code); f.pos = const_cast<uint32_t *>(mn.fpos); f.kept = const_cast<uint32_t *>(mn.fkept);
        hipLaunchKernelGGL((k_seed_filter<kSrc, false, kGuard>), tiles, wave, 0, s, f);
        hipLaunchKernelGGL(k_seed_min<kGuard>, chunks, wave, 0, s, mn);
        hipLaunchKernelGGL((k_seed_probe<true, kGuard>), chunks, wave, 0, s, a);
    }
    hipLaunchKernelGGL(k_seed_scan<kGuard>, dim3(1), dim3(1024), 0, s, a.chits, a.n, a.hoff, a.tot, dv_hoff, a.decl);
}

const char *const kDeclined = "the detection in front of this seeding declined (a chunk over its room, or events_cap below the round's events): nothing was seeded";
const char *const kOverflow = "a chunk's minimizer sketch has more elements than the chunk has events: seed this round on the host (rawdtw_seed_hits_host)";

} // namespace
} // namespace rawdtw

using namespace rawdtw;
using namespace rawdtw::capi;

struct rawdtw_seed_ws { SeedWs w; };

namespace {

SeedWs *ws_of(rawdtw_ctx *ctx)
{
    if (!ctx->seed_ws) ctx->seed_ws = new (std::nothrow) rawdtw_seed_ws;
    return ctx->seed_ws ? &ctx->seed_ws->w : nullptr;
}

// what every begin refuses alike: the context's workspace, or null with the refusal in *st
SeedWs *seedable(rawdtw_ctx *ctx, int *st)
{
    SeedWs *w = ctx->seed_ws ? &ctx->seed_ws->w : nullptr;
    if (!w || !w->has_table) *st = fail(ctx, RAWDTW_ERR_INVALID, "no seed index on this context (rawdtw_seed_index_upload)");
    else if (w->pending) *st = fail(ctx, RAWDTW_ERR_INVALID, "a seeding is begun on this context and not ended");
    else if (w->pars.w && !ctx->seed_minimizer) *st = fail(ctx, RAWDTW_ERR_UNSUPPORTED, "the minimizer sketch (w > 0) is seeded on the host (rawdtw_seed_hits_host)");
    else return w;
    return nullptr;
}

// where a seeding's offsets, source starts and events come from, and where its results go
struct Source {
    seed::Kind kind;
    uint32_t n = 0;  // chunks
    uint64_t N = 0;  // the events the workspace is sized for
    uint64_t *hit_off = nullptr;
    // plain: the caller's arrays, uploaded; the hits written on the way
    const uint64_t *event_off = nullptr;
    const float *events = nullptr;
    rawdtw_seed_hit_t *hits = nullptr;
    uint64_t hits_cap = 0;
    // resident: the caller's tables, uploaded; the events are in the arena
    const uint64_t *ev_start = nullptr;
    const uint32_t *ev_len = nullptr;
    // detected: the detection's device arrays and flag word; the host has seen no count
    DetectView det;
};

// Everything after an entry's own checks: the workspace, the state of a seeding begun, the upload (or the copies out of the detection's
// workspace, so that the retained words do not depend on it), the launches and what comes home.
int seed_enqueue(rawdtw_ctx *ctx, SeedWs &w, const Source &in)
{
    const bool plain = in.kind == seed::Kind::plain, detected = in.kind == seed::Kind::detected;
    const uint64_t n = in.n, N = in.N;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    w.ready = false; w.resident = false; // (the workspace is this seeding's from here on: an ended resident seeding's words are gone)
    const seed::Layout L = w.at = seed::layout(in.kind, n, N, w.pars.w != 0);
    if (const int st = blocks_reserve(ctx, w, L.need, L.pin_need, "seeding workspace allocation failed")) return st;
    uint64_t *dv_hoff = nullptr;
    uint4 *dv_hits = nullptr;
    if (plain) {
        dv_hoff = static_cast<uint64_t *>(device_view(in.hit_off, (n + 1) * 8));
        dv_hits = in.hits_cap ? static_cast<uint4 *>(device_view(in.hits, in.hits_cap * sizeof(rawdtw_seed_hit_t))) : nullptr;
        if (n && N && in.hits_cap && !dv_hits && w.hits_bytes < in.hits_cap * sizeof(rawdtw_seed_hit_t)) {
            if (w.d_hits) (void)hipFree(w.d_hits);
            w.d_hits = nullptr; w.hits_bytes = 0;
            if (hipMalloc(&w.d_hits, in.hits_cap * sizeof(rawdtw_seed_hit_t)) != hipSuccess) {
                (void)hipGetLastError();
                return fail(ctx, RAWDTW_ERR_OOM, "no device memory for hits_cap hits (page-locked hits need none)");
            }
            w.hits_bytes = in.hits_cap * sizeof(rawdtw_seed_hit_t);
        }
    }
    uint64_t *const h_off = pinned(w, L.p_off); // (plain and resident: the dense offsets going up)
    if (!plain) { // the tables going up; what comes home reads as zeros until it has
        uint64_t *const h_src = pinned(w, L.p_src), *const h_hoff = pinned(w, L.p_hoff);
        if (!detected) {
            h_off[0] = 0;
            for (uint64_t k = 0; k < n; k++) { h_off[k + 1] = h_off[k] + in.ev_len[k]; h_src[k] = in.ev_start[k]; }
        }
        for (uint64_t k = 0; k <= n; k++) h_hoff[k] = 0;
        *pinned(w, L.p_tot) = *pinned(w, L.p_over) = 0;
        if (detected) *pinned(w, L.p_decl) = 0;
        w.r_total = 0; w.enqueued = false;
    }
    w.pending = true; w.resident = !plain; w.n = in.n; w.n_events = N; w.cap = in.hits_cap;
    w.h_hoff = in.hit_off; w.h_hits = in.hits; w.direct_off = w.direct_hits = false;
    if (n == 0 || (plain && N == 0)) return RAWDTW_OK; // (nothing to enqueue: the ends fill the zeros)
    SeedArgs a{};
    uint64_t *const d_off = dev<uint64_t>(w, L.off), *const d_src = plain ? nullptr : dev<uint64_t>(w, L.src);
    a.off = d_off; a.src = d_src; a.ev = plain ? dev<float>(w, L.ev) : ctx->d_ev;
    a.code = dev<uint32_t>(w, L.code); a.pos = dev<uint32_t>(w, L.pos); a.cnt = dev<uint32_t>(w, L.cnt); a.val = dev<uint64_t>(w, L.val);
    a.kept = dev<uint32_t>(w, L.kept); a.chits = dev<uint64_t>(w, L.chits); a.hoff = dev<uint64_t>(w, L.hoff); a.tot = dev<uint64_t>(w, L.tot);
    a.n = in.n; a.e = w.pars.e; a.q = w.pars.q; a.lq = w.pars.lq;
    a.slots = w.d_slots; a.list = w.d_list; a.log2_slots = w.log2_slots;
    a.decl = detected ? in.det.d_flag : nullptr;
    MinArgs mn{};
    if (w.pars.w) { // the filter's three arrays become k_seed_min's input; the sketch takes their place in `a`
        mn = MinArgs{a.off, a.code, a.pos, a.kept, dev<uint32_t>(w, L.hash), dev<uint32_t>(w, L.spos), dev<uint32_t>(w, L.count), a.tot + 1,
                     w.pars.e, w.pars.lq + 2, w.pars.w, a.decl};
        a.code = mn.hash; a.pos = mn.pos; a.kept = mn.count;
    }
    w.d_hoff = a.hoff;
    if (plain) {
        for (uint64_t k = 0; k <= n; k++) h_off[k] = in.event_off[k] - in.event_off[0];
        w.direct_off = dv_hoff != nullptr; w.direct_hits = dv_hits != nullptr;
    } else { // what is kept (the sketch's words with w > 0) serves the unguarded k_seed_write / k_seed_write_chain, after an end that saw the flag clear
        w.ra = a; w.ra.decl = nullptr;
    }
    hipStream_t s = ctx->stream;
    auto undo = [&](int st) { w.pending = false; w.resident = false; return st; };
    hipError_t e = hipSuccess;
    if (!detected) {
        if (hipMemcpyAsync(d_off, h_off, (n + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
            (plain ? hipMemcpyAsync(dev<float>(w, L.ev), in.events + in.event_off[0], N * 4, hipMemcpyHostToDevice, s)
                   : hipMemcpyAsync(d_src, pinned(w, L.p_src), n * 8, hipMemcpyHostToDevice, s)) != hipSuccess ||
            hipMemsetAsync(a.tot, 0, 32, s) != hipSuccess || hipEventRecord(w.ev0, s) != hipSuccess)
            return undo(hip_fail(ctx, hipGetLastError(), "seeding upload"));
        if (plain) launch_seeding<false>(a, mn, w.pars.w, s, dv_hoff);
        else launch_seeding<true>(a, mn, w.pars.w, s, nullptr);
        if (in.hits_cap) hipLaunchKernelGGL(k_seed_write, dim3(in.n), dim3(kW), 0, s, a, in.hits_cap, dv_hits ? dv_hits : static_cast<uint4 *>(w.d_hits));
        e = hipGetLastError();
    } else { // (ev0 in front of the copies)
        if (hipEventRecord(w.ev0, s) != hipSuccess) return undo(hip_fail(ctx, hipGetLastError(), "seeding launches"));
        if (!in.det.enqueued) { // the detection had no sample: every chunk is empty -- zero offsets, counts and hits for whoever reads them
            e = hipMemsetAsync(w.dev, 0, L.need, s);
        } else {
            e = hipMemcpyAsync(d_off, in.det.d_eoff, (n + 1) * 8, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(d_src, in.det.d_dst, n * 8, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipMemsetAsync(a.tot, 0, 32, s);
            if (e == hipSuccess) e = hipMemcpyAsync(pinned(w, L.p_decl), in.det.d_flag, 8, hipMemcpyDeviceToHost, s);
            if (e != hipSuccess) return undo(hip_fail(ctx, e, "seeding upload"));
            launch_seeding<true, true>(a, mn, w.pars.w, s, nullptr);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipEventRecord(w.ev1, s);
    if (e == hipSuccess) // plain: the total and k_seed_min's overflow flag; resident: the hit offsets, then that flag alone
        e = plain ? hipMemcpyAsync(pinned(w, L.p_tot), a.tot, 16, hipMemcpyDeviceToHost, s) : hipMemcpyAsync(pinned(w, L.p_hoff), a.hoff, (n + 1) * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && !plain) e = hipMemcpyAsync(pinned(w, L.p_over), a.tot + 1, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipEventRecord(w.done, s);
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "seeding launches"));
    if (!plain) w.enqueued = true;
    return RAWDTW_OK;
}

} // namespace

extern "C" {

int rawdtw_seed_index_upload(rawdtw_ctx *ctx, const rawdtw_seed_index *six)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!six) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    SeedWs *w = ws_of(ctx);
    if (!w) return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    if (w->pending) return fail(ctx, RAWDTW_ERR_INVALID, "a seeding is begun on this context and not ended");
    if (w->has_table && w->table_serial == six->serial) return RAWDTW_OK; // (this very index is there already)
    if (six->resident) // (no host copy to send: the table lives, or lived, on the context that built it)
        return six->owner == ctx ? fail(ctx, RAWDTW_ERR_INVALID, "the resident index's table on this context has been replaced")
                                 : fail(ctx, RAWDTW_ERR_UNSUPPORTED, "a resident index has no host copy for another context: rawdtw_seed_index_fetch first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (an earlier table may still be read)
    if (w->d_slots) (void)hipFree(w->d_slots);
    if (w->d_list) (void)hipFree(w->d_list);
    w->d_slots = nullptr; w->d_list = nullptr; w->has_table = false; w->table_serial = 0;
    w->ready = false; // (an ended resident seeding's list words point into the table that went)
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&w->d_slots), std::max<size_t>(six->slots.size(), 1) * sizeof(Slot)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&w->d_list), std::max<size_t>(six->pos.size(), 1) * 8));
    if (!six->slots.empty()) HIP_TRY(ctx, hipMemcpyAsync(w->d_slots, six->slots.data(), six->slots.size() * sizeof(Slot), hipMemcpyHostToDevice, ctx->stream));
    else HIP_TRY(ctx, hipMemsetAsync(w->d_slots, 0, sizeof(Slot), ctx->stream));
    if (!six->pos.empty()) HIP_TRY(ctx, hipMemcpyAsync(w->d_list, six->pos.data(), six->pos.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (the index may be destroyed when this returns)
    w->log2_slots = six->slots.empty() ? 0 : six->log2_slots;
    w->pars = six->pars;
    w->table_serial = six->serial;
    w->has_table = true;
    return RAWDTW_OK;
}

int rawdtw_seed_index_fetch(rawdtw_ctx *ctx, rawdtw_seed_index *six)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!six) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (!six->resident) return RAWDTW_OK;
    const void *d_slots = nullptr;
    const uint64_t *d_list = nullptr;
    if (six->owner != ctx || !seed_table_view(ctx, six->serial, &d_slots, &d_list))
        return fail(ctx, RAWDTW_ERR_INVALID, "the resident index's table is not on this context (built elsewhere, or replaced since)");
    std::vector<Slot> slots;
    std::vector<uint64_t> pos;
    try { slots.resize((size_t)1 << six->log2_slots); pos.resize(six->n_list); } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(slots.data(), d_slots, slots.size() * sizeof(Slot), hipMemcpyDeviceToHost, ctx->stream));
    if (!pos.empty()) HIP_TRY(ctx, hipMemcpyAsync(pos.data(), d_list, pos.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    six->slots.swap(slots); six->pos.swap(pos);
    six->resident = false; // (an ordinary index from here on, under the same serial)
    return RAWDTW_OK;
}

int rawdtw_seed_begin(rawdtw_ctx *ctx, uint32_t n_chunks, const uint64_t *event_off, const float *events, uint64_t *hit_off,
                      rawdtw_seed_hit_t *hits, uint64_t hits_cap)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!hit_off || (n_chunks && !event_off)) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n_chunks >= 0x7fffffffu) return fail(ctx, RAWDTW_ERR_INVALID, "2^31 chunks or more");
    for (uint32_t k = 0; k < n_chunks; k++)
        if (event_off[k + 1] < event_off[k] || event_off[k + 1] - event_off[k] > 0xffffffffull)
            return fail(ctx, RAWDTW_ERR_INVALID, "a chunk of 2^32 events or more, or offsets that descend");
    Source in{seed::Kind::plain, n_chunks, n_chunks ? event_off[n_chunks] - event_off[0] : 0, hit_off};
    if ((in.N && !events) || (hits_cap && !hits)) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    int st = RAWDTW_OK;
    SeedWs *w = seedable(ctx, &st);
    if (!w) return st;
    in.event_off = event_off; in.events = events; in.hits = hits; in.hits_cap = hits_cap;
    return seed_enqueue(ctx, *w, in);
}

int rawdtw_seed_end(rawdtw_ctx *ctx, float *kernel_ms)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!ctx->seed_ws || !ctx->seed_ws->w.pending) return fail(ctx, RAWDTW_ERR_INVALID, "no seeding begun on this context");
    if (ctx->seed_ws->w.resident) return fail(ctx, RAWDTW_ERR_INVALID, "the seeding begun on this context is a resident one (rawdtw_seed_resident_end)");
    SeedWs &w = ctx->seed_ws->w;
    w.pending = false;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (w.n == 0 || w.n_events == 0) { // nothing was enqueued
        for (uint64_t k = 0; k <= w.n; k++) w.h_hoff[k] = 0;
        return RAWDTW_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipEventSynchronize(w.done)); // (the seeding's own work: what the caller enqueued behind it goes on)
    const uint64_t tot = *pinned(w, w.at.p_tot);
    if (!w.direct_off) {
        HIP_TRY(ctx, hipMemcpyAsync(w.h_hoff, w.d_hoff, ((uint64_t)w.n + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    if (kernel_ms) HIP_TRY(ctx, hipEventElapsedTime(kernel_ms, w.ev0, w.ev1));
    if (*pinned(w, w.at.p_over)) return fail(ctx, RAWDTW_ERR_UNSUPPORTED, kOverflow); // (no hit was written)
    if (tot > w.cap) return fail(ctx, RAWDTW_ERR_RANGE, "hits_cap is below the round's hits (hit_off is filled)");
    if (!w.direct_hits && tot) {
        HIP_TRY(ctx, hipMemcpyAsync(w.h_hits, w.d_hits, tot * sizeof(rawdtw_seed_hit_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    return RAWDTW_OK;
}

// ---- resident seeding: the events are in the arena, the hits stay in the workspace ----
int rawdtw_seed_resident_begin(rawdtw_ctx *ctx, uint32_t n_chunks, const uint64_t *ev_start, const uint32_t *ev_len, uint64_t *hit_off)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!hit_off || (n_chunks && (!ev_start || !ev_len))) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (n_chunks >= 0x7fffffffu) return fail(ctx, RAWDTW_ERR_INVALID, "2^31 chunks or more");
    int st = RAWDTW_OK;
    SeedWs *w = seedable(ctx, &st);
    if (!w) return st;
    Source in{seed::Kind::resident, n_chunks, 0, hit_off};
    for (uint32_t k = 0; k < n_chunks; k++) {
        if (ev_len[k] && (!ctx->d_ev || ev_start[k] > ctx->n_ev || ctx->n_ev - ev_start[k] < ev_len[k]))
            return fail(ctx, RAWDTW_ERR_RANGE, "a chunk outside the context's event arena");
        in.N += ev_len[k];
    }
    in.ev_start = ev_start; in.ev_len = ev_len;
    return seed_enqueue(ctx, *w, in);
}

// A resident seeding straight behind the context's resident detection: see the head of this file.
int rawdtw_seed_detected_begin(rawdtw_ctx *ctx, uint64_t *hit_off)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!hit_off) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    Source in{seed::Kind::detected, 0, 0, hit_off};
    if (!detect_resident_view(ctx, &in.det)) return fail(ctx, RAWDTW_ERR_INVALID, "no resident detection begun on this context and not ended");
    int st = RAWDTW_OK;
    SeedWs *w = seedable(ctx, &st);
    if (!w) return st;
    // the host has seen no count: room for as many events as the detection may write (its events_cap; never more than it has samples)
    in.n = in.det.n; in.N = in.det.enqueued ? std::min(in.det.cap, in.det.n_samples) : 0;
    return seed_enqueue(ctx, *w, in);
}

int rawdtw_seed_resident_end(rawdtw_ctx *ctx, float *kernel_ms)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!ctx->seed_ws || !ctx->seed_ws->w.pending || !ctx->seed_ws->w.resident)
        return fail(ctx, RAWDTW_ERR_INVALID, "no resident seeding begun on this context");
    SeedWs &w = ctx->seed_ws->w;
    w.pending = false; w.resident = false;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (w.n && w.enqueued) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipEventSynchronize(w.done));
        if (kernel_ms) HIP_TRY(ctx, hipEventElapsedTime(kernel_ms, w.ev0, w.ev1));
        if (w.at.p_decl.bytes && *pinned(w, w.at.p_decl)) return fail(ctx, RAWDTW_ERR_RANGE, kDeclined); // (nothing written, nothing readable)
        if (*pinned(w, w.at.p_over)) return fail(ctx, RAWDTW_ERR_UNSUPPORTED, kOverflow); // (nothing written, nothing readable)
    }
    const uint64_t *const r_hoff = pinned(w, w.at.p_hoff); // (the library's own host copy)
    for (uint64_t k = 0; k <= w.n; k++) w.h_hoff[k] = r_hoff[k];
    w.r_total = r_hoff[w.n];
    w.ready = true;
    return RAWDTW_OK;
}

int rawdtw_seed_resident_fetch(rawdtw_ctx *ctx, rawdtw_seed_hit_t *hits, uint64_t hits_cap)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    SeedWs *wp = ctx->seed_ws ? &ctx->seed_ws->w : nullptr;
    if (!wp || !wp->ready || wp->pending) return fail(ctx, RAWDTW_ERR_INVALID, "no ended resident seeding on this context");
    SeedWs &w = *wp;
    const uint64_t tot = w.r_total;
    if (tot > hits_cap) return fail(ctx, RAWDTW_ERR_RANGE, "hits_cap is below the seeding's hits");
    if (tot == 0) return RAWDTW_OK;
    if (!hits) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint4 *dv = static_cast<uint4 *>(device_view(hits, tot * sizeof(rawdtw_seed_hit_t)));
    if (!dv && w.hits_bytes < tot * sizeof(rawdtw_seed_hit_t)) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (an earlier seeding's copy may still read the old array)
        if (w.d_hits) (void)hipFree(w.d_hits);
        w.d_hits = nullptr; w.hits_bytes = 0;
        if (hipMalloc(&w.d_hits, tot * sizeof(rawdtw_seed_hit_t)) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, RAWDTW_ERR_OOM, "no device memory for the hits"); }
        w.hits_bytes = tot * sizeof(rawdtw_seed_hit_t);
    }
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_seed_write, dim3(w.n), dim3(kW), 0, s, w.ra, tot, dv ? dv : static_cast<uint4 *>(w.d_hits));
    HIP_TRY(ctx, hipGetLastError());
    if (!dv) HIP_TRY(ctx, hipMemcpyAsync(hits, w.d_hits, tot * sizeof(rawdtw_seed_hit_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return RAWDTW_OK;
}

} // extern "C"

namespace rawdtw { namespace capi {
const uint64_t *seed_resident_hit_off(const rawdtw_ctx *ctx, uint64_t *n_chunks)
{
    const SeedWs *w = ctx && ctx->seed_ws ? &ctx->seed_ws->w : nullptr;
    if (!w || !w->ready || w->pending) return nullptr;
    *n_chunks = w->n;
    return pinned(*w, w->at.p_hoff);
}

void seed_resident_write_chain(rawdtw_ctx *ctx, rawdtw_seed_t *d_seeds, const uint64_t *d_seed_off, const uint64_t *d_prev_off, const rawdtw_seed_t *d_prev,
                               const uint32_t *d_chunk_start, const uint8_t *d_sits_out, const uint32_t *d_prev_src)
{
    const SeedWs &w = ctx->seed_ws->w;
    KeepStoreView kv;
    if (!d_prev_src || !keep_store_view(ctx, &kv)) { d_prev_src = nullptr; kv = KeepStoreView{}; } // (the chaining's begin has checked that a source has its store)
    hipLaunchKernelGGL(k_seed_write_chain, dim3(w.n), dim3(kW), 0, ctx->stream, w.ra, ChainDst{d_seeds, d_seed_off, d_prev_off, d_prev, d_chunk_start, d_sits_out, d_prev_src, kv.store, kv.L});
}

int seed_table_installable(rawdtw_ctx *ctx)
{
    SeedWs *w = ws_of(ctx);
    if (!w) return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    if (w->pending) return fail(ctx, RAWDTW_ERR_INVALID, "a seeding is begun on this context and not ended");
    return RAWDTW_OK;
}

void seed_table_install(rawdtw_ctx *ctx, void *d_slots, uint64_t *d_list, uint32_t log2_slots, const rawdtw_seed_pars_t &pars, uint64_t serial)
{
    SeedWs &w = ctx->seed_ws->w; // (seed_table_installable made it)
    if (w.d_slots) (void)hipFree(w.d_slots);
    if (w.d_list) (void)hipFree(w.d_list);
    w.ready = false; // (an ended resident seeding's list words point into the table that went)
    w.d_slots = static_cast<Slot *>(d_slots); w.d_list = d_list;
    w.log2_slots = log2_slots; w.pars = pars; w.table_serial = serial; w.has_table = true;
}

bool seed_table_view(const rawdtw_ctx *ctx, uint64_t serial, const void **d_slots, const uint64_t **d_list)
{
    const SeedWs *w = ctx && ctx->seed_ws ? &ctx->seed_ws->w : nullptr;
    if (!w || !w->has_table || w->table_serial != serial) return false;
    *d_slots = w->d_slots; *d_list = w->d_list;
    return true;
}

void seed_ws_free(rawdtw_ctx *ctx)
{
    if (!ctx || !ctx->seed_ws) return;
    SeedWs &w = ctx->seed_ws->w;
    for (void *p : {(void *)w.d_slots, (void *)w.d_list, w.d_hits}) if (p) (void)hipFree(p);
    blocks_release(w);
    delete ctx->seed_ws;
    ctx->seed_ws = nullptr;
}
} }
