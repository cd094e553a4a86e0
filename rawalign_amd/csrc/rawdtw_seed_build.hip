// rawdtw_seed_build.hip -- the seed index of ri_idx_add / ri_idx_sort (src/rawindex.cpp:91-97, 194-246) built from the context's reference
// arena on the device: equal to what rawdtw_seed_index_build (rawdtw_seed_host.cpp) makes from the same arrays -- for w = 0 by
// rawdtw_seed_index_build_device, for any w by rawdtw_seed_index_build_device_min.
//
//   k_sb_filter   rsketch.c:242-247, the kept-event recurrence: serial a strand, so a wave a (sequence, strand).  64 events a step come
//                 in with one load; the recurrence runs over them out of scalar registers (v_readlane), alike in every lane; lane t then
//                 writes event t's position and code at its rank among the kept ones.
//   k_sb_emit     a thread a kept event with e - 1 kept events in front of it: the packed codes' hash32 and
//                 y = seq << 32 | pos << 1 | strand (rsketch.c:253; forward carries strand bit 1, rawindex.cpp:141-147).
//   w > 0         instead of k_sb_emit: k_sb_hash (a thread an e-mer: its hash), k_sb_min_count (a workgroup a tile of 256 e-mers of a
//                 strand, the hashes m0 - w .. m0 + 255 in LDS, a thread a step of rawdtw_seed_min.h, a count a tile), rocPRIM's exclusive
//                 scan of the tile counts (the total comes home and sizes the entries), k_sb_min_write (the same tiling; the elements at
//                 the tile's offset plus an in-block scan, y from the e-mer's FIRST kept event).  The filter runs without the mask test.
//   the sort      rocPRIM's device radix sort, twice: stable by y, then stable by hash -- the order of by_hash_then_position.
//   home          the sorted entries come home and fill_table (rawdtw_seed_host.cpp) builds the slots, as for every other index.
// skipped, code_of and hash32 are rawdtw_seed.h's: one definition.
//
// rawdtw_seed_index_build_resident: the same, with the two phases that were serial done otherwise and nothing coming home.
//   the filter    k_sb_next (a workgroup a tile of kFilterTile events: every element's next kept element, its chain's length and its
//                 chain's last value, by pointer doubling in LDS), k_sb_chain (a wave a strand, one step a tile: the tile's entry against
//                 the carried value, by ballot; the carry is one load at the entry), k_sb_mark (a wave a tile: the chain from the entry
//                 written out at the tile's place among the strand's kept events).  The step functions are rawdtw_seed_tile.h's.
//   the table     rocPRIM's select over the sorted entries (the groups' starts; their number comes home and sizes the slots), an
//                 exclusive scan of the lists' lengths, k_tb_insert (a thread a key: its rank into a 32-bit rank table by atomic minimum,
//                 rawdtw_seed_tile.h's step), k_tb_slots (a thread a slot: Slot{key, count, val} from the rank), and a second select that
//                 compacts the y of the groups with more than one entry into the lists.  The slots and lists stay: the context's table.
//
// The device block: per strand a row (below); per event of the arena a kept position and a kept code (4 bytes each); per entry a hash
// and a y, twice over for the sort's double buffer, and rocPRIM's temporary storage.  w > 0 adds a hash per event of the arena (4 bytes),
// a count and an offset a tile (8 bytes each), the scan's temporary storage and the word the write counts in.
#include "rawdtw_capi.h"
#include "rawdtw_seed.h"
#include "rawdtw_seed_min.h"
#include "rawdtw_seed_tile.h"

#include <algorithm>
#include <chrono>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace rawdtw {
namespace {

using namespace seed;

struct StrandRow {
    uint64_t arena_off; // where the strand starts in the arena
    uint64_t kept_base; // ... in the kept arrays
    uint64_t entry_base; // ... in the entries (filled behind the filter)
    uint32_t len, kept;
};

// kMask: the w == 0 rule (rsketch.c:243); without it ri_sketch_min's (rsketch.c:172), which keeps a masked value -- as k_seed_filter's.
template <bool kMask>
__global__ __launch_bounds__(64) void k_sb_filter(const float *__restrict__ arena, StrandRow *__restrict__ rows, uint32_t q, uint32_t lq,
                                                  uint32_t *__restrict__ kept_pos, uint32_t *__restrict__ kept_code)
{
    const uint32_t pair = blockIdx.x, lane = threadIdx.x;
    const StrandRow row = rows[pair];
    const float *s = arena + row.arena_off;
    const uint32_t n = row.len;
    uint32_t kept = 0;
    float last = n ? s[0] : 0.0f; // (s[last] with last = 0, as rsketch.c starts)
    float x_next = n ? (lane < n ? s[lane] : 0.0f) : 0.0f; // (a step's load is under way while the step before it runs)
    for (uint64_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t c = (uint32_t)(n - i0 < 64 ? n - i0 : 64);
        const float x = x_next;
        x_next = i0 + 64 + lane < n ? s[i0 + 64 + lane] : 0.0f;
        const int xb = __float_as_int(x);
        uint64_t mask = 0;
#pragma unroll
        for (uint32_t t = 0; t < 64; t++) {
            const float xt = __int_as_float(__builtin_amdgcn_readlane(xb, t));
            const bool skip = kMask ? skipped(xt, last, i0 + t == 0) : skipped_min(xt, last, i0 + t == 0);
            if (t < c && !skip) { last = xt; mask |= 1ull << t; }
        }
        if (mask >> lane & 1) {
            const uint64_t at = row.kept_base + kept + __popcll(mask & ((1ull << lane) - 1));
            kept_pos[at] = (uint32_t)(i0 + lane);
            kept_code[at] = code_of((uint32_t)xb, q, lq);
        }
        kept += __popcll(mask);
    }
    if (lane == 0) rows[pair].kept = kept;
}

__global__ __launch_bounds__(256) void k_sb_emit(const StrandRow *__restrict__ rows, const uint32_t *__restrict__ kept_pos,
                                                 const uint32_t *__restrict__ kept_code, uint32_t e, uint32_t quant_bit,
                                                 uint32_t *__restrict__ hash_out, uint64_t *__restrict__ y_out)
{
    const uint32_t pair = blockIdx.x;
    const StrandRow row = rows[pair];
    const uint32_t n = row.kept >= e ? row.kept - e + 1 : 0, strand = (pair & 1) ? 0u : 1u;
    const uint64_t mask_events = (1ULL << (quant_bit * e)) - 1, seq = pair >> 1;
    for (uint64_t t = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.y * blockDim.x) {
        uint64_t quant = 0;
        for (uint32_t a = 0; a < e; a++) quant = quant << quant_bit | kept_code[row.kept_base + t + a];
        quant &= mask_events;
        const uint32_t i = kept_pos[row.kept_base + t + e - 1];
        hash_out[row.entry_base + t] = hash32((uint32_t)quant);
        y_out[row.entry_base + t] = seq << 32 | (uint32_t)(i << 1) | strand;
    }
}

// ---- w > 0: the minimizer windows over whole strands.  rawdtw_seed_min.h's step makes every e-mer's elements a function of the hashes
// m - w .. m alone, so the selection is a count, a scan and a write with no serial part.  In these launches a row's entry_base is the
// strand's first tile among all strands' tiles.
constexpr uint32_t kMinTile = 256;                // e-mers a workgroup takes at a time; also the block size
constexpr uint32_t kMinStage = kMinTile + 256;    // the tile's hashes and the w <= 255 in front of them

__global__ __launch_bounds__(256) void k_sb_hash(const StrandRow *__restrict__ rows, const uint32_t *__restrict__ kept_code, uint32_t e,
                                                 uint32_t quant_bit, uint32_t *__restrict__ h_out)
{
    const StrandRow row = rows[blockIdx.x];
    const uint32_t n = row.kept >= e ? row.kept - e + 1 : 0;
    const uint64_t mask_events = (1ULL << (quant_bit * e)) - 1;
    for (uint64_t t = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.y * blockDim.x) {
        uint64_t quant = 0;
        for (uint32_t a = 0; a < e; a++) quant = quant << quant_bit | kept_code[row.kept_base + t + a];
        h_out[row.kept_base + t] = hash32((uint32_t)(quant & mask_events)); // (an array of its own: e-mer t reads codes t .. t + e - 1)
    }
}

// the hashes max(0, m0 - w) .. min(m0 + kMinTile, M) - 1 of a strand into LDS; returns the e-mer that sh[0] belongs to
__device__ inline uint32_t min_stage(const uint32_t *__restrict__ h, uint32_t M, uint32_t m0, uint32_t w, uint32_t *sh)
{
    const uint32_t base = m0 >= w ? m0 - w : 0, end = M - m0 < kMinTile ? M : m0 + kMinTile;
    for (uint32_t i = base + threadIdx.x; i < end; i += kMinTile) sh[i - base] = h[i];
    return base;
}

// the sum of v over the block's 256 threads, in every thread (part: 4 words of LDS; a barrier on either side)
__device__ inline uint32_t block_sum(uint32_t v, uint32_t *part)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void k_sb_min_count(const StrandRow *__restrict__ rows, const uint32_t *__restrict__ h, uint32_t e, uint32_t w,
                                                      uint64_t *__restrict__ tile_count)
{
    __shared__ uint32_t sh[kMinStage], part[4];
    const StrandRow row = rows[blockIdx.x];
    const uint32_t M = row.kept >= e ? row.kept - e + 1 : 0, tiles = (M + kMinTile - 1) / kMinTile;
    for (uint32_t t = blockIdx.y; t < tiles; t += gridDim.y) {
        const uint32_t m0 = t * kMinTile, m = m0 + threadIdx.x;
        const uint32_t base = min_stage(h + row.kept_base, M, m0, w, sh);
        __syncthreads();
        const uint32_t c = m < M ? min_step_count(sh, base, m, M, w) : 0; // (the strand's last e-mer: the end's one is in its count)
        const uint32_t sum = block_sum(c, part);
        if (threadIdx.x == 0) tile_count[row.entry_base + t] = sum;
        __syncthreads(); // (the next tile's staging writes sh and part)
    }
}

__global__ __launch_bounds__(256) void k_sb_min_write(const StrandRow *__restrict__ rows, const uint32_t *__restrict__ h,
                                                      const uint32_t *__restrict__ kept_pos, uint32_t e, uint32_t w,
                                                      const uint64_t *__restrict__ tile_off, uint64_t n_entries, uint32_t *__restrict__ hash_out,
                                                      uint64_t *__restrict__ y_out, unsigned long long *__restrict__ written)
{
    __shared__ uint32_t sh[kMinStage], scan[kMinTile], part[4];
    const uint32_t pair = blockIdx.x, strand = (pair & 1) ? 0u : 1u;
    const StrandRow row = rows[pair];
    const uint32_t M = row.kept >= e ? row.kept - e + 1 : 0, tiles = (M + kMinTile - 1) / kMinTile;
    const uint64_t seq = pair >> 1;
    uint32_t done = 0;
    for (uint32_t t = blockIdx.y; t < tiles; t += gridDim.y) {
        const uint32_t m0 = t * kMinTile, m = m0 + threadIdx.x;
        const uint32_t base = min_stage(h + row.kept_base, M, m0, w, sh);
        __syncthreads();
        const uint32_t c = m < M ? min_step_count(sh, base, m, M, w) : 0;
        scan[threadIdx.x] = c; // the thread's place: an inclusive scan of the counts, less its own
        __syncthreads();
        for (uint32_t d = 1; d < kMinTile; d <<= 1) {
            const uint32_t v = threadIdx.x >= d ? scan[threadIdx.x - d] : 0;
            __syncthreads();
            scan[threadIdx.x] += v;
            __syncthreads();
        }
        uint64_t at = tile_off[row.entry_base + t] + (scan[threadIdx.x] - c);
        if (c)
            min_step_walk(MinHashes{sh, base}, m, M, w, [&](uint32_t i) {
                if (at < n_entries) { // (the scan's total sized the arrays: a place past them would be a fault of this file, told by `written`)
                    hash_out[at] = sh[i - base];
                    y_out[at] = seq << 32 | (uint32_t)(kept_pos[row.kept_base + i] << 1) | strand;
                    done++;
                }
                at++;
            });
        __syncthreads(); // (the next tile's staging writes sh and scan)
    }
    const uint32_t sum = block_sum(done, part);
    if (threadIdx.x == 0 && sum) atomicAdd(written, (unsigned long long)sum);
}


// ---- the filter without a chain over events (rawdtw_seed_tile.h).  Per event of the arena, at the kept arrays' index: a word
// next | steps << 16 (next: the tile-local index of the next kept element, the tile's length for none; steps: the elements behind it on
// its chain) and the value of its chain's last element.  Per tile: its entry (kNoEntry: it keeps nothing) and the strand's kept events in
// front of it.  tile0[pair]: the strand's first tile among all strands' tiles.
constexpr uint32_t kTileGridY = 1024;              // blocks a strand in k_sb_next and k_sb_mark: a strand of more tiles takes the grid-stride loop
constexpr uint32_t kNextPer = kFilterTile / 256;   // elements a thread of k_sb_next

template <bool kMask>
__global__ __launch_bounds__(256) void k_sb_next(const float *__restrict__ arena, const StrandRow *__restrict__ rows, uint32_t *__restrict__ nc,
                                                 float *__restrict__ xe)
{
    __shared__ float x[kFilterTile];
    __shared__ uint16_t jmp[kFilterTile], cnt[kFilterTile];
    const StrandRow row = rows[blockIdx.x];
    const uint32_t tiles = (uint32_t)(((uint64_t)row.len + kFilterTile - 1) / kFilterTile);
    for (uint32_t t = blockIdx.y; t < tiles; t += gridDim.y) {
        const uint64_t i0 = (uint64_t)t * kFilterTile;
        const uint32_t n = (uint32_t)(row.len - i0 < kFilterTile ? row.len - i0 : kFilterTile);
        for (uint32_t j = threadIdx.x; j < n; j += 256) x[j] = arena[row.arena_off + i0 + j];
        __syncthreads();
        uint32_t nx[kNextPer];
#pragma unroll
        for (uint32_t k = 0; k < kNextPer; k++) {
            const uint32_t j = threadIdx.x + 256 * k;
            if (j < n) {
                nx[k] = tile_next<kMask>(x, j, n);
                jmp[j] = (uint16_t)(nx[k] < n ? nx[k] : j); // (the chain's last element points at itself and counts no step)
                cnt[j] = nx[k] < n ? 1 : 0;
            }
        }
        __syncthreads();
        // pointer doubling: after the round with d, jmp is 2d steps on (or the chain's last) and cnt the steps taken
        for (uint32_t d = 1; d < n; d <<= 1) {
            uint16_t a[kNextPer], c[kNextPer];
#pragma unroll
            for (uint32_t k = 0; k < kNextPer; k++) {
                const uint32_t j = threadIdx.x + 256 * k;
                if (j < n) { const uint32_t m = jmp[j]; a[k] = jmp[m]; c[k] = (uint16_t)(cnt[j] + cnt[m]); }
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < kNextPer; k++) {
                const uint32_t j = threadIdx.x + 256 * k;
                if (j < n) { jmp[j] = a[k]; cnt[j] = c[k]; }
            }
            __syncthreads();
        }
#pragma unroll
        for (uint32_t k = 0; k < kNextPer; k++) {
            const uint32_t j = threadIdx.x + 256 * k;
            if (j < n) {
                nc[row.kept_base + i0 + j] = nx[k] | (uint32_t)cnt[j] << 16;
                xe[row.kept_base + i0 + j] = x[jmp[j]];
            }
        }
        __syncthreads(); // (the next tile's staging writes x, jmp and cnt)
    }
}

template <bool kMask>
__global__ __launch_bounds__(64) void k_sb_chain(const float *__restrict__ arena, StrandRow *__restrict__ rows, const uint64_t *__restrict__ tile0,
                                                 const uint32_t *__restrict__ nc, const float *__restrict__ xe, uint32_t *__restrict__ tile_entry,
                                                 uint32_t *__restrict__ tile_kept)
{
    const uint32_t pair = blockIdx.x, lane = threadIdx.x;
    const StrandRow row = rows[pair];
    const float *s = arena + row.arena_off;
    const uint32_t n = row.len, tiles = (uint32_t)(((uint64_t)n + kFilterTile - 1) / kFilterTile);
    const uint64_t tb = tile0[pair];
    uint32_t kept = 0;
    float v = n ? s[0] : 0.0f; // (s[last] with last = 0, as rsketch.c starts)
    float x_next = lane < n ? s[lane] : 0.0f; // (a tile's first 64 values are under way while the tile before it is stepped)
    for (uint32_t t = 0; t < tiles; t++) {
        const uint64_t i0 = (uint64_t)t * kFilterTile;
        const uint32_t tn = (uint32_t)(n - i0 < kFilterTile ? n - i0 : kFilterTile);
        float x = x_next;
        x_next = i0 + kFilterTile + lane < n ? s[i0 + kFilterTile + lane] : 0.0f;
        uint32_t entry = kNoEntry;
        for (uint32_t c0 = 0; c0 < tn; c0 += 64) {
            if (c0) x = c0 + lane < tn ? s[i0 + c0 + lane] : 0.0f;
            const uint64_t b = __ballot(c0 + lane < tn && tile_enters<kMask>(x, v, i0 + c0 + lane == 0));
            if (b) { entry = c0 + (uint32_t)__ffsll((long long)b) - 1; break; }
        }
        if (lane == 0) { tile_entry[tb + t] = entry; tile_kept[tb + t] = kept; }
        if (entry != kNoEntry) { // the one dependent load of a step: the entry's chain, its length and its last value
            const uint64_t at = row.kept_base + i0 + entry;
            kept += (nc[at] >> 16) + 1;
            v = xe[at];
        }
    }
    if (lane == 0) rows[pair].kept = kept;
}

__global__ __launch_bounds__(64) void k_sb_mark(const float *__restrict__ arena, const StrandRow *__restrict__ rows, const uint64_t *__restrict__ tile0,
                                                const uint32_t *__restrict__ nc, const uint32_t *__restrict__ tile_entry,
                                                const uint32_t *__restrict__ tile_kept, uint32_t q, uint32_t lq, uint32_t *__restrict__ kept_pos,
                                                uint32_t *__restrict__ kept_code)
{
    __shared__ uint16_t nx[kFilterTile], list[kFilterTile];
    __shared__ uint32_t on_chain;
    const StrandRow row = rows[blockIdx.x];
    const uint32_t tiles = (uint32_t)(((uint64_t)row.len + kFilterTile - 1) / kFilterTile), lane = threadIdx.x;
    const uint64_t tb = tile0[blockIdx.x];
    for (uint32_t t = blockIdx.y; t < tiles; t += gridDim.y) {
        const uint32_t entry = tile_entry[tb + t];
        if (entry == kNoEntry) continue; // (alike in the whole wave)
        const uint64_t i0 = (uint64_t)t * kFilterTile;
        const uint32_t tn = (uint32_t)(row.len - i0 < kFilterTile ? row.len - i0 : kFilterTile);
        for (uint32_t j = lane; j < tn; j += 64) nx[j] = (uint16_t)(nc[row.kept_base + i0 + j] & 0xffffu);
        __syncthreads();
        if (lane == 0) { // the walk: next is ahead of its element, so at most tn steps
            uint32_t r = 0;
            for (uint32_t j = entry; j < tn && r < tn; j = nx[j]) list[r++] = (uint16_t)j;
            on_chain = r;
        }
        __syncthreads();
        const uint64_t at = row.kept_base + tile_kept[tb + t]; // (the kept events in front of the tile are no more than the events in front of it)
        for (uint32_t r = lane; r < on_chain; r += 64) {
            const uint64_t i = i0 + list[r];
            kept_pos[at + r] = (uint32_t)i;
            kept_code[at + r] = code_of((uint32_t)__float_as_int(arena[row.arena_off + i]), q, lq);
        }
        __syncthreads(); // (the next tile's staging writes nx, list and on_chain)
    }
}

// ---- the table's slots and lists from the sorted entries.  A group: the entries of one hash; its rank: its place among the groups.
struct GroupHead { // entry i starts a group
    const uint32_t *h;
    __device__ bool operator()(uint64_t i) const { return i == 0 || h[i] != h[i - 1]; }
};
struct InList { // entry i belongs to a group of more than one entry
    const uint32_t *h;
    uint64_t n;
    __device__ uint8_t operator()(uint64_t i) const { return ((i && h[i] == h[i - 1]) || (i + 1 < n && h[i] == h[i + 1])) ? 1 : 0; }
};
struct ListLen { // the list words of group r (0 for a single position, and behind the last group)
    const uint64_t *start;
    uint64_t n_keys, n;
    __device__ uint64_t operator()(uint64_t r) const
    {
        if (r >= n_keys) return 0;
        const uint64_t c = (r + 1 < n_keys ? start[r + 1] : n) - start[r];
        return c > 1 ? c : 0;
    }
};

// flags[0]: probes that found no free slot in a whole turn of the table (a fault of this file); flags[1]: a group of 2^32 entries or
// more; flags[2]: the keys not in their home slot
__global__ __launch_bounds__(256) void k_tb_insert(const uint32_t *__restrict__ hash, const uint64_t *__restrict__ start, uint32_t n_keys, uint32_t lg,
                                                   uint32_t *__restrict__ tab, unsigned long long *__restrict__ flags)
{
    const uint32_t mask = (1u << lg) - 1u;
    auto amin = [tab](uint32_t at, uint32_t r) { return atomicMin(&tab[at], r); }; // (device scope)
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n_keys; k += (uint64_t)gridDim.x * 256) {
        uint32_t r = (uint32_t)k, at = first_slot(hash[start[k]], lg), turns = 0;
        while (!table_insert_step(amin, r, at, mask))
            if (turns++ == mask) { atomicAdd(&flags[0], 1ull); break; } // (load <= 0.5: never)
    }
}

__global__ __launch_bounds__(256) void k_tb_slots(const uint32_t *__restrict__ hash, const uint64_t *__restrict__ y, const uint64_t *__restrict__ start,
                                                  const uint64_t *__restrict__ list_off, uint64_t n_keys, uint64_t n, uint32_t lg,
                                                  const uint32_t *__restrict__ tab, Slot *__restrict__ slots, unsigned long long *__restrict__ flags)
{
    __shared__ uint32_t part[4];
    const uint64_t n_slots = 1ull << lg;
    uint32_t away = 0;
    for (uint64_t at = (uint64_t)blockIdx.x * 256 + threadIdx.x; at < n_slots; at += (uint64_t)gridDim.x * 256) {
        const uint32_t r = tab[at];
        Slot s{0, 0, 0};
        if (r != kNoEntry) {
            const uint64_t from = start[r], c = (r + 1 < n_keys ? start[r + 1] : n) - from;
            if (c > 0xffffffffull) atomicAdd(&flags[1], 1ull);
            s.key = hash[from]; s.count = (uint32_t)c;
            s.val = c == 1 ? y[from] : list_off[r];
            away += first_slot(s.key, lg) != (uint32_t)at;
        }
        slots[at] = s;
    }
    const uint32_t sum = block_sum(away, part);
    if (threadIdx.x == 0 && sum) atomicAdd(&flags[2], (unsigned long long)sum);
}

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

} // namespace
} // namespace rawdtw

using namespace rawdtw;
using namespace rawdtw::capi;
using namespace rawdtw::seed;

// The table of n sorted entries in device memory, built there: on success the slots and lists are the caller's to install or free.
struct DeviceTable {
    Slot *d_slots = nullptr;
    uint64_t *d_list = nullptr;
    uint32_t lg = 0;
    uint64_t n_keys = 0, n_list = 0, displaced = 0;
    float ms = 0.f;
};

static int table_on_device(rawdtw_ctx *ctx, const uint32_t *d_hash, const uint64_t *d_y, uint64_t n, DeviceTable *out)
{
    DeviceTable t;
    uint64_t *d_start = nullptr, *d_loff = nullptr, *d_count = nullptr;
    unsigned long long *d_flags = nullptr;
    uint32_t *d_tab = nullptr;
    void *d_tmp = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    unsigned long long flags[3] = {0, 0, 0};
    int st = RAWDTW_OK;
    hipError_t e = hipSuccess;
    auto hip_ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
    hipStream_t s = ctx->stream;
    const rocprim::counting_iterator<uint64_t> index(0);
    for (int i = 0; i < 2; i++) hip_ok(hipEventCreate(&ev[i]));
    hip_ok(hipMalloc((void **)&d_count, 16));
    hip_ok(hipMalloc((void **)&d_flags, sizeof(flags)));
    if (e == hipSuccess) hip_ok(hipMemsetAsync(d_flags, 0, sizeof(flags), s));
    if (e == hipSuccess) hip_ok(hipEventRecord(ev[0], s));
    if (n) { // the groups' starts, compacted in order; their number comes home
        size_t bytes = 0;
        hip_ok(hipMalloc((void **)&d_start, n * 8));
        if (e == hipSuccess) hip_ok(rocprim::select(nullptr, bytes, index, d_start, d_count, (size_t)n, GroupHead{d_hash}, s));
        if (e == hipSuccess) hip_ok(hipMalloc(&d_tmp, std::max<size_t>(bytes, 16)));
        if (e == hipSuccess) hip_ok(rocprim::select(d_tmp, bytes, index, d_start, d_count, (size_t)n, GroupHead{d_hash}, s));
        if (e == hipSuccess) hip_ok(hipMemcpyAsync(&t.n_keys, d_count, 8, hipMemcpyDeviceToHost, s));
        if (e == hipSuccess) hip_ok(hipStreamSynchronize(s));
        if (d_tmp) { (void)hipFree(d_tmp); d_tmp = nullptr; }
    }
    if (e == hipSuccess) {
        t.lg = table_log2_slots(t.n_keys);
        if (!t.lg) st = RAWDTW_ERR_RANGE;
    }
    if (e == hipSuccess && st == RAWDTW_OK) {
        const uint64_t n_slots = 1ull << t.lg;
        hip_ok(hipMalloc((void **)&t.d_slots, n_slots * sizeof(Slot)));
        if (t.n_keys) { // each list's start: the exclusive scan of the lists' lengths in ascending hash order; the total behind the last
            size_t bytes = 0;
            const auto len = rocprim::make_transform_iterator(index, ListLen{d_start, t.n_keys, n});
            hip_ok(hipMalloc((void **)&d_loff, (t.n_keys + 1) * 8));
            hip_ok(hipMalloc((void **)&d_tab, n_slots * 4));
            if (e == hipSuccess) hip_ok(rocprim::exclusive_scan(nullptr, bytes, len, d_loff, (uint64_t)0, (size_t)(t.n_keys + 1), rocprim::plus<uint64_t>(), s));
            if (e == hipSuccess) hip_ok(hipMalloc(&d_tmp, std::max<size_t>(bytes, 16)));
            if (e == hipSuccess) hip_ok(rocprim::exclusive_scan(d_tmp, bytes, len, d_loff, (uint64_t)0, (size_t)(t.n_keys + 1), rocprim::plus<uint64_t>(), s));
            if (e == hipSuccess) hip_ok(hipMemcpyAsync(&t.n_list, d_loff + t.n_keys, 8, hipMemcpyDeviceToHost, s));
            if (e == hipSuccess) hip_ok(hipMemsetAsync(d_tab, 0xff, n_slots * 4, s)); // (kNoEntry in every slot)
            if (e == hipSuccess) {
                const uint32_t blocks = (uint32_t)std::min<uint64_t>((t.n_keys + 255) / 256, 1u << 20);
                hipLaunchKernelGGL(k_tb_insert, dim3(blocks), dim3(256), 0, s, d_hash, d_start, (uint32_t)t.n_keys, t.lg, d_tab, d_flags);
                hip_ok(hipGetLastError());
            }
            if (e == hipSuccess) {
                const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_slots + 255) / 256, 1u << 20);
                hipLaunchKernelGGL(k_tb_slots, dim3(blocks), dim3(256), 0, s, d_hash, d_y, d_start, d_loff, t.n_keys, n, t.lg, d_tab, t.d_slots, d_flags);
                hip_ok(hipGetLastError());
            }
            if (e == hipSuccess) hip_ok(hipStreamSynchronize(s)); // (the lists' total is home)
            if (d_tmp) { (void)hipFree(d_tmp); d_tmp = nullptr; }
        } else if (e == hipSuccess) hip_ok(hipMemsetAsync(t.d_slots, 0, n_slots * sizeof(Slot), s));
        if (e == hipSuccess) hip_ok(hipMalloc((void **)&t.d_list, std::max<uint64_t>(t.n_list, 1) * 8));
        if (e == hipSuccess && t.n_list) { // pos: the y of the groups with more than one entry, compacted in sorted order
            size_t bytes = 0;
            const auto in_list = rocprim::make_transform_iterator(index, InList{d_hash, n});
            hip_ok(rocprim::select(nullptr, bytes, d_y, in_list, t.d_list, d_count + 1, (size_t)n, s));
            if (e == hipSuccess) hip_ok(hipMalloc(&d_tmp, std::max<size_t>(bytes, 16)));
            if (e == hipSuccess) hip_ok(rocprim::select(d_tmp, bytes, d_y, in_list, t.d_list, d_count + 1, (size_t)n, s));
        }
        if (e == hipSuccess) hip_ok(hipEventRecord(ev[1], s));
        if (e == hipSuccess) hip_ok(hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, s));
        if (e == hipSuccess) hip_ok(hipStreamSynchronize(s));
        if (e == hipSuccess) (void)hipEventElapsedTime(&t.ms, ev[0], ev[1]);
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(s);
    for (void *p : {(void *)d_start, (void *)d_loff, (void *)d_count, (void *)d_flags, (void *)d_tab, d_tmp}) if (p) (void)hipFree(p);
    for (int i = 0; i < 2; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (e == hipSuccess && st == RAWDTW_OK && flags[0]) st = RAWDTW_ERR_INTERNAL;
    if (e == hipSuccess && st == RAWDTW_OK && flags[1]) st = RAWDTW_ERR_RANGE;
    if (e != hipSuccess || st != RAWDTW_OK) {
        if (t.d_slots) (void)hipFree(t.d_slots);
        if (t.d_list) (void)hipFree(t.d_list);
        if (e != hipSuccess) return hip_fail(ctx, e, "the seed table's device build");
        return fail(ctx, st, st == RAWDTW_ERR_INTERNAL ? "a key found no free slot in a table at most half full" : "more keys than 2^30, or a key with 2^32 positions or more");
    }
    t.displaced = flags[2];
    *out = t;
    return RAWDTW_OK;
}

// a resident index's handle: the header alone
static rawdtw_seed_index *resident_handle(rawdtw_ctx *ctx, rawdtw_seed_index *six, const DeviceTable &t, uint64_t n_positions)
{
    six->log2_slots = t.lg; six->n_keys = t.n_keys; six->n_positions = n_positions; six->n_list = t.n_list;
    six->resident = true; six->owner = ctx;
    return six;
}

// All three entries: the checks, the filter, then the entries -- k_sb_emit for w == 0, the hash / count / scan / write launches for w > 0
// (min_ok: the entry takes them) -- the two sorts, the entries' way home and fill_table.  resident: the filter is the three tiled
// launches, nothing comes home, and the table is built on the device and installed as the context's behind the last check.
static int build_device(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out, bool min_ok, bool resident = false)
{
    if (!ctx || !out) return RAWDTW_ERR_INVALID;
    *out = nullptr;
    if (check_pars(pars) != RAWDTW_OK) return fail(ctx, RAWDTW_ERR_INVALID, "bad seed parameters");
    if (!ctx->d_ref || 2 * ctx->ref_len.size() != ctx->ref_off.size() || (ctx->ref_len.empty() && !ctx->ref_hold))
        return fail(ctx, RAWDTW_ERR_INVALID, "the context holds no reference with a sequence table");
    if (pars->w > 0 && !min_ok) return fail(ctx, RAWDTW_ERR_UNSUPPORTED, "w > 0: minimizer windows over whole strands are built on the host");
    if (resident)
        if (const int no = seed_table_installable(ctx)) return no;
    const bool windowed = pars->w > 0;
    const uint32_t n_seq = (uint32_t)ctx->ref_len.size();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<StrandRow> rows;
    std::vector<uint64_t> tile0; // resident: a strand's first tile of kFilterTile events among all strands' tiles
    uint64_t total_len = 0, max_len = 0, f_tiles = 0;
    try { rows.resize(2ull * n_seq); tile0.resize(2ull * n_seq); } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    for (uint32_t s = 0; s < n_seq; s++)
        for (int slot = 0; slot < 2; slot++) { // slot 0: forward (strand 1)
            rows[2 * s + slot] = StrandRow{ctx->ref_off[2 * s + slot], total_len, 0, ctx->ref_len[s], 0};
            tile0[2 * s + slot] = f_tiles;
            f_tiles += ((uint64_t)ctx->ref_len[s] + kFilterTile - 1) / kFilterTile;
            total_len += ctx->ref_len[s];
            max_len = std::max<uint64_t>(max_len, ctx->ref_len[s]);
        }
    rawdtw_seed_index *six = new (std::nothrow) rawdtw_seed_index;
    if (!six) return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    six->pars = *pars; six->n_seq = n_seq; six->serial = next_serial();
    StrandRow *d_rows = nullptr;
    uint32_t *d_kpos = nullptr, *d_kcode = nullptr, *d_hash[2] = {nullptr, nullptr};
    uint64_t *d_y[2] = {nullptr, nullptr};
    void *d_tmp = nullptr;
    // w > 0: the e-mers' hashes, a count a tile (and a 0 behind the last), their exclusive scan (the total behind the last), the word
    // k_sb_min_write counts its elements in, the scan's temporary storage
    uint32_t *d_h = nullptr;
    uint64_t *d_cnt = nullptr, *d_off = nullptr;
    unsigned long long *d_written = nullptr;
    void *d_scan_tmp = nullptr;
    // resident: the tiled filter's words (a next | steps word and a last value an event, an entry and a kept count a tile) and its events
    uint32_t *d_nc = nullptr, *d_tentry = nullptr, *d_tkept = nullptr;
    float *d_xe = nullptr;
    uint64_t *d_tile0 = nullptr;
    hipEvent_t evf[2] = {nullptr, nullptr}; // between the three launches (ev[0] and ev[1] lie around them)
    float filter_ms[3] = {0.f, 0.f, 0.f};
    DeviceTable table;
    uint64_t kept_total = 0;
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // filter | emit | sort; w > 0: hash | count + scan, write
    float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, min_ms[3] = {0.f, 0.f, 0.f};
    int st = RAWDTW_OK;
    std::vector<uint32_t> h_hash;
    std::vector<uint64_t> h_y;
    std::vector<Entry> all;
    uint64_t N = 0, emers = 0;
    hipError_t e = hipSuccess;
    auto hip_ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
    size_t tmp_a = 0, tmp_b = 0;
    uint32_t seq_bits = 0;
    while (seq_bits < 32 && (1ull << seq_bits) < n_seq) seq_bits++;
    // the entry arrays for N entries, twice over, and the sorts' temporary storage
    auto sort_arrays = [&]() {
        for (int i = 0; i < 2; i++) { hip_ok(hipMalloc((void **)&d_hash[i], N * 4)); hip_ok(hipMalloc((void **)&d_y[i], N * 8)); }
        if (e == hipSuccess) hip_ok(rocprim::radix_sort_pairs(nullptr, tmp_a, d_y[0], d_y[1], d_hash[0], d_hash[1], (size_t)N, 0u, 32u + seq_bits, ctx->stream));
        if (e == hipSuccess) hip_ok(rocprim::radix_sort_pairs(nullptr, tmp_b, d_hash[1], d_hash[0], d_y[1], d_y[0], (size_t)N, 0u, 32u, ctx->stream));
        if (e == hipSuccess) hip_ok(hipMalloc(&d_tmp, std::max<size_t>(std::max(tmp_a, tmp_b), 16)));
    };
    // the entries in d_hash[0] / d_y[0]: stable by y, then stable by hash, then home (from: the event at the sorts' start, done: at their end)
    auto sort_and_home = [&](hipEvent_t from, hipEvent_t done) {
        if (e == hipSuccess) hip_ok(rocprim::radix_sort_pairs(d_tmp, tmp_a, d_y[0], d_y[1], d_hash[0], d_hash[1], (size_t)N, 0u, 32u + seq_bits, ctx->stream));
        if (e == hipSuccess) hip_ok(rocprim::radix_sort_pairs(d_tmp, tmp_b, d_hash[1], d_hash[0], d_y[1], d_y[0], (size_t)N, 0u, 32u, ctx->stream));
        if (e == hipSuccess) hip_ok(hipEventRecord(done, ctx->stream));
        if (e == hipSuccess) hip_ok(hipEventSynchronize(done));
        const double t0 = now_ms();
        if (!resident) try { h_hash.resize(N); h_y.resize(N); } catch (const std::bad_alloc &) { st = RAWDTW_ERR_OOM; }
        if (!resident && st == RAWDTW_OK && e == hipSuccess) {
            hip_ok(hipMemcpyAsync(h_hash.data(), d_hash[0], N * 4, hipMemcpyDeviceToHost, ctx->stream));
            hip_ok(hipMemcpyAsync(h_y.data(), d_y[0], N * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        hip_ok(hipStreamSynchronize(ctx->stream));
        if (e == hipSuccess && st == RAWDTW_OK) {
            (void)hipEventElapsedTime(&ms[2], from, done);
            ms[3] = (float)(now_ms() - t0);
        }
    };
    for (int i = 0; i < 8; i++) hip_ok(hipEventCreate(&ev[i]));
    if (resident) for (int i = 0; i < 2; i++) hip_ok(hipEventCreate(&evf[i]));
    if (n_seq && total_len) {
        hip_ok(hipMalloc((void **)&d_rows, rows.size() * sizeof(StrandRow)));
        hip_ok(hipMalloc((void **)&d_kpos, total_len * 4));
        hip_ok(hipMalloc((void **)&d_kcode, total_len * 4));
        if (e == hipSuccess) hip_ok(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(StrandRow), hipMemcpyHostToDevice, ctx->stream));
        if (resident) {
            hip_ok(hipMalloc((void **)&d_nc, total_len * 4));
            hip_ok(hipMalloc((void **)&d_xe, total_len * 4));
            hip_ok(hipMalloc((void **)&d_tile0, tile0.size() * 8));
            hip_ok(hipMalloc((void **)&d_tentry, f_tiles * 4));
            hip_ok(hipMalloc((void **)&d_tkept, f_tiles * 4));
            if (e == hipSuccess) hip_ok(hipMemcpyAsync(d_tile0, tile0.data(), tile0.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        }
        if (e == hipSuccess) hip_ok(hipEventRecord(ev[0], ctx->stream));
        if (e == hipSuccess && resident) {
            const dim3 by_tile(2 * n_seq, (uint32_t)std::min<uint64_t>((max_len + kFilterTile - 1) / kFilterTile, kTileGridY));
            if (windowed) hipLaunchKernelGGL(k_sb_next<false>, by_tile, dim3(256), 0, ctx->stream, ctx->d_ref, d_rows, d_nc, d_xe);
            else hipLaunchKernelGGL(k_sb_next<true>, by_tile, dim3(256), 0, ctx->stream, ctx->d_ref, d_rows, d_nc, d_xe);
            hip_ok(hipGetLastError());
            if (e == hipSuccess) hip_ok(hipEventRecord(evf[0], ctx->stream));
            if (e == hipSuccess) {
                if (windowed) hipLaunchKernelGGL(k_sb_chain<false>, dim3(2 * n_seq), dim3(64), 0, ctx->stream, ctx->d_ref, d_rows, d_tile0, d_nc, d_xe, d_tentry, d_tkept);
                else hipLaunchKernelGGL(k_sb_chain<true>, dim3(2 * n_seq), dim3(64), 0, ctx->stream, ctx->d_ref, d_rows, d_tile0, d_nc, d_xe, d_tentry, d_tkept);
                hip_ok(hipGetLastError());
            }
            if (e == hipSuccess) hip_ok(hipEventRecord(evf[1], ctx->stream));
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_sb_mark, by_tile, dim3(64), 0, ctx->stream, ctx->d_ref, d_rows, d_tile0, d_nc, d_tentry, d_tkept, pars->q, pars->lq, d_kpos, d_kcode);
                hip_ok(hipGetLastError());
            }
        }
        if (e == hipSuccess && !resident) {
            if (windowed) hipLaunchKernelGGL(k_sb_filter<false>, dim3(2 * n_seq), dim3(64), 0, ctx->stream, ctx->d_ref, d_rows, pars->q, pars->lq, d_kpos, d_kcode);
            else hipLaunchKernelGGL(k_sb_filter<true>, dim3(2 * n_seq), dim3(64), 0, ctx->stream, ctx->d_ref, d_rows, pars->q, pars->lq, d_kpos, d_kcode);
            hip_ok(hipGetLastError());
        }
        if (e == hipSuccess) hip_ok(hipEventRecord(ev[1], ctx->stream));
        if (e == hipSuccess) hip_ok(hipMemcpyAsync(rows.data(), d_rows, rows.size() * sizeof(StrandRow), hipMemcpyDeviceToHost, ctx->stream));
        if (e == hipSuccess) hip_ok(hipStreamSynchronize(ctx->stream));
        if (e == hipSuccess && !windowed) {
            uint64_t max_n = 0;
            for (StrandRow &r : rows) {
                r.entry_base = N;
                const uint64_t n = r.kept >= pars->e ? r.kept - pars->e + 1 : 0;
                N += n; max_n = std::max(max_n, n);
            }
            if (N) {
                sort_arrays();
                if (e == hipSuccess) hip_ok(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(StrandRow), hipMemcpyHostToDevice, ctx->stream));
                if (e == hipSuccess) hip_ok(hipEventRecord(ev[2], ctx->stream));
                if (e == hipSuccess) {
                    const uint32_t gy = (uint32_t)std::min<uint64_t>((max_n + 255) / 256, 1024);
                    hipLaunchKernelGGL(k_sb_emit, dim3(2 * n_seq, gy), dim3(256), 0, ctx->stream, d_rows, d_kpos, d_kcode, pars->e, pars->lq + 2, d_hash[0],
                                       d_y[0]);
                    hip_ok(hipGetLastError());
                }
                if (e == hipSuccess) hip_ok(hipEventRecord(ev[3], ctx->stream));
                sort_and_home(ev[3], ev[4]);
                if (e == hipSuccess && st == RAWDTW_OK) (void)hipEventElapsedTime(&ms[1], ev[2], ev[3]);
            }
        }
        if (e == hipSuccess && windowed) {
            uint64_t n_tiles = 0, max_tiles = 0;
            for (StrandRow &r : rows) {
                r.entry_base = n_tiles; // (the strand's first tile)
                const uint64_t n = r.kept >= pars->e ? r.kept - pars->e + 1 : 0, tiles = (n + kMinTile - 1) / kMinTile;
                emers += n; n_tiles += tiles; max_tiles = std::max(max_tiles, tiles);
            }
            if (n_tiles) {
                size_t scan_bytes = 0;
                const uint32_t gy = (uint32_t)std::min<uint64_t>(max_tiles, 1024); // (a hash launch's blocks take kMinTile e-mers at a time too)
                hip_ok(hipMalloc((void **)&d_h, total_len * 4));
                hip_ok(hipMalloc((void **)&d_cnt, (n_tiles + 1) * 8));
                hip_ok(hipMalloc((void **)&d_off, (n_tiles + 1) * 8));
                hip_ok(hipMalloc((void **)&d_written, 8));
                if (e == hipSuccess) hip_ok(rocprim::exclusive_scan(nullptr, scan_bytes, d_cnt, d_off, (uint64_t)0, (size_t)(n_tiles + 1), rocprim::plus<uint64_t>(), ctx->stream));
                if (e == hipSuccess) hip_ok(hipMalloc(&d_scan_tmp, std::max<size_t>(scan_bytes, 16)));
                if (e == hipSuccess) hip_ok(hipMemsetAsync(d_cnt + n_tiles, 0, 8, ctx->stream));
                if (e == hipSuccess) hip_ok(hipMemsetAsync(d_written, 0, 8, ctx->stream));
                if (e == hipSuccess) hip_ok(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(StrandRow), hipMemcpyHostToDevice, ctx->stream));
                if (e == hipSuccess) hip_ok(hipEventRecord(ev[2], ctx->stream));
                if (e == hipSuccess) {
                    hipLaunchKernelGGL(k_sb_hash, dim3(2 * n_seq, gy), dim3(256), 0, ctx->stream, d_rows, d_kcode, pars->e, pars->lq + 2, d_h);
                    hip_ok(hipGetLastError());
                }
                if (e == hipSuccess) hip_ok(hipEventRecord(ev[3], ctx->stream));
                if (e == hipSuccess) {
                    hipLaunchKernelGGL(k_sb_min_count, dim3(2 * n_seq, gy), dim3(kMinTile), 0, ctx->stream, d_rows, d_h, pars->e, pars->w, d_cnt);
                    hip_ok(hipGetLastError());
                }
                if (e == hipSuccess) hip_ok(rocprim::exclusive_scan(d_scan_tmp, scan_bytes, d_cnt, d_off, (uint64_t)0, (size_t)(n_tiles + 1), rocprim::plus<uint64_t>(), ctx->stream));
                if (e == hipSuccess) hip_ok(hipEventRecord(ev[4], ctx->stream));
                // the total comes home and sizes the entry arrays exactly (no cap: more entries than e-mers is legal)
                if (e == hipSuccess) hip_ok(hipMemcpyAsync(&N, d_off + n_tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
                if (e == hipSuccess) hip_ok(hipStreamSynchronize(ctx->stream));
                if (e != hipSuccess) N = 0;
                if (N) {
                    unsigned long long written = 0;
                    sort_arrays();
                    if (e == hipSuccess) hip_ok(hipEventRecord(ev[5], ctx->stream));
                    if (e == hipSuccess) {
                        hipLaunchKernelGGL(k_sb_min_write, dim3(2 * n_seq, gy), dim3(kMinTile), 0, ctx->stream, d_rows, d_h, d_kpos, pars->e, pars->w, d_off, N,
                                           d_hash[0], d_y[0], d_written);
                        hip_ok(hipGetLastError());
                    }
                    if (e == hipSuccess) hip_ok(hipEventRecord(ev[6], ctx->stream));
                    if (e == hipSuccess) hip_ok(hipMemcpyAsync(&written, d_written, 8, hipMemcpyDeviceToHost, ctx->stream));
                    sort_and_home(ev[6], ev[7]);
                    if (e == hipSuccess && st == RAWDTW_OK) {
                        (void)hipEventElapsedTime(&min_ms[0], ev[2], ev[3]);
                        (void)hipEventElapsedTime(&min_ms[1], ev[3], ev[4]);
                        (void)hipEventElapsedTime(&min_ms[2], ev[5], ev[6]);
                        ms[1] = min_ms[0] + min_ms[1] + min_ms[2];
                        if (written != N) st = RAWDTW_ERR_INTERNAL; // the write did not put down what the count counted: no table
                    }
                }
            }
        }
        if (e == hipSuccess) (void)hipEventElapsedTime(&ms[0], ev[0], ev[1]);
        if (e == hipSuccess && resident) {
            (void)hipEventElapsedTime(&filter_ms[0], ev[0], evf[0]);
            (void)hipEventElapsedTime(&filter_ms[1], evf[0], evf[1]);
            (void)hipEventElapsedTime(&filter_ms[2], evf[1], ev[1]);
            for (const StrandRow &r : rows) kept_total += r.kept;
        }
    }
    // resident: the table from the sorted entries where they lie (no entry: 16 empty slots), before the entries are let go
    int table_st = RAWDTW_OK;
    if (resident && e == hipSuccess && st == RAWDTW_OK) table_st = table_on_device(ctx, d_hash[0], d_y[0], N, &table);
    if (e != hipSuccess) (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < 2; i++) if (evf[i]) (void)hipEventDestroy(evf[i]);
    for (void *p : {(void *)d_nc, (void *)d_xe, (void *)d_tile0, (void *)d_tentry, (void *)d_tkept}) if (p) (void)hipFree(p);
    for (int i = 0; i < 8; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
    for (int i = 0; i < 2; i++) { if (d_hash[i]) (void)hipFree(d_hash[i]); if (d_y[i]) (void)hipFree(d_y[i]); }
    if (d_tmp) (void)hipFree(d_tmp);
    if (d_scan_tmp) (void)hipFree(d_scan_tmp);
    if (d_written) (void)hipFree(d_written);
    if (d_off) (void)hipFree(d_off);
    if (d_cnt) (void)hipFree(d_cnt);
    if (d_h) (void)hipFree(d_h);
    if (d_kpos) (void)hipFree(d_kpos);
    if (d_kcode) (void)hipFree(d_kcode);
    if (d_rows) (void)hipFree(d_rows);
    if (e != hipSuccess) { delete six; return hip_fail(ctx, e, resident ? "rawdtw_seed_index_build_resident" : windowed ? "rawdtw_seed_index_build_device_min" : "rawdtw_seed_index_build_device"); }
    if (st == RAWDTW_ERR_INTERNAL) { delete six; return fail(ctx, st, "the write launch's element count is not the scan's total"); }
    if (resident) { // behind the last check: the table becomes the context's, the handle carries the header
        if (table_st != RAWDTW_OK) { delete six; return table_st; } // (table_on_device has said why, and freed what it made)
        seed_table_install(ctx, table.d_slots, table.d_list, table.lg, *pars, six->serial);
        memcpy(ctx->seed_build_ms, ms, sizeof(ms));
        if (windowed) {
            ctx->seed_min_emers = emers; ctx->seed_min_entries = N;
            memcpy(ctx->seed_min_ms, min_ms, sizeof(min_ms));
        }
        ctx->seed_resident = rawdtw_seed_resident_stats_t{kFilterTile, table.lg, f_tiles, kept_total, N, table.n_keys, table.displaced,
                                                          filter_ms[0], filter_ms[1], filter_ms[2], ms[1], ms[2], table.ms};
        *out = resident_handle(ctx, six, table, N);
        return RAWDTW_OK;
    }
    const double t1 = now_ms();
    if (st == RAWDTW_OK) {
        try {
            all.resize(N);
            for (uint64_t i = 0; i < N; i++) all[i] = Entry{h_hash[i], h_y[i]};
            std::vector<uint32_t>().swap(h_hash);
            std::vector<uint64_t>().swap(h_y);
        } catch (const std::bad_alloc &) { st = RAWDTW_ERR_OOM; }
    }
    if (st == RAWDTW_OK) st = fill_table(six, all);
    ms[4] = (float)(now_ms() - t1);
    if (st != RAWDTW_OK) { delete six; return fail(ctx, st, "building the table failed"); }
    memcpy(ctx->seed_build_ms, ms, sizeof(ms));
    if (windowed) {
        ctx->seed_min_emers = emers; ctx->seed_min_entries = N;
        memcpy(ctx->seed_min_ms, min_ms, sizeof(min_ms));
    }
    *out = six;
    return RAWDTW_OK;
}

extern "C" {

int rawdtw_seed_index_build_device(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out)
{
    return build_device(ctx, pars, out, false);
}

int rawdtw_seed_index_build_device_min(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out)
{
    return build_device(ctx, pars, out, true);
}

int rawdtw_seed_index_build_resident(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out)
{
    return build_device(ctx, pars, out, true, true);
}

int rawdtw_seed_table_from_entries(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, uint32_t n_seq, uint64_t n, const uint32_t *hash,
                                   const uint64_t *y, rawdtw_seed_index **out)
{
    if (!ctx || !out) return RAWDTW_ERR_INVALID;
    *out = nullptr;
    if (check_pars(pars) != RAWDTW_OK) return fail(ctx, RAWDTW_ERR_INVALID, "bad seed parameters");
    if (n && (!hash || !y)) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (!entries_sorted(n, hash, y)) return fail(ctx, RAWDTW_ERR_INVALID, "the entries are not sorted by (hash, y)");
    if (const int no = seed_table_installable(ctx)) return no;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rawdtw_seed_index *six = new (std::nothrow) rawdtw_seed_index;
    if (!six) return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    six->pars = *pars; six->n_seq = n_seq; six->serial = next_serial();
    uint32_t *d_hash = nullptr;
    uint64_t *d_y = nullptr;
    hipError_t e = hipSuccess;
    if (n) {
        e = hipMalloc((void **)&d_hash, n * 4);
        if (e == hipSuccess) e = hipMalloc((void **)&d_y, n * 8);
        if (e == hipSuccess) e = hipMemcpyAsync(d_hash, hash, n * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_y, y, n * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    DeviceTable table;
    const int st = e == hipSuccess ? table_on_device(ctx, d_hash, d_y, n, &table) : hip_fail(ctx, e, "rawdtw_seed_table_from_entries");
    if (d_hash) (void)hipFree(d_hash);
    if (d_y) (void)hipFree(d_y);
    if (st != RAWDTW_OK) { delete six; return st; }
    seed_table_install(ctx, table.d_slots, table.d_list, table.lg, *pars, six->serial);
    ctx->seed_resident = rawdtw_seed_resident_stats_t{kFilterTile, table.lg, 0, 0, n, table.n_keys, table.displaced, 0.f, 0.f, 0.f, 0.f, 0.f, table.ms};
    *out = resident_handle(ctx, six, table, n);
    return RAWDTW_OK;
}

int rawdtw_seed_index_build_resident_stats(const rawdtw_ctx *ctx, rawdtw_seed_resident_stats_t *out)
{
    if (!ctx || !out) return RAWDTW_ERR_INVALID;
    *out = ctx->seed_resident;
    return RAWDTW_OK;
}

int rawdtw_seed_index_build_min_stats(const rawdtw_ctx *ctx, uint64_t *emers, uint64_t *entries, float select_ms[3])
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (emers) *emers = ctx->seed_min_emers;
    if (entries) *entries = ctx->seed_min_entries;
    if (select_ms) memcpy(select_ms, ctx->seed_min_ms, sizeof(ctx->seed_min_ms));
    return RAWDTW_OK;
}

int rawdtw_seed_index_build_stats(const rawdtw_ctx *ctx, float phase_ms[5])
{
    if (!ctx || !phase_ms) return RAWDTW_ERR_INVALID;
    memcpy(phase_ms, ctx->seed_build_ms, sizeof(ctx->seed_build_ms));
    return RAWDTW_OK;
}

} // extern "C"
