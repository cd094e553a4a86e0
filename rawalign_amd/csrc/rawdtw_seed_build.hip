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
// The device arrays, each a hipMalloc of its own, for their sizes become known in three stages (after the host's pass over the sequence
// table, after the filter, after the selection's scan): per strand a row (below); per event of the arena a kept position and a kept code
// (4 bytes each); per entry a hash and a y, twice over for the sort's double buffer, and rocPRIM's temporary storage.  w > 0 adds a hash
// per event of the arena (4 bytes), a count and an offset a tile (8 bytes each), the scan's temporary storage and the word the write counts
// in; the tiled filter a next | steps word and a last value an event, an entry and a kept count a tile.
//
// The host side: every array and event is the Owner's, whose destructor frees them whatever way a call ends.  A build is phases over one
// Build -- the checks, the strands' rows, the filter, the entries, the two sorts, the end on the host or the resident end -- each returning
// at its first error, with the statistics written at one commit point (commit_stats) behind the last check.  What an asynchronous copy
// brings home lands in the Build or its DeviceTable, never in a phase's frame.
#include "rawdtw_capi.h"
#include "rawdtw_seed.h"
#include "rawdtw_seed_min.h"
#include "rawdtw_seed_tile.h"

#include <algorithm>
#include <chrono>
#include <memory>
#include <vector>

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
    const uint32_t n = strand_emers(row.kept, e), strand = (pair & 1) ? 0u : 1u;
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
    const uint32_t n = strand_emers(row.kept, e);
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
    const uint32_t M = strand_emers(row.kept, e), tiles = (M + kMinTile - 1) / kMinTile;
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
    const uint32_t M = strand_emers(row.kept, e), tiles = (M + kMinTile - 1) / kMinTile;
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
    const uint32_t tiles = filter_tiles(row.len);
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
    const uint32_t n = row.len, tiles = filter_tiles(n);
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
    const uint32_t tiles = filter_tiles(row.len), lane = threadIdx.x;
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

namespace {

// The one owner of what a build has on the device: every array is a hipMalloc of its own, taken here, and every event is created here.
// Whatever way a build ends, the destructor frees and destroys them all -- behind a wait for the stream where a call has failed with
// work enqueued.  release() takes out an array that outlives the build: the resident table's slots and list.
struct Owner {
    rawdtw_ctx *ctx;
    const char *what;              // the entry point a failed HIP call is reported under
    hipError_t err = hipSuccess;   // the first HIP call that failed
    std::vector<void *> arrays;
    std::vector<hipEvent_t> events;

    Owner(rawdtw_ctx *c, const char *w) : ctx(c), what(w) {}
    Owner(const Owner &) = delete;
    Owner &operator=(const Owner &) = delete;
    ~Owner()
    {
        if (err != hipSuccess && !(arrays.empty() && events.empty())) (void)hipStreamSynchronize(ctx->stream);
        for (void *p : arrays) (void)hipFree(p);
        for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
    }
    bool ok(hipError_t r)
    {
        if (err == hipSuccess) err = r;
        return err == hipSuccess;
    }
    int failed() const { return hip_fail(ctx, err, what); }
    // (no room on the host to remember x: the same answer as no room on the device)
    template <typename V, typename X> bool remember(V &list, X x)
    {
        try { list.push_back(x); } catch (const std::bad_alloc &) { err = hipErrorOutOfMemory; }
        return err == hipSuccess;
    }
    template <typename T> hipError_t take(T *&p, uint64_t count)
    {
        void *q = nullptr;
        if (err == hipSuccess && ok(hipMalloc(&q, count * sizeof(T))) && !remember(arrays, q)) { (void)hipFree(q); q = nullptr; }
        p = static_cast<T *>(q);
        return err;
    }
    hipEvent_t event()
    {
        hipEvent_t ev = nullptr;
        if (err == hipSuccess && ok(hipEventCreate(&ev)) && !remember(events, ev)) { (void)hipEventDestroy(ev); ev = nullptr; }
        return ev;
    }
    template <typename T> T *release(T *p)
    {
        arrays.erase(std::remove(arrays.begin(), arrays.end(), static_cast<void *>(p)), arrays.end());
        return p;
    }
};

// A HIP or rocPRIM call of a phase: the first that fails ends the phase, reported under the entry point's name.  Nothing is enqueued behind it.
#define SB_HIP(own, expr)                                                                             \
    do {                                                                                              \
        if (!(own).ok(expr)) return (own).failed();                                                   \
    } while (0)
#define SB_LAUNCH(own, kernel, grid, block, ...)                                                      \
    do {                                                                                              \
        hipLaunchKernelGGL(kernel, grid, block, 0, (own).ctx->stream, __VA_ARGS__);                   \
        SB_HIP(own, hipGetLastError());                                                               \
    } while (0)
// a phase inside a phase
#define SB_TRY(expr)                                                                                  \
    do {                                                                                              \
        const int st_ = (expr);                                                                       \
        if (st_ != RAWDTW_OK) return st_;                                                             \
    } while (0)

// rocPRIM's two-call form, call(storage, bytes): with no storage the call says how many bytes it wants.  prim_take: the storage for an
// answer, 16 bytes at least; prim_run: the question, the storage, the call.  (Where launches lie between the question and the call -- the
// selection's scan, the two sorts, which share one storage of the larger size -- the call is written once and made twice.)
hipError_t prim_take(Owner &own, void *&tmp, size_t bytes)
{
    char *p = nullptr;
    const hipError_t e = own.take(p, std::max<size_t>(bytes, 16));
    tmp = p;
    return e;
}
template <typename F> hipError_t prim_run(Owner &own, void *&tmp, F call)
{
    size_t bytes = 0;
    if (!own.ok(call(nullptr, bytes)) || prim_take(own, tmp, bytes) != hipSuccess) return own.err;
    return call(tmp, bytes);
}

// The table of n sorted entries in device memory, built there: on success the slots and lists are the caller's to install or free.
struct DeviceTable {
    Slot *d_slots = nullptr;
    uint64_t *d_list = nullptr;
    uint32_t lg = 0;
    uint64_t n_keys = 0, n_list = 0, displaced = 0;
    unsigned long long flags[3] = {0, 0, 0}; // (k_tb_insert's and k_tb_slots')
    float ms = 0.f;
};

// What the phases of a build hand to each other.  Every destination of an asynchronous copy to the host -- rows, N, written, and
// DeviceTable's n_keys, n_list and flags -- lives here, never in the frame of a phase: a phase may return before the copy has landed, and
// the owner, declared last and so destroyed first, waits for the stream before any of this goes.
struct Build {
    rawdtw_ctx *ctx;
    const rawdtw_seed_pars_t *pars;
    rawdtw_seed_index **out;
    const bool resident;      // the filter is the three tiled launches, nothing comes home, the table is built on the device and installed
    const bool windowed;      // w > 0: the minimizers of the e-mers
    const bool from_entries;  // rawdtw_seed_table_from_entries: the entries are the caller's, the build's times are not this call's to write
    std::unique_ptr<rawdtw_seed_index> six;
    // the strands: a row each, and (for the tiled filter) each one's first tile of kFilterTile events among all strands' tiles
    std::vector<StrandRow> rows;
    std::vector<uint64_t> tile0;
    uint32_t n_seq = 0, seq_bits = 0;
    uint64_t total_len = 0, max_len = 0, f_tiles = 0, kept_total = 0;
    // the owner's arrays that more than one phase uses: the rows, the kept events' positions and codes, the entries twice over for the
    // sorts' double buffer, the sorts' temporary storage and what each sort asked for
    StrandRow *d_rows = nullptr;
    uint32_t *d_kpos = nullptr, *d_kcode = nullptr, *d_hash[2] = {nullptr, nullptr};
    uint64_t *d_y[2] = {nullptr, nullptr};
    void *d_tmp = nullptr;
    size_t tmp_a = 0, tmp_b = 0;
    // filter | emit | sort; w > 0: hash | count + scan, write.  evf: between the three tiled launches (ev[0] and ev[1] lie around them)
    hipEvent_t ev[8] = {}, evf[2] = {}, sort_from = nullptr, sort_done = nullptr;
    uint64_t N = 0, emers = 0;           // the entries in d_hash[0] / d_y[0]; w > 0: the e-mers over all strands
    unsigned long long written = 0;      // w > 0: what k_sb_min_write put down
    float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, min_ms[3] = {0.f, 0.f, 0.f}, filter_ms[3] = {0.f, 0.f, 0.f};
    std::vector<uint32_t> h_hash;        // the sorted entries at home (not resident)
    std::vector<uint64_t> h_y;
    DeviceTable table;
    Owner own;

    Build(rawdtw_ctx *c, const rawdtw_seed_pars_t *p, rawdtw_seed_index **o, const char *what, bool res, bool from)
        : ctx(c), pars(p), out(o), resident(res), windowed(!from && p->w > 0), from_entries(from), own(c, what)
    {
    }
};

// ---- the table's launches (rawdtw_seed_index_build_resident, rawdtw_seed_table_from_entries) ----------------------------------------------
// t: the caller's, for n_keys, n_list and the flags come home into it.  A failed call leaves nothing on the device.
int table_on_device(rawdtw_ctx *ctx, const uint32_t *d_hash, const uint64_t *d_y, uint64_t n, DeviceTable &t)
{
    Owner own(ctx, "the seed table's device build");
    const hipStream_t s = ctx->stream;
    const rocprim::counting_iterator<uint64_t> index(0);
    uint64_t *d_start = nullptr, *d_count = nullptr, *d_loff = nullptr, *d_list = nullptr;
    unsigned long long *d_flags = nullptr;
    uint32_t *d_tab = nullptr;
    Slot *d_slots = nullptr;
    void *tmp = nullptr;
    t = DeviceTable{};
    const hipEvent_t ev0 = own.event(), ev1 = own.event();
    SB_HIP(own, own.err);
    SB_HIP(own, own.take(d_count, 2));
    SB_HIP(own, own.take(d_flags, 3));
    SB_HIP(own, hipMemsetAsync(d_flags, 0, sizeof(t.flags), s));
    SB_HIP(own, hipEventRecord(ev0, s));
    if (n) { // the groups' starts, compacted in order; their number comes home
        SB_HIP(own, own.take(d_start, n));
        SB_HIP(own, prim_run(own, tmp, [&](void *p, size_t &bytes) { return rocprim::select(p, bytes, index, d_start, d_count, (size_t)n, GroupHead{d_hash}, s); }));
        SB_HIP(own, hipMemcpyAsync(&t.n_keys, d_count, 8, hipMemcpyDeviceToHost, s));
        SB_HIP(own, hipStreamSynchronize(s));
        (void)hipFree(own.release(tmp));
    }
    t.lg = table_log2_slots(t.n_keys);
    if (!t.lg) return fail(ctx, RAWDTW_ERR_RANGE, "more keys than 2^30, or a key with 2^32 positions or more");
    const uint64_t n_slots = 1ull << t.lg;
    SB_HIP(own, own.take(d_slots, n_slots));
    if (t.n_keys) { // each list's start: the exclusive scan of the lists' lengths in ascending hash order; the total behind the last
        const auto len = rocprim::make_transform_iterator(index, ListLen{d_start, t.n_keys, n});
        SB_HIP(own, own.take(d_loff, t.n_keys + 1));
        SB_HIP(own, own.take(d_tab, n_slots));
        SB_HIP(own, prim_run(own, tmp, [&](void *p, size_t &bytes) {
                   return rocprim::exclusive_scan(p, bytes, len, d_loff, (uint64_t)0, (size_t)(t.n_keys + 1), rocprim::plus<uint64_t>(), s);
               }));
        SB_HIP(own, hipMemcpyAsync(&t.n_list, d_loff + t.n_keys, 8, hipMemcpyDeviceToHost, s));
        SB_HIP(own, hipMemsetAsync(d_tab, 0xff, n_slots * 4, s)); // (kNoEntry in every slot)
        const uint32_t by_key = (uint32_t)std::min<uint64_t>((t.n_keys + 255) / 256, 1u << 20), by_slot = (uint32_t)std::min<uint64_t>((n_slots + 255) / 256, 1u << 20);
        SB_LAUNCH(own, k_tb_insert, dim3(by_key), dim3(256), d_hash, d_start, (uint32_t)t.n_keys, t.lg, d_tab, d_flags);
        SB_LAUNCH(own, k_tb_slots, dim3(by_slot), dim3(256), d_hash, d_y, d_start, d_loff, t.n_keys, n, t.lg, d_tab, d_slots, d_flags);
        SB_HIP(own, hipStreamSynchronize(s)); // (the lists' total is home)
        (void)hipFree(own.release(tmp));
    } else SB_HIP(own, hipMemsetAsync(d_slots, 0, n_slots * sizeof(Slot), s));
    SB_HIP(own, own.take(d_list, std::max<uint64_t>(t.n_list, 1)));
    if (t.n_list) { // pos: the y of the groups with more than one entry, compacted in sorted order
        const auto in_list = rocprim::make_transform_iterator(index, InList{d_hash, n});
        SB_HIP(own, prim_run(own, tmp, [&](void *p, size_t &bytes) { return rocprim::select(p, bytes, d_y, in_list, d_list, d_count + 1, (size_t)n, s); }));
    }
    SB_HIP(own, hipEventRecord(ev1, s));
    SB_HIP(own, hipMemcpyAsync(t.flags, d_flags, sizeof(t.flags), hipMemcpyDeviceToHost, s));
    SB_HIP(own, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&t.ms, ev0, ev1);
    if (t.flags[0]) return fail(ctx, RAWDTW_ERR_INTERNAL, "a key found no free slot in a table at most half full");
    if (t.flags[1]) return fail(ctx, RAWDTW_ERR_RANGE, "more keys than 2^30, or a key with 2^32 positions or more");
    t.displaced = t.flags[2];
    t.d_slots = own.release(d_slots);
    t.d_list = own.release(d_list);
    return RAWDTW_OK;
}

// ---- the phases of a build ---------------------------------------------------------------------------------------------------------------
// 1. everything a build refuses (min_ok: the entry takes w > 0)
int build_checks(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out, bool min_ok, bool resident)
{
    if (!ctx || !out) return RAWDTW_ERR_INVALID;
    *out = nullptr;
    if (check_pars(pars) != RAWDTW_OK) return fail(ctx, RAWDTW_ERR_INVALID, "bad seed parameters");
    if (!ctx->d_ref || 2 * ctx->ref_len.size() != ctx->ref_off.size() || (ctx->ref_len.empty() && !ctx->ref_hold))
        return fail(ctx, RAWDTW_ERR_INVALID, "the context holds no reference with a sequence table");
    if (pars->w > 0 && !min_ok) return fail(ctx, RAWDTW_ERR_UNSUPPORTED, "w > 0: minimizer windows over whole strands are built on the host");
    if (resident)
        if (const int no = seed_table_installable(ctx)) return no;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return RAWDTW_OK;
}

// the handle the call will return: the parameters, the sequences and a fresh serial
int new_handle(Build &b, uint32_t n_seq)
{
    b.six.reset(new (std::nothrow) rawdtw_seed_index);
    if (!b.six) return fail(b.ctx, RAWDTW_ERR_OOM, "host allocation failed");
    b.six->pars = *b.pars; b.six->n_seq = n_seq; b.six->serial = next_serial();
    return RAWDTW_OK;
}

// 2. a row a strand, on the host
int strand_rows(Build &b)
{
    const rawdtw_ctx *ctx = b.ctx;
    b.n_seq = (uint32_t)ctx->ref_len.size();
    try { b.rows.resize(2ull * b.n_seq); b.tile0.resize(2ull * b.n_seq); } catch (const std::bad_alloc &) { return fail(b.ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    for (uint32_t s = 0; s < b.n_seq; s++)
        for (int slot = 0; slot < 2; slot++) { // slot 0: forward (strand 1)
            b.rows[2 * s + slot] = StrandRow{ctx->ref_off[2 * s + slot], b.total_len, 0, ctx->ref_len[s], 0};
            b.tile0[2 * s + slot] = b.f_tiles;
            b.f_tiles += filter_tiles(ctx->ref_len[s]);
            b.total_len += ctx->ref_len[s];
            b.max_len = std::max<uint64_t>(b.max_len, ctx->ref_len[s]);
        }
    while (b.seq_bits < 32 && (1ull << b.seq_bits) < b.n_seq) b.seq_bits++;
    return RAWDTW_OK;
}

// 3. the filter's launches between ev[0] and ev[1]: k_sb_filter, a wave a strand, or the three tiled launches with their words (a next |
// steps word and a last value an event, an entry and a kept count a tile)
template <bool kMask> int filter_launches(Build &b)
{
    Owner &own = b.own;
    const hipStream_t s = b.ctx->stream;
    const uint32_t pairs = 2 * b.n_seq;
    if (!b.resident) {
        SB_HIP(own, hipEventRecord(b.ev[0], s));
        SB_LAUNCH(own, k_sb_filter<kMask>, dim3(pairs), dim3(64), b.ctx->d_ref, b.d_rows, b.pars->q, b.pars->lq, b.d_kpos, b.d_kcode);
        return RAWDTW_OK;
    }
    uint32_t *d_nc = nullptr, *d_tentry = nullptr, *d_tkept = nullptr;
    float *d_xe = nullptr;
    uint64_t *d_tile0 = nullptr;
    SB_HIP(own, own.take(d_nc, b.total_len));
    SB_HIP(own, own.take(d_xe, b.total_len));
    SB_HIP(own, own.take(d_tile0, b.tile0.size()));
    SB_HIP(own, own.take(d_tentry, b.f_tiles));
    SB_HIP(own, own.take(d_tkept, b.f_tiles));
    SB_HIP(own, hipMemcpyAsync(d_tile0, b.tile0.data(), b.tile0.size() * 8, hipMemcpyHostToDevice, s));
    SB_HIP(own, hipEventRecord(b.ev[0], s));
    const dim3 by_tile(pairs, std::min(filter_tiles((uint32_t)b.max_len), kTileGridY));
    SB_LAUNCH(own, k_sb_next<kMask>, by_tile, dim3(256), b.ctx->d_ref, b.d_rows, d_nc, d_xe);
    SB_HIP(own, hipEventRecord(b.evf[0], s));
    SB_LAUNCH(own, k_sb_chain<kMask>, dim3(pairs), dim3(64), b.ctx->d_ref, b.d_rows, d_tile0, d_nc, d_xe, d_tentry, d_tkept);
    SB_HIP(own, hipEventRecord(b.evf[1], s));
    SB_LAUNCH(own, k_sb_mark, by_tile, dim3(64), b.ctx->d_ref, b.d_rows, d_tile0, d_nc, d_tentry, d_tkept, b.pars->q, b.pars->lq, b.d_kpos, b.d_kcode);
    return RAWDTW_OK;
}

// the kept events' positions and codes in d_kpos / d_kcode; the rows come home with every strand's kept events
int filter(Build &b)
{
    Owner &own = b.own;
    const hipStream_t s = b.ctx->stream;
    const size_t rows_bytes = b.rows.size() * sizeof(StrandRow);
    SB_HIP(own, own.take(b.d_rows, b.rows.size()));
    SB_HIP(own, own.take(b.d_kpos, b.total_len));
    SB_HIP(own, own.take(b.d_kcode, b.total_len));
    SB_HIP(own, hipMemcpyAsync(b.d_rows, b.rows.data(), rows_bytes, hipMemcpyHostToDevice, s));
    SB_TRY(b.windowed ? filter_launches<false>(b) : filter_launches<true>(b));
    SB_HIP(own, hipEventRecord(b.ev[1], s));
    SB_HIP(own, hipMemcpyAsync(b.rows.data(), b.d_rows, rows_bytes, hipMemcpyDeviceToHost, s));
    SB_HIP(own, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&b.ms[0], b.ev[0], b.ev[1]);
    if (b.resident) {
        (void)hipEventElapsedTime(&b.filter_ms[0], b.ev[0], b.evf[0]);
        (void)hipEventElapsedTime(&b.filter_ms[1], b.evf[0], b.evf[1]);
        (void)hipEventElapsedTime(&b.filter_ms[2], b.evf[1], b.ev[1]);
        for (const StrandRow &r : b.rows) b.kept_total += r.kept;
    }
    return RAWDTW_OK;
}

// the two sorts of the N entries in d_hash[0] / d_y[0]: stable by y over its used bits, then stable by hash -- the order of
// by_hash_then_position.  With no storage: what each asks for.
int two_sorts(Build &b, void *tmp)
{
    SB_HIP(b.own, rocprim::radix_sort_pairs(tmp, b.tmp_a, b.d_y[0], b.d_y[1], b.d_hash[0], b.d_hash[1], (size_t)b.N, 0u, 32u + b.seq_bits, b.ctx->stream));
    SB_HIP(b.own, rocprim::radix_sort_pairs(tmp, b.tmp_b, b.d_hash[1], b.d_hash[0], b.d_y[1], b.d_y[0], (size_t)b.N, 0u, 32u, b.ctx->stream));
    return RAWDTW_OK;
}

// the entry arrays for N entries, twice over, and the sorts' temporary storage
int sort_arrays(Build &b)
{
    for (int i = 0; i < 2; i++) {
        SB_HIP(b.own, b.own.take(b.d_hash[i], b.N));
        SB_HIP(b.own, b.own.take(b.d_y[i], b.N));
    }
    SB_TRY(two_sorts(b, nullptr));
    SB_HIP(b.own, prim_take(b.own, b.d_tmp, std::max(b.tmp_a, b.tmp_b)));
    return RAWDTW_OK;
}

// 4. the entries, w == 0: every e-mer of every strand, a row's entry_base its first
int entries_all(Build &b)
{
    Owner &own = b.own;
    const hipStream_t s = b.ctx->stream;
    uint64_t max_n = 0;
    for (StrandRow &r : b.rows) {
        r.entry_base = b.N;
        const uint64_t n = strand_emers(r.kept, b.pars->e);
        b.N += n; max_n = std::max(max_n, n);
    }
    if (!b.N) return RAWDTW_OK;
    SB_TRY(sort_arrays(b));
    SB_HIP(own, hipMemcpyAsync(b.d_rows, b.rows.data(), b.rows.size() * sizeof(StrandRow), hipMemcpyHostToDevice, s));
    SB_HIP(own, hipEventRecord(b.ev[2], s));
    const uint32_t gy = (uint32_t)std::min<uint64_t>((max_n + 255) / 256, 1024);
    SB_LAUNCH(own, k_sb_emit, dim3(2 * b.n_seq, gy), dim3(256), b.d_rows, b.d_kpos, b.d_kcode, b.pars->e, b.pars->lq + 2, b.d_hash[0], b.d_y[0]);
    SB_HIP(own, hipEventRecord(b.ev[3], s));
    b.sort_from = b.ev[3]; b.sort_done = b.ev[4];
    return RAWDTW_OK;
}

// 4. the entries, w > 0: the e-mers' hashes, a count a tile of kMinTile e-mers (and a 0 behind the last), their exclusive scan (the total
// behind the last), and the write at the scan's places, which counts what it puts down in a word.  A row's entry_base is its first tile.
int entries_minimizers(Build &b)
{
    Owner &own = b.own;
    const hipStream_t s = b.ctx->stream;
    const rawdtw_seed_pars_t &p = *b.pars;
    uint64_t n_tiles = 0, max_tiles = 0;
    for (StrandRow &r : b.rows) {
        r.entry_base = n_tiles;
        const uint64_t n = strand_emers(r.kept, p.e), tiles = (n + kMinTile - 1) / kMinTile;
        b.emers += n; n_tiles += tiles; max_tiles = std::max(max_tiles, tiles);
    }
    if (!n_tiles) return RAWDTW_OK;
    const dim3 grid(2 * b.n_seq, (uint32_t)std::min<uint64_t>(max_tiles, 1024)); // (a hash launch's blocks take kMinTile e-mers at a time too)
    uint32_t *d_h = nullptr;
    uint64_t *d_cnt = nullptr, *d_off = nullptr;
    unsigned long long *d_written = nullptr;
    void *d_scan_tmp = nullptr;
    size_t scan_bytes = 0;
    SB_HIP(own, own.take(d_h, b.total_len));
    SB_HIP(own, own.take(d_cnt, n_tiles + 1));
    SB_HIP(own, own.take(d_off, n_tiles + 1));
    SB_HIP(own, own.take(d_written, 1));
    const auto scan = [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, d_cnt, d_off, (uint64_t)0, (size_t)(n_tiles + 1), rocprim::plus<uint64_t>(), s);
    };
    SB_HIP(own, scan(nullptr, scan_bytes));
    SB_HIP(own, prim_take(own, d_scan_tmp, scan_bytes));
    SB_HIP(own, hipMemsetAsync(d_cnt + n_tiles, 0, 8, s));
    SB_HIP(own, hipMemsetAsync(d_written, 0, 8, s));
    SB_HIP(own, hipMemcpyAsync(b.d_rows, b.rows.data(), b.rows.size() * sizeof(StrandRow), hipMemcpyHostToDevice, s));
    SB_HIP(own, hipEventRecord(b.ev[2], s));
    SB_LAUNCH(own, k_sb_hash, grid, dim3(256), b.d_rows, b.d_kcode, p.e, p.lq + 2, d_h);
    SB_HIP(own, hipEventRecord(b.ev[3], s));
    SB_LAUNCH(own, k_sb_min_count, grid, dim3(kMinTile), b.d_rows, d_h, p.e, p.w, d_cnt);
    SB_HIP(own, scan(d_scan_tmp, scan_bytes));
    SB_HIP(own, hipEventRecord(b.ev[4], s));
    // the total comes home and sizes the entry arrays exactly (no cap: more entries than e-mers is legal)
    SB_HIP(own, hipMemcpyAsync(&b.N, d_off + n_tiles, 8, hipMemcpyDeviceToHost, s));
    SB_HIP(own, hipStreamSynchronize(s));
    if (!b.N) return RAWDTW_OK;
    SB_TRY(sort_arrays(b));
    SB_HIP(own, hipEventRecord(b.ev[5], s));
    SB_LAUNCH(own, k_sb_min_write, grid, dim3(kMinTile), b.d_rows, d_h, b.d_kpos, p.e, p.w, d_off, b.N, b.d_hash[0], b.d_y[0], d_written);
    SB_HIP(own, hipEventRecord(b.ev[6], s));
    SB_HIP(own, hipMemcpyAsync(&b.written, d_written, 8, hipMemcpyDeviceToHost, s)); // (home behind the sorts' wait)
    b.sort_from = b.ev[6]; b.sort_done = b.ev[7];
    return RAWDTW_OK;
}

// 5. the sorts where the entries lie; behind the wait the events of the entries' launches have passed too
int sorts(Build &b)
{
    Owner &own = b.own;
    SB_TRY(two_sorts(b, b.d_tmp));
    SB_HIP(own, hipEventRecord(b.sort_done, b.ctx->stream));
    SB_HIP(own, hipEventSynchronize(b.sort_done));
    (void)hipEventElapsedTime(&b.ms[2], b.sort_from, b.sort_done);
    if (!b.windowed) {
        (void)hipEventElapsedTime(&b.ms[1], b.ev[2], b.ev[3]);
        return RAWDTW_OK;
    }
    (void)hipEventElapsedTime(&b.min_ms[0], b.ev[2], b.ev[3]);
    (void)hipEventElapsedTime(&b.min_ms[1], b.ev[3], b.ev[4]);
    (void)hipEventElapsedTime(&b.min_ms[2], b.ev[5], b.ev[6]);
    b.ms[1] = b.min_ms[0] + b.min_ms[1] + b.min_ms[2];
    return RAWDTW_OK;
}

// the sorted entries' way home; a resident build brings nothing and waits alone (the `home` slot of the times is this wait either way)
int entries_home(Build &b)
{
    Owner &own = b.own;
    const hipStream_t s = b.ctx->stream;
    const double t0 = now_ms();
    if (!b.resident) {
        try { b.h_hash.resize(b.N); b.h_y.resize(b.N); } catch (const std::bad_alloc &) { return fail(b.ctx, RAWDTW_ERR_OOM, "building the table failed"); }
        SB_HIP(own, hipMemcpyAsync(b.h_hash.data(), b.d_hash[0], b.N * 4, hipMemcpyDeviceToHost, s));
        SB_HIP(own, hipMemcpyAsync(b.h_y.data(), b.d_y[0], b.N * 8, hipMemcpyDeviceToHost, s));
    }
    SB_HIP(own, hipStreamSynchronize(s));
    b.ms[3] = (float)(now_ms() - t0);
    return RAWDTW_OK;
}

// 7. the one commit point, behind the last check: the statistics of the call become the context's.  The build's times and the w > 0
// numbers are a build's to write, the resident statistics a resident build's and rawdtw_seed_table_from_entries'.
void commit_stats(const Build &b)
{
    rawdtw_ctx *ctx = b.ctx;
    if (!b.from_entries) memcpy(ctx->seed_build_ms, b.ms, sizeof(b.ms));
    if (b.windowed) {
        ctx->seed_min_emers = b.emers; ctx->seed_min_entries = b.N;
        memcpy(ctx->seed_min_ms, b.min_ms, sizeof(b.min_ms));
    }
    if (b.resident)
        ctx->seed_resident = rawdtw_seed_resident_stats_t{kFilterTile, b.table.lg, b.f_tiles, b.kept_total, b.N, b.table.n_keys, b.table.displaced,
                                                          b.filter_ms[0], b.filter_ms[1], b.filter_ms[2], b.ms[1], b.ms[2], b.table.ms};
}

// 6. the end on the host: fill_table builds the slots from the entries, as for every other index
int end_on_host(Build &b)
{
    const double t1 = now_ms();
    int st = RAWDTW_OK;
    try {
        std::vector<Entry> all(b.N);
        for (uint64_t i = 0; i < b.N; i++) all[i] = Entry{b.h_hash[i], b.h_y[i]};
        std::vector<uint32_t>().swap(b.h_hash);
        std::vector<uint64_t>().swap(b.h_y);
        st = fill_table(b.six.get(), all);
    } catch (const std::bad_alloc &) { st = RAWDTW_ERR_OOM; }
    b.ms[4] = (float)(now_ms() - t1);
    if (st != RAWDTW_OK) return fail(b.ctx, st, "building the table failed");
    commit_stats(b);
    *b.out = b.six.release();
    return RAWDTW_OK;
}

// 6. the resident end: the table from the sorted entries where they lie (no entry: 16 empty slots) becomes the context's, and the handle
// carries the header alone
int end_resident(Build &b)
{
    SB_TRY(table_on_device(b.ctx, b.d_hash[0], b.d_y[0], b.N, b.table)); // (it has said why, and freed what it made)
    const DeviceTable &t = b.table;
    seed_table_install(b.ctx, t.d_slots, t.d_list, t.lg, *b.pars, b.six->serial);
    commit_stats(b);
    rawdtw_seed_index *six = b.six.release();
    six->log2_slots = t.lg; six->n_keys = t.n_keys; six->n_positions = b.N; six->n_list = t.n_list;
    six->resident = true; six->owner = b.ctx;
    *b.out = six;
    return RAWDTW_OK;
}

// All three builds: the checks, the strands' rows, the filter, the entries (N of them in d_hash[0] / d_y[0]), the two sorts, and the end.
int build_device(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out, bool min_ok, bool resident)
{
    SB_TRY(build_checks(ctx, pars, out, min_ok, resident));
    Build b(ctx, pars, out, resident ? "rawdtw_seed_index_build_resident" : pars->w > 0 ? "rawdtw_seed_index_build_device_min" : "rawdtw_seed_index_build_device",
            resident, false);
    SB_TRY(strand_rows(b));
    SB_TRY(new_handle(b, b.n_seq));
    for (int i = 0; i < 8; i++) b.ev[i] = b.own.event();
    if (resident) for (int i = 0; i < 2; i++) b.evf[i] = b.own.event();
    SB_HIP(b.own, b.own.err);
    if (b.n_seq && b.total_len) {
        SB_TRY(filter(b));
        SB_TRY(b.windowed ? entries_minimizers(b) : entries_all(b));
        if (b.N) {
            SB_TRY(sorts(b));
            // the write did not put down what the count counted: no table
            if (b.windowed && b.written != b.N) return fail(ctx, RAWDTW_ERR_INTERNAL, "the write launch's element count is not the scan's total");
            SB_TRY(entries_home(b));
        }
    }
    return resident ? end_resident(b) : end_on_host(b);
}

} // namespace

extern "C" {

int rawdtw_seed_index_build_device(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out)
{
    return build_device(ctx, pars, out, false, false);
}

int rawdtw_seed_index_build_device_min(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out)
{
    return build_device(ctx, pars, out, true, false);
}

int rawdtw_seed_index_build_resident(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out)
{
    return build_device(ctx, pars, out, true, true);
}

// the checks, the entries up, the resident end
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
    Build b(ctx, pars, out, "rawdtw_seed_table_from_entries", true, true);
    SB_TRY(new_handle(b, n_seq));
    b.N = n;
    if (n) {
        SB_HIP(b.own, b.own.take(b.d_hash[0], n));
        SB_HIP(b.own, b.own.take(b.d_y[0], n));
        SB_HIP(b.own, hipMemcpyAsync(b.d_hash[0], hash, n * 4, hipMemcpyHostToDevice, ctx->stream));
        SB_HIP(b.own, hipMemcpyAsync(b.d_y[0], y, n * 8, hipMemcpyHostToDevice, ctx->stream));
        SB_HIP(b.own, hipStreamSynchronize(ctx->stream));
    }
    return end_resident(b);
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
