// The packed records a device-planned batch hands from k_plan to k_runs (rawdtw_runs.hip), and the host reads back in the
// plan's self-check and profile (rawdtw_plan_check.cpp): their one definition.  Shared by the kernels, the host and a plain
// C++ test program (tests/abi/plan_fmt.cpp): no HIP include here, plain 32-bit words in and out.  Every site packs and reads
// through these functions; to change a format, change it here (the static_asserts say what has to fit) and run that test.
//
//   pass entry   StreamArgs::todo, one a PASS (a tile's tile-class parts, or as many of them as fit the image budget and
//                the run table), at the index of its slot: [0, cnt[kCntTodo]) the listed tiles' first passes,
//                [n_tiles, n_tiles + cnt[kCntPool]) the others.
//                  x  tile            y  copy-order slot
//                  z  jobs | runs << 16 | n_hi << 22     (n_hi: the pass's first radius-1 record, rawdtw_chunks.h)
//                  w  region | rec0 << 16                (region: floats of the image's event region; rec0: the pass's
//                                                         first record in its tile's stretch of kStreamRecStride, even)
//   job record   StreamArgs::recs, n_tiles x kStreamRecStride, a pass's in the order the lanes take them (sort_bin).
//                  x  long window | short window << 16   (float offsets into the pass's image, longer sequence first)
//                  y  N | M << 7 | R << 14 | excl << 16 | item << 17
//                     (N >= M the sides, R the slanted radius, excl: exclude_last; item u = the part that ends at anchor
//                      (tile end - 1 - u): its cost goes to out[that anchor])
//   copy order   StreamArgs::runtab, n_slots x 2 kStreamMaxSeg, entry 2 g + w = run g of arena w (0 events, 1 reference):
//                  the 16-byte pieces [x, y) of the image come from arena float index 4 piece + (int64)(z | w << 32).
//   sort bin     (3 - R) * 64 + (63 - min(N, 63)): radius 3 first, then 2, then 1, each run longest first; sides of 63
//                and more share a bin.
//   item word    k_plan's own word per item (tm[]): its low 17 bits are the record's y without the item (rec_shape), above
//                them the kItem* bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RAWDTW_FMT_FN __host__ __device__ constexpr inline
#else
#define RAWDTW_FMT_FN constexpr inline
#endif

namespace rawdtw {

// ---- what the widths depend on ----
constexpr int kMaxLaneRadius = 3;      // lane-per-job DP is instantiated for R in [0, 3]: a sweep showed that the rare
                                       // jobs with larger radii (0.4 % of a sparse batch) cost half of the tile kernel's
                                       // time through divergence and register pressure; they go to k_band_wreg<1>
constexpr int kLaneMaxN = 73;          // ... and for jobs whose longer side is at most this
constexpr uint32_t kStreamTile = 512;         // anchors (= candidate parts) of a tile: what one wave of the scan plans (eight a lane)
constexpr uint32_t kStreamRecStride = 576;    // job records of a tile: its passes' records one behind the other, each pass on a 16-byte boundary
constexpr uint32_t kStreamMaxSeg = 32;        // runs of one pass over a tile's image (more: the tile takes another pass)
constexpr uint32_t kStreamMaxImageFloats = 40000; // the most the "tile_lds_floats" option admits (rawdtw_set_option)

// Device job record, 32 bytes, in PLAN order.  Written by the planner.
struct DevJob {
    uint64_t ref_off;  // element offset of b[0] in the reference arena
    uint32_t read_off; // element offset of a[0] in the event arena
    uint32_t n;        // a_length
    uint32_t m;        // b_length
    int32_t R;         // banded: radius AFTER the slant correction (dtw.cpp:298-300); full: -1
    uint32_t flags;    // bit0: exclude_last_element
    uint32_t aux;      // the job's index in the caller's batch: kernels store their cost at out[aux]
};
static_assert(sizeof(DevJob) == 32, "DevJob must stay 32 bytes");

enum : uint32_t { kFlagExcludeLast = 1u };

// post-slant radius, dtw.cpp:298-300 (unsigned 32-bit arithmetic for the correction)
inline int slanted_radius(uint32_t n, uint32_t m, int r0)
{
    uint32_t N = n > m ? n : m, M = n > m ? m : n;
    uint32_t extra = ((N - M) * (uint32_t)r0 + N - 1u) / N;
    return r0 + (int)extra;
}

// The three records as the host holds them (the kernels keep uint4 / uint2: same words, same order).
struct PassEntry { uint32_t x, y, z, w; };
struct JobRec { uint32_t x, y; };
struct CopyOrder { uint32_t x, y, z, w; };

// ---- job record ----
constexpr uint32_t kRecSideBits = 7, kRecRadiusBits = 2, kRecItemBits = 9;
constexpr uint32_t kRecMShift = kRecSideBits, kRecRadiusShift = 2 * kRecSideBits, kRecExclShift = kRecRadiusShift + kRecRadiusBits,
                   kRecItemShift = kRecExclShift + 1;
constexpr uint32_t kRecSideMask = (1u << kRecSideBits) - 1u, kRecRadiusMask = (1u << kRecRadiusBits) - 1u,
                   kRecShapeMask = (1u << kRecItemShift) - 1u; // y without the item
static_assert((uint32_t)kLaneMaxN <= kRecSideMask, "a record's N and M: 7 bits");
static_assert((uint32_t)kMaxLaneRadius <= kRecRadiusMask, "a record's radius: 2 bits");
static_assert(kStreamTile == 1u << kRecItemBits && kRecItemShift + kRecItemBits <= 32, "a record's item: 9 bits, a power of two (rec_item masks with kStreamTile - 1)");
static_assert(kStreamMaxImageFloats <= 0xffffu, "window offsets and a pass's event region: 16 bits");

RAWDTW_FMT_FN uint32_t rec_windows(uint32_t p_long, uint32_t p_short) { return p_long | (p_short << 16); }
RAWDTW_FMT_FN uint32_t rec_long(uint32_t x) { return x & 0xffffu; }
RAWDTW_FMT_FN uint32_t rec_short(uint32_t x) { return x >> 16; }
RAWDTW_FMT_FN uint32_t rec_shape(uint32_t N, uint32_t M, uint32_t R, uint32_t excl)
{
    return N | (M << kRecMShift) | (R << kRecRadiusShift) | (excl << kRecExclShift);
}
// (`shape` may carry bits above the record's: an item word of k_plan)
RAWDTW_FMT_FN uint32_t rec_with_item(uint32_t shape, uint32_t item) { return (shape & kRecShapeMask) | (item << kRecItemShift); }
RAWDTW_FMT_FN uint32_t rec_n(uint32_t y) { return y & kRecSideMask; }
RAWDTW_FMT_FN uint32_t rec_m(uint32_t y) { return (y >> kRecMShift) & kRecSideMask; }
RAWDTW_FMT_FN uint32_t rec_radius(uint32_t y) { return (y >> kRecRadiusShift) & kRecRadiusMask; }
RAWDTW_FMT_FN uint32_t rec_excl(uint32_t y) { return (y >> kRecExclShift) & 1u; }
RAWDTW_FMT_FN uint32_t rec_item(uint32_t y) { return (y >> kRecItemShift) & (kStreamTile - 1u); }

// ---- k_plan's item word: rec_shape in the low bits, then ----
constexpr uint32_t kItemSwapped = kRecItemShift,      // the reference window is the longer one
                   kItemRunStart = kRecItemShift + 1, // its predecessor along the chain is no tile part
                   kItemRunEnd = kRecItemShift + 2,   // its successor is none
                   kItemTile = kRecItemShift + 3;     // a tile-class part at all (0: the lane bodies do not take it)
// ... and its packed running sums: floats of the event region | run starts << 20
constexpr uint32_t kSumRunShift = 20, kSumFloatsMask = (1u << kSumRunShift) - 1u;
static_assert(kStreamTile * ((uint32_t)kLaneMaxN + 6u) <= kSumFloatsMask && kStreamTile < 1u << (32 - kSumRunShift), "a tile's sums");

// ---- pass entry ----
constexpr uint32_t kPassRunsShift = 16, kPassRunsBits = 6, kPassNHiShift = kPassRunsShift + kPassRunsBits;
constexpr uint32_t kPassJobsMask = (1u << kPassRunsShift) - 1u, kPassRunsMask = (1u << kPassRunsBits) - 1u;
static_assert(kStreamTile <= kPassJobsMask, "an entry's jobs: 16 bits");
static_assert(kStreamMaxSeg <= kPassRunsMask, "an entry's runs: 6 bits");
static_assert(kStreamTile < 1u << (32 - kPassNHiShift), "an entry's first radius-1 record: 10 bits");
static_assert(kStreamRecStride <= 0xffffu && kStreamRecStride >= kStreamTile, "an entry's first record: 16 bits");

RAWDTW_FMT_FN uint32_t pass_counts(uint32_t jobs, uint32_t runs, uint32_t n_hi) { return jobs | (runs << kPassRunsShift) | (n_hi << kPassNHiShift); }
RAWDTW_FMT_FN uint32_t pass_jobs(uint32_t z) { return z & kPassJobsMask; }
RAWDTW_FMT_FN uint32_t pass_runs(uint32_t z) { return (z >> kPassRunsShift) & kPassRunsMask; }
RAWDTW_FMT_FN uint32_t pass_n_hi(uint32_t z) { return z >> kPassNHiShift; }
RAWDTW_FMT_FN uint32_t pass_place(uint32_t region, uint32_t rec0) { return region | (rec0 << 16); }
RAWDTW_FMT_FN uint32_t pass_region(uint32_t w) { return w & 0xffffu; }
RAWDTW_FMT_FN uint32_t pass_rec0(uint32_t w) { return w >> 16; }

// ---- copy order: the source offset's two words ----
RAWDTW_FMT_FN uint32_t order_src_lo(long long src) { return (uint32_t)(unsigned long long)src; }
RAWDTW_FMT_FN uint32_t order_src_hi(long long src) { return (uint32_t)((unsigned long long)src >> 32); }
RAWDTW_FMT_FN long long order_src(uint32_t z, uint32_t w) { return (long long)((unsigned long long)z | ((unsigned long long)w << 32)); }

// ---- the lanes' order ----
constexpr uint32_t kSortBins = 192;
// (= (3 - R) * 64 + (63 - min(N, 63)), written as one difference: in the other form k_plan, at the edge of its register
// budget, spills one more register -- profiles/plan_fmt_codegen.json)
RAWDTW_FMT_FN uint32_t sort_bin(uint32_t R, uint32_t N) { return 3u * 64u + 63u - R * 64u - (N < 63u ? N : 63u); }
// The first radius-1 bin.  Its first place -- the pass's first radius-1 record -- goes into the pass's entry (n_hi): k_runs
// starts the radius-1 run on a chunk boundary of its own, so that no wave holds parts of both radius 2 and radius 1.
constexpr uint32_t kSortBinRadius1 = sort_bin(1u, kRecSideMask);
static_assert(kMaxLaneRadius == 3 && sort_bin(3u, kRecSideMask) == 0u && sort_bin(1u, 0u) == kSortBins - 1u && kSortBinRadius1 == 128u, "the bins");

} // namespace rawdtw
