// rawdtw_seed_tile.h -- the two constructions of the resident seed index (rawdtw_seed_build.hip: rawdtw_seed_index_build_resident) as
// functions a plain compiler takes too: the kept-event filter cut into tiles, and the insertion of a key into the table's slots in any
// order.  The kernels and the host restatements (below; tests/abi/seed_tile.cpp, tests/abi/seed_insert.cpp) call the same code, as
// rawdtw_seed_min.h is shared for the window.  No HIP include.
//
// The filter.  rsketch.c:243 / :172 keep event i iff it is not skipped against the value of the last kept event: one float of carried
// state.  A strand is cut into tiles of kFilterTile events.  Inside a tile, for every i:
//   next(i)  the first j > i of the tile that is not skipped against x[i] (first = false), or none
//   exit(i)  the last element of the chain i, next(i), next(next(i)), ...
// Neither reads anything outside the tile.  If the serial loop keeps i, the next event it keeps is next(i) as long as that lies in the
// tile: the test of j against `last = x[i]` is the very test next(i) scans with.  So a tile's kept events are the chain from its ENTRY --
// its first element not skipped against the value v carried in -- and the value carried out is x[exit(entry)] (v itself where the tile
// has no entry).  The strand's carry starts as s[0], and `first` is true for event 0 alone, as k_sb_filter starts.
// Two cases fall out of this rather than being handled: event 0 masked under the w = 0 rule leaves v the mask, against which the next
// unmasked event is far away and kept; a NaN kept makes every compare against it unordered, so the event behind it is next(i).
//
// The insertion.  fill_table (rawdtw_seed_host.cpp) puts the keys down in ascending hash order, each in the first free slot from its
// home slot on.  With the keys known by their rank in that order, the same layout comes out of any schedule: a slot holds the smallest
// rank that ever probed it (atomic min), and whoever loses a slot -- the newcomer with the larger rank, or the holder it displaced --
// moves on to the next one.  By induction over the ranks: rank r's final slot is the first slot from its home on that no smaller rank
// ends in, which is where sequential insertion puts it.
#pragma once
#include <cstdint>

#include "rawdtw_seed.h"

namespace rawdtw {
namespace seed {

constexpr uint32_t kFilterTile = 2048;    // T: the events of a tile (next and the chain's length share a 32-bit word: T < 2^16)
constexpr uint32_t kNoEntry = 0xffffffffu; // a tile that keeps nothing; an empty slot of the rank table
static_assert(kFilterTile >= 64 && kFilterTile < 65536 && kFilterTile % 256 == 0, "a tile's offsets are 16 bits; a workgroup of 256 takes it in whole rounds");

// the tiles of a strand of len events
RAWDTW_HD inline uint32_t filter_tiles(uint32_t len)
{
    return (uint32_t)(((uint64_t)len + kFilterTile - 1) / kFilterTile);
}

// the rule switch: kMask is the w == 0 rule (rsketch.c:243), without it ri_sketch_min's (rsketch.c:172)
template <bool kMask> RAWDTW_HD inline bool tile_skipped(float x, float last, bool first)
{
    return kMask ? skipped(x, last, first) : skipped_min(x, last, first);
}

// next(i) in a tile of n values; n: none
template <bool kMask> RAWDTW_HD inline uint32_t tile_next(const float *x, uint32_t i, uint32_t n)
{
    const float xi = x[i];
    uint32_t j = i + 1;
    while (j < n && tile_skipped<kMask>(x[j], xi, false)) j++;
    return j;
}

// the entry test of one element against the carried value (strand_first: the element is the strand's event 0)
template <bool kMask> RAWDTW_HD inline bool tile_enters(float x, float v, bool strand_first)
{
    return !tile_skipped<kMask>(x, v, strand_first);
}

// One probe of the insertion: amin(at, r) is an atomic minimum on slot `at` of the rank table that returns what was there.  True: the
// rank carried has found its slot.  Else r and at are what to probe with next (r may now be the rank that was displaced).
template <typename AtomicMin> RAWDTW_HD inline bool table_insert_step(AtomicMin amin, uint32_t &r, uint32_t &at, uint32_t mask)
{
    const uint32_t old = amin(at, r);
    if (old == kNoEntry) return true;
    if (old > r) r = old; // (the slot is r's now; its holder moves on)
    at = (at + 1) & mask;
    return false;
}

// the table's size as fill_table takes it: the smallest lg >= 4 with 2^lg >= 2 * n_keys; 0: beyond 2^31 slots (RAWDTW_ERR_RANGE)
RAWDTW_HD inline uint32_t table_log2_slots(uint64_t n_keys)
{
    uint32_t lg = 4;
    while (lg < 31 && (1ull << lg) < 2 * n_keys) lg++;
    return (1ull << lg) < 2 * n_keys ? 0u : lg;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host restatement of the three launches, at any tile size: what the kernels do, in their order, on one strand.  For tests.
// kept_pos, nxt and ext have room for n words; returns the kept events.
template <bool kMask> inline uint32_t tiled_filter(const float *s, uint32_t n, uint32_t T, uint32_t *kept_pos, uint32_t *nxt, uint32_t *ext)
{
    const uint32_t tiles = (uint32_t)(((uint64_t)n + T - 1) / T);
    // per tile (k_sb_next): next, then exit through next from the tile's end backwards
    for (uint32_t t = 0; t < tiles; t++) {
        const uint32_t i0 = t * T, tn = n - i0 < T ? n - i0 : T;
        for (uint32_t j = 0; j < tn; j++) nxt[i0 + j] = tile_next<kMask>(s + i0, j, tn);
        for (uint32_t j = tn; j-- > 0;) ext[i0 + j] = nxt[i0 + j] < tn ? ext[i0 + nxt[i0 + j]] : j;
    }
    // per strand (k_sb_chain) and per tile again (k_sb_mark)
    float v = n ? s[0] : 0.0f;
    uint32_t kept = 0;
    for (uint32_t t = 0; t < tiles; t++) {
        const uint32_t i0 = t * T, tn = n - i0 < T ? n - i0 : T;
        uint32_t entry = kNoEntry;
        for (uint32_t j = 0; j < tn && entry == kNoEntry; j++)
            if (tile_enters<kMask>(s[i0 + j], v, i0 + j == 0)) entry = j;
        if (entry == kNoEntry) continue;
        v = s[i0 + ext[i0 + entry]];
        for (uint32_t j = entry; j < tn; j = nxt[i0 + j]) kept_pos[kept++] = i0 + j;
    }
    return kept;
}
#endif

} // namespace seed
} // namespace rawdtw
