// rawdtw_keep_layout.h -- the store of kept chains (rawdtw_keep.hip): where a half's count and its seeds lie in the store's one device
// block, as byte offsets from (n_slots, N seeds a half).  Host and device code share it; no HIP include: a plain compiler takes it
// (tests/abi/keep_layout.cpp).
//
// A slot is a read's place; it has two halves, so that a round writes the half the read is NOT seeded from and a failed round leaves
// the other as it was.  A store address is slot * 2 + half.
//
//   region   bytes                                      what
//   counts   n_slots * 2 * 4, rounded up to 256         per half: the seeds it holds, or RAWDTW_NOT_KEPT
//   seeds    n_slots * 2 * stride                       per half: room for N 12-byte seeds; stride = N * 12 rounded up to 64
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RAWDTW_KEEP_HD __host__ __device__
#else
#define RAWDTW_KEEP_HD
#endif

namespace rawdtw {
namespace keep {

constexpr size_t kSeedBytes = 12;          // sizeof(rawdtw_seed_t)
constexpr uint64_t kMaxSeeds = 1u << 20;   // "resident_chains" at most
constexpr uint64_t kMaxSlots = 1u << 30;   // (a store address is a uint32_t other than 0xffffffff)

struct Layout {
    uint64_t n_slots = 0, n_seeds = 0; // n_seeds: N, the seeds a half holds
    size_t counts_bytes = 0, stride = 0, need = 0;

    RAWDTW_KEEP_HD uint64_t halves() const { return n_slots * 2; }
    RAWDTW_KEEP_HD static uint32_t address(uint32_t slot, uint32_t half) { return slot * 2u + half; }
    RAWDTW_KEEP_HD size_t count_at(uint64_t addr) const { return (size_t)addr * 4; }
    RAWDTW_KEEP_HD size_t seeds_at(uint64_t addr) const { return counts_bytes + (size_t)addr * stride; }
};

RAWDTW_KEEP_HD inline Layout layout(uint64_t n_slots, uint64_t n_seeds)
{
    Layout L;
    L.n_slots = n_slots; L.n_seeds = n_seeds;
    L.counts_bytes = ((size_t)n_slots * 2 * 4 + 255) & ~(size_t)255;
    L.stride = ((size_t)n_seeds * kSeedBytes + 63) & ~(size_t)63;
    L.need = L.counts_bytes + (size_t)n_slots * 2 * L.stride;
    return L;
}

} // namespace keep
} // namespace rawdtw
