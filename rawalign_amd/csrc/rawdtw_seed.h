// rawdtw_seed.h -- what the host side (rawdtw_seed_host.cpp) and the device path (rawdtw_seed.hip) of seeding share: the seed index's
// record, its table slot, the hash and the code of an event.  Internal: nothing here is part of the ABI.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/rawdtw.h"

#if defined(__HIPCC__)
#define RAWDTW_HD __host__ __device__
#else
#define RAWDTW_HD
#endif

namespace rawdtw {
namespace seed {

constexpr float kLastSigDiff = 0.3F;            // LAST_SIG_DIFF, rsketch.h:10
constexpr float kMaskSignal = 3.402823466e+32F; // RI_MASK_SIGNAL, rsketch.h:8

// One slot of the open-addressing table, the same 16 bytes on the host and on the device.  count == 0: empty (every 32-bit
// value is a legal key); count == 1: val is the position; else val is the list's first entry in the position array.
struct Slot {
    uint32_t key, count;
    uint64_t val;
};
static_assert(sizeof(Slot) == 16, "a probe is one 16-byte load");

// hash64 with the 32-bit mask (rsketch.c:6-15) in 32-bit arithmetic: the first step's `& mask` drops everything above bit 31 of
// the key, and every later step is masked again or xors a right shift in, so the upper half never reaches the result
// (tests/test_seed_host.py checks this against the 64-bit form).
RAWDTW_HD inline uint32_t hash32(uint32_t key)
{
    key = ~key + (key << 21);
    key = key ^ key >> 24;
    key = (key + (key << 3)) + (key << 8);
    key = key ^ key >> 14;
    key = (key + (key << 2)) + (key << 4);
    key = key ^ key >> 28;
    key = key + (key << 31);
    return key;
}

// where a hash's probe sequence starts in a table of 1 << log2_slots slots (Fibonacci hashing on top of the key: its low bits
// alone are the reference's bucket number and need not be even for a crafted index)
RAWDTW_HD inline uint32_t first_slot(uint32_t hash, uint32_t log2_slots)
{
    return log2_slots ? (uint32_t)(hash * 2654435761u) >> (32 - log2_slots) : 0u;
}

// the (lq + 2)-bit code of an event (rsketch.c:246-247): its sign and top exponent bit, then lq bits from bit 32 - q on
RAWDTW_HD inline uint32_t code_of(uint32_t bits, uint32_t q, uint32_t lq)
{
    return bits >> 30 << lq | ((bits >> (32 - q)) & ((1u << lq) - 1u));
}

// rsketch.c:243: the event at i is skipped against the last kept one (ordered compares: a NaN is kept)
RAWDTW_HD inline bool skipped(float x, float last, bool first)
{
    const float d = x - last;
    return (!first && (d < 0.0f ? -d : d) < kLastSigDiff) || x == kMaskSignal;
}

// rsketch.c:172: the minimizer sketch's form of the same test -- no RI_MASK_SIGNAL clause: a masked value is kept and coded
RAWDTW_HD inline bool skipped_min(float x, float last, bool first)
{
    const float d = x - last;
    return !first && (d < 0.0f ? -d : d) < kLastSigDiff;
}

// w, e, n, q, lq, k as ri_idx_t keeps them; RAWDTW_ERR_INVALID where the reference asserts or shifts out of range
int check_pars(const rawdtw_seed_pars_t *p);

// What the builders of an index share (rawdtw_seed_host.cpp defines them; rawdtw_seed_build.hip is the second user): an entry of the
// sketch, the table from entries grouped by hash with each hash's positions in the order ri_idx_get gives them, and an index's serial.
struct Entry { uint32_t hash; uint64_t y; };
int fill_table(rawdtw_seed_index *six, const std::vector<Entry> &a);
uint64_t next_serial();
bool entries_sorted(uint64_t n, const uint32_t *hash, const uint64_t *y); // by (hash, y), equal entries allowed

} // namespace seed
} // namespace rawdtw

struct rawdtw_seed_index {
    uint64_t serial = 0; // unique among the process's indices (never reused, unlike an address): what a context's table is known by
    rawdtw_seed_pars_t pars{};
    uint32_t n_seq = 0;
    uint32_t log2_slots = 0;
    std::vector<rawdtw::seed::Slot> slots; // 1 << log2_slots, load at most 0.5
    std::vector<uint64_t> pos;             // the lists of the keys with more than one position, each ascending
    uint64_t n_keys = 0, n_positions = 0;  // (n_positions: every key's, single ones included)
    // A resident index (rawdtw_seed_index_build_resident, rawdtw_seed_table_from_entries) has no host copy until rawdtw_seed_index_fetch:
    // slots and pos are empty, the table is the context's (rawdtw_seed.hip: SeedWs) under this serial, and n_list counts its list words.
    bool resident = false;
    uint64_t n_list = 0;
    const rawdtw_ctx *owner = nullptr; // (compared, never followed: the context may be gone)
};
