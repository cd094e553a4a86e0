// The insertion of keys into the table's slots in any order (rawalign_amd/csrc/rawdtw_seed_tile.h: table_insert_step, table_log2_slots)
// held to a copy of fill_table's loop (rawdtw_seed_host.cpp: ascending hash order, the first free slot from first_slot on): a stand-alone
// program, no HIP, no library.  "Threads" hold one key each and are stepped one probe at a time, in ascending, descending and random order
// and in random interleavings.  tests/test_seed_resident_cpu.py builds it plain and with AddressSanitizer + UndefinedBehaviorSanitizer.
//   seed_insert [TABLES]   prints "ok N D", N the slots compared and D the displacements seen in descending order
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rawdtw_seed_tile.h"

using namespace rawdtw::seed;

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

constexpr uint32_t kInverse = 244002641u; // of first_slot's multiplier modulo 2^32: kInverse * 2654435761 == 1
static_assert((uint32_t)(kInverse * 2654435761u) == 1u, "the multiplier's inverse");

// a hash whose home slot in a table of 1 << lg slots is `home`; `low` picks among those that share it
static uint32_t hash_at(uint32_t home, uint32_t lg, uint32_t low)
{
    return (uint32_t)((home << (32 - lg) | (low & ((1u << (32 - lg)) - 1u))) * kInverse);
}

// fill_table's slots, as ranks: keys ascending, each to the first free slot from its home on
static std::vector<uint32_t> sequential(const std::vector<uint32_t> &keys, uint32_t lg)
{
    std::vector<uint32_t> tab((size_t)1 << lg, kNoEntry);
    const uint32_t mask = (uint32_t)tab.size() - 1;
    for (uint32_t r = 0; r < keys.size(); r++) {
        uint32_t at = first_slot(keys[r], lg);
        while (tab[at] != kNoEntry) at = (at + 1) & mask;
        tab[at] = r;
    }
    return tab;
}

struct Thread { uint32_t r, at; bool done; };

static uint64_t compared = 0, displaced_desc = 0;

// order: 0 ascending, 1 descending (each thread to its end before the next), 2 a random order likewise, 3 random interleaving
static bool same(const std::vector<uint32_t> &keys, int order)
{
    const uint32_t lg = table_log2_slots(keys.size()), mask = (1u << lg) - 1u;
    if (!lg || (1ull << lg) < 2 * keys.size() || (lg > 4 && (1ull << (lg - 1)) >= 2 * keys.size())) return false;
    const std::vector<uint32_t> want = sequential(keys, lg);
    std::vector<uint32_t> tab(want.size(), kNoEntry);
    uint64_t displaced = 0;
    auto amin = [&](uint32_t at, uint32_t r) {
        const uint32_t old = tab.at(at);
        if (r < old) { tab[at] = r; displaced += old != kNoEntry; }
        return old;
    };
    std::vector<Thread> th(keys.size());
    for (uint32_t r = 0; r < keys.size(); r++) th[r] = Thread{r, first_slot(keys[r], lg), false};
    std::vector<uint32_t> turn(keys.size());
    for (uint32_t i = 0; i < turn.size(); i++) turn[i] = order == 1 ? (uint32_t)turn.size() - 1 - i : i;
    if (order >= 2)
        for (size_t i = turn.size(); i > 1; i--) std::swap(turn[i - 1], turn[rnd() % i]);
    if (order < 3) {
        for (uint32_t t : turn)
            while (!table_insert_step(amin, th[t].r, th[t].at, mask)) {}
    } else {
        std::vector<uint32_t> live = turn;
        while (!live.empty()) { // one probe of one thread at a time
            const size_t i = rnd() % live.size();
            Thread &t = th[live[i]];
            if (table_insert_step(amin, t.r, t.at, mask)) { live[i] = live.back(); live.pop_back(); }
        }
    }
    if (order == 1) displaced_desc += displaced;
    compared += want.size();
    if (tab == want) return true;
    fprintf(stderr, "order %d: %zu keys in %zu slots differ from sequential insertion\n", order, keys.size(), want.size());
    return false;
}

static bool every_order(std::vector<uint32_t> keys)
{
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    bool ok = true;
    for (int order = 0; order < 4; order++) ok = same(keys, order) && ok;
    return ok && same(keys, 3);
}

int main(int argc, char **argv)
{
    const int tables = argc > 1 ? atoi(argv[1]) : 3000;
    bool ok = table_log2_slots(0) == 4 && table_log2_slots(8) == 4 && table_log2_slots(9) == 5 && table_log2_slots(1u << 30) == 31 &&
              table_log2_slots((1ull << 30) + 1) == 0;
    for (uint32_t n : {0u, 1u, 8u, 9u}) { // (the lg 4 -> 5 edge)
        std::vector<uint32_t> keys;
        for (uint32_t i = 0; i < n; i++) keys.push_back(rnd());
        ok = every_order(keys) && ok;
    }
    for (uint32_t n : {8u, 200u}) { // every key on one home slot
        const uint32_t lg = table_log2_slots(n);
        std::vector<uint32_t> keys;
        for (uint32_t i = 0; i < n; i++) keys.push_back(hash_at(5, lg, i * 7919u + 1));
        for (uint32_t k : keys) ok = first_slot(k, lg) == 5 && ok;
        ok = every_order(keys) && ok;
    }
    { // a cluster that starts in the last slot and wraps, beside keys at the table's start that it has to pass
        const uint32_t n = 40, lg = table_log2_slots(n), last = (1u << lg) - 1;
        std::vector<uint32_t> keys;
        for (uint32_t i = 0; i < 12; i++) keys.push_back(hash_at(last, lg, i * 104729u + 3));
        for (uint32_t i = 0; i < 10; i++) keys.push_back(hash_at(last - 2, lg, i * 31u + 1));
        for (uint32_t i = 0; i < 18; i++) keys.push_back(hash_at(i % 4, lg, i * 977u + 5));
        ok = keys.size() == n && every_order(keys) && ok;
        std::sort(keys.begin(), keys.end());
        const std::vector<uint32_t> tab = sequential(keys, lg);
        ok = tab[0] != kNoEntry && tab[last] != kNoEntry && first_slot(keys[tab[0]], lg) >= last - 2 && ok; // (it did wrap)
    }
    for (int it = 0; it < tables && ok; it++) { // random tables at load just under 0.5, hashes clustered on few home slots every other time
        const uint32_t lg = 4 + rnd() % 6, n = (1u << (lg - 1)) - rnd() % 3;
        std::vector<uint32_t> keys;
        while (keys.size() < n) {
            keys.push_back(it & 1 ? hash_at(rnd() % (1u << lg) % (1 + rnd() % 8) * 3 % (1u << lg), lg, rnd()) : rnd());
            std::sort(keys.begin(), keys.end());
            keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        }
        ok = table_log2_slots(n) == lg && every_order(keys);
    }
    ok = ok && displaced_desc > 0; // the descending order was seen to displace
    if (!ok) return 1;
    printf("ok %llu %llu\n", (unsigned long long)compared, (unsigned long long)displaced_desc);
    return 0;
}
