// The kept-event filter cut into tiles (rawalign_amd/csrc/rawdtw_seed_tile.h: tile_next, tile_enters and the host restatement of the three
// launches) held to a copy of the serial loop (src/rsketch.c:243 and :172) under both rules, at tile sizes 1, 2, 3, 64 and kFilterTile:
// a stand-alone program, no HIP, no library.  tests/test_seed_resident_cpu.py builds it plain and with AddressSanitizer +
// UndefinedBehaviorSanitizer.  Every strand lies in a buffer of its own that ends where it ends.
//   seed_tile [STRANDS]   prints "ok N T", N the kept events compared and T the real tile size
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "rawdtw_seed_tile.h"

using namespace rawdtw::seed;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 20);
}

// the serial loop, written again: `last` is an index, as the reference keeps it
template <bool kMask> static void serial(const std::vector<float> &s, std::vector<uint32_t> &out)
{
    uint32_t last = 0;
    for (uint32_t i = 0; i < s.size(); i++) {
        const float d = s[i] - s[last];
        const bool near = i > 0 && std::fabs(d) < 0.3F;
        if (near || (kMask && s[i] == 3.402823466e+32F)) continue;
        last = i;
        out.push_back(i);
    }
}

static uint64_t compared = 0;

template <bool kMask> static bool same(const std::vector<float> &s, uint32_t T, const char *what)
{
    std::vector<uint32_t> want, got(s.size()), nxt(s.size()), ext(s.size());
    serial<kMask>(s, want);
    const uint32_t k = tiled_filter<kMask>(s.data(), (uint32_t)s.size(), T, got.data(), nxt.data(), ext.data());
    got.resize(k);
    compared += want.size();
    if (got == want) return true;
    fprintf(stderr, "%s: rule %s, tile %u, %zu events: %u kept, the serial loop keeps %zu\n", what, kMask ? "w = 0" : "w > 0", T, s.size(), k, want.size());
    return false;
}

static bool both(const std::vector<float> &s, const char *what)
{
    bool ok = true;
    for (uint32_t T : {1u, 2u, 3u, 64u, kFilterTile}) ok = same<true>(s, T, what) && same<false>(s, T, what) && ok;
    return ok;
}

// far-apart values: every event kept
static std::vector<float> all_kept(uint32_t n)
{
    std::vector<float> s(n);
    for (uint32_t i = 0; i < n; i++) s[i] = (float)(i % 7) * 0.5F + (i & 1 ? 10.0F : 0.0F);
    return s;
}

int main(int argc, char **argv)
{
    const int strands = argc > 1 ? atoi(argv[1]) : 3000;
    const uint32_t T = kFilterTile;
    const float mask = kMaskSignal, nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    bool ok = true;
    for (uint32_t n : {0u, 1u, T - 1, T, T + 1, 2 * T + 1}) {
        ok = both(all_kept(n), "all kept") && ok; // (an all-kept strand at every length)
        ok = both(std::vector<float>(n, 1.25F), "flat") && ok;
    }
    { // a flat stretch longer than two whole tiles, between kept events; drifting slowly inside (each against the LAST KEPT value)
        std::vector<float> s = all_kept(3 * T + 40);
        for (uint32_t i = T / 2; i < T / 2 + 2 * T + 9; i++) s[i] = 4.0F + 0.0001F * (float)(i % 1000);
        ok = both(s, "flat stretch") && ok;
    }
    for (int at_last = 0; at_last < 2; at_last++) { // the only kept event of a flat neighbourhood at a tile's last element and at its first
        std::vector<float> s(3 * T, 2.0F);
        s[at_last ? 2 * T - 1 : T] = 5.0F;
        ok = both(s, at_last ? "kept at a tile's last" : "kept at a tile's first") && ok;
    }
    for (float special : {nan, inf, -inf, mask}) { // on both sides of a tile boundary, at position 0 and at the strand's end
        for (uint32_t where = 0; where < 8; where++) {
            std::vector<float> s = where & 4 ? std::vector<float>(2 * T + 3, 0.5F) : all_kept(2 * T + 3);
            if (where & 1) s[T - 1] = special;
            if (where & 2) s[T] = special;
            if ((where & 3) == 0) { s[0] = special; s[2 * T + 2] = special; s[2 * T - 1] = s[2 * T] = special; }
            if ((where & 3) == 3) s[T + 1] = special; // (a run of three across the boundary)
            ok = both(s, "special values") && ok;
        }
    }
    { // the mask at position 0 under the w = 0 rule: `last` stays the mask, the next unmasked event is kept
        std::vector<float> s = {mask, 1.0F, 1.1F, mask, 1.2F, 2.0F};
        std::vector<uint32_t> want;
        serial<true>(s, want);
        ok = want == std::vector<uint32_t>{1, 5} && both(s, "mask first") && ok;
        s = {nan, 1.0F, 1.1F, 1.2F, nan, nan, 1.2F, 1.3F}; // a NaN kept keeps the event behind it
        want.clear();
        serial<false>(s, want);
        ok = want == std::vector<uint32_t>{0, 1, 4, 5, 6} && both(s, "nan") && ok;
    }
    // random strands over alphabets whose neighbours tie at the threshold, the specials sprinkled in
    const float levels[] = {0.0F, 0.1F, 0.3F, 0.30000004F, 0.29999998F, 0.6F, 0.9F, 1.5F, -0.3F, -0.31F, 2.0F, 2.2F};
    for (int it = 0; it < strands; it++) {
        const uint32_t a = 2 + rnd() % 11, n = it % 16 == 0 ? T + rnd() % (2 * T) : rnd() % 400, sprinkle = it % 3 ? 0 : 2 + rnd() % 30;
        std::vector<float> s(n);
        for (uint32_t i = 0; i < n; i++) {
            s[i] = levels[rnd() % a];
            if (sprinkle && rnd() % sprinkle == 0) { const float sp[] = {nan, inf, -inf, mask}; s[i] = sp[rnd() % 4]; }
        }
        const uint32_t tile = 1u + rnd() % 16;
        const bool one = both(s, "random") && same<true>(s, tile, "random") && same<false>(s, tile, "random");
        if (!one) { ok = false; break; }
    }
    if (!ok) return 1;
    printf("ok %llu %u\n", (unsigned long long)compared, T);
    return 0;
}
