// The minimizer window's step (rawalign_amd/csrc/rawdtw_seed_min.h) held to the serial loop of ri_sketch_min (src/rsketch.c:193-220, as
// rawdtw_seed_host.cpp restates it) on random hash strings: a stand-alone program, no HIP, no library.  tests/test_seed_build_min_cpu.py
// builds it plain and with AddressSanitizer + UndefinedBehaviorSanitizer.  Every step gets exactly the hashes it may read, in a buffer
// of its own that ends where they end, so that a read outside max(0, m - w) .. m is one the sanitizer sees.
//   seed_min [STRINGS]   prints "ok N", N the elements compared
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rawdtw_seed_min.h"

using namespace rawdtw::seed;

// the serial state machine over e-mer hashes: x = hash << 6 | span, y = the e-mer's index (its first event's position in the reference)
static void serial(const std::vector<uint32_t> &h, int w, std::vector<uint32_t> &out)
{
    struct Item { uint64_t x, y; };
    const uint64_t none = ~0ull, span = 11;
    Item buf[256], mn = {none, none};
    for (int j = 0; j < w; j++) buf[j] = Item{none, none};
    int buf_pos = 0, min_pos = 0;
    uint32_t l = 0; // e-mers so far (the reference counts kept events: l there is this l + e - 1)
    auto push = [&](const Item &it) { out.push_back((uint32_t)it.y); };
    for (size_t m = 0; m < h.size(); m++) {
        l++;
        const Item info = {(uint64_t)h[m] << 6 | span, m};
        buf[buf_pos] = info;
        if (l == (uint32_t)w && mn.x != none) {
            for (int j = buf_pos + 1; j < w; ++j)
                if (mn.x == buf[j].x && buf[j].y != mn.y) push(buf[j]);
            for (int j = 0; j < buf_pos; ++j)
                if (mn.x == buf[j].x && buf[j].y != mn.y) push(buf[j]);
        }
        if (info.x <= mn.x) {
            if (l >= (uint32_t)w + 1 && mn.x != none) push(mn);
            mn = info; min_pos = buf_pos;
        } else if (buf_pos == min_pos) {
            if (l >= (uint32_t)w && mn.x != none) push(mn);
            mn.x = none;
            for (int j = buf_pos + 1; j < w; ++j)
                if (mn.x >= buf[j].x) { mn = buf[j]; min_pos = j; }
            for (int j = 0; j <= buf_pos; ++j)
                if (mn.x >= buf[j].x) { mn = buf[j]; min_pos = j; }
            if (l >= (uint32_t)w && mn.x != none) {
                for (int j = buf_pos + 1; j < w; ++j)
                    if (mn.x == buf[j].x && mn.y != buf[j].y) push(buf[j]);
                for (int j = 0; j <= buf_pos; ++j)
                    if (mn.x == buf[j].x && mn.y != buf[j].y) push(buf[j]);
            }
        }
        if (++buf_pos == w) buf_pos = 0;
    }
    if (mn.x != none) push(mn);
}

int main(int argc, char **argv)
{
    const long strings = argc > 1 ? atol(argv[1]) : 4000;
    const int ws[] = {1, 2, 3, 4, 5, 7, 10, 16, 63, 64, 65, 255}, letters[] = {2, 3, 5, 50};
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    uint64_t compared = 0, over = 0;
    for (long s = 0; s < strings; s++) {
        const int w = ws[s % 12], a = letters[(s / 12) % 4];
        const uint32_t M = (uint32_t)(next() % (s % 3 ? (uint64_t)w + 4 : 700));
        std::vector<uint32_t> h(M), want, got;
        for (uint32_t &x : h) x = (uint32_t)(next() % a) * 0x10001u + (a == 50 ? 0xFFFFFF00u : 0u); // (a == 50: hashes at the top of 32 bits)
        serial(h, w, want);
        for (uint32_t m = 0; m < M; m++) {
            const uint32_t base = m >= (uint32_t)w ? m - w : 0;
            std::vector<uint32_t> window(h.begin() + base, h.begin() + m + 1); // what the step may read, and no more
            const uint32_t c = min_step_count(window.data(), base, m, M, w);
            std::vector<uint32_t> idx(c);
            if (min_step_emit(window.data(), base, m, M, w, idx.data()) != c) { fprintf(stderr, "string %ld, step %u: the two calls disagree\n", s, m); return 1; }
            got.insert(got.end(), idx.begin(), idx.end());
        }
        if (got != want) { fprintf(stderr, "string %ld (w %d, %d letters, %u e-mers): %zu elements, the serial loop %zu\n", s, w, a, M, got.size(), want.size()); return 1; }
        compared += want.size();
        over += want.size() > M;
    }
    printf("ok %" PRIu64 "\n", compared);
    fprintf(stderr, "strings with more elements than e-mers: %" PRIu64 "\n", over);
    return 0;
}
