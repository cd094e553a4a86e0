// rawdtw_sort_order.h against std::sort itself, permutation for permutation, in a program of its own (tests/test_sort_order_cpu.py builds
// it plain and with AddressSanitizer + UndefinedBehaviorSanitizer: the permutation and the stack are exact-size heap arrays, so a store
// past either is caught).  The cases are the Python test's recipe: every n from 0 to 300, 1 000 and 4 096; scores from alphabets of 1, 2, 3, 5,
// 17 and n values; random (8 draws), ascending, descending, all equal and organ-pipe.  A file of scores given as argv[1] (one a line: the
// frozen adversary) is sorted too and must reach the heap phase.  Prints "ok <cases> heap <cases that reached the heap phase>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rawdtw_sort_order.h"

namespace so = rawdtw::sort_order;

struct Item { float score; uint32_t idx; };

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t below)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % below);
}

static uint32_t stack_need(uint32_t n)
{
    uint32_t lg = 0;
    while ((n >> (lg + 1)) != 0) lg++;
    return 2 * lg + 1;
}

// false: the restated order differs from std::sort's
static bool check(const std::vector<float> &score, uint32_t *phases)
{
    const uint32_t n = (uint32_t)score.size();
    std::vector<Item> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = Item{score[i], i};
    std::sort(v.begin(), v.end(), [](const Item &a, const Item &b) { return a.score > b.score; });
    // exact sizes, on the heap: the sanitizer sees the first store past them
    uint32_t *perm = new uint32_t[n];
    const uint32_t cap = n <= so::kMaxElements ? std::min(so::kStackCap, stack_need(n)) : stack_need(n);
    so::Range *stack = new so::Range[cap];
    float *sc = new float[n];
    for (uint32_t i = 0; i < n; i++) { perm[i] = i; sc[i] = score[i]; }
    bool ok = so::sort_order_desc((const float *)sc, perm, n, stack, cap, phases);
    for (uint32_t i = 0; ok && i < n; i++) ok = perm[i] == v[i].idx;
    delete[] perm; delete[] stack; delete[] sc;
    return ok;
}

int main(int argc, char **argv)
{
    std::vector<uint32_t> sizes;
    for (uint32_t n = 0; n <= 300; n++) sizes.push_back(n);
    sizes.push_back(1000); sizes.push_back(4096);
    unsigned long cases = 0, heap = 0;
    for (uint32_t n : sizes)
        for (uint32_t alpha : {1u, 2u, 3u, 5u, 17u, 0u}) {
            const uint32_t a = alpha ? alpha : (n ? n : 1);
            for (int order = 0; order < 12; order++) { // 0 .. 7 random, 8 ascending, 9 descending, 10 all equal, 11 organ-pipe
                std::vector<float> s(n);
                for (uint32_t i = 0; i < n; i++) {
                    uint32_t x;
                    if (order < 8) x = rnd(a);
                    else if (order == 8) x = (uint32_t)((uint64_t)i * a / n);
                    else if (order == 9) x = (uint32_t)((uint64_t)(n - 1 - i) * a / n);
                    else if (order == 10) x = a - 1;
                    else x = (uint32_t)((uint64_t)std::min(i, n - 1 - i) * 2 * a / n) % a;
                    s[i] = 10.0f + (float)x;
                }
                uint32_t ph = 0;
                if (!check(s, &ph)) { printf("differs: n %u alphabet %u order %d\n", n, a, order); return 1; }
                cases++; heap += (ph & so::kRanHeap) != 0;
            }
        }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
        std::vector<float> s;
        float x;
        while (fscanf(f, "%f", &x) == 1) s.push_back(x);
        fclose(f);
        uint32_t ph = 0;
        if (!check(s, &ph)) { printf("differs: the adversary of %zu\n", s.size()); return 1; }
        if (!(ph & so::kRanHeap)) { printf("the adversary of %zu did not reach the heap phase\n", s.size()); return 3; }
        cases++; heap++;
    }
    printf("ok %lu heap %lu\n", cases, heap);
    return 0;
}
