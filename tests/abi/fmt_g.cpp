// fmt_g.cpp -- rawalign_amd/csrc/rawdtw_fmt_g.h against the C library, as a stand-alone program (tests/test_aln_text_cpu.py builds it
// plain and with AddressSanitizer + UndefinedBehaviorSanitizer, together with rawdtw_aln_text.cpp).
//   fmt_g values FILE   every uint32 of FILE as a float's bits: fmt_g's bytes against snprintf("%g", (double)x).  "ok N"
//   fmt_g all T         all 2^32 bit patterns on T threads (outside the suite: minutes).  "ok 4294967296"
//   fmt_g u64           uint64 -> decimal: every power of ten +- 1, 2^32 +- 1, 2^64 - 1, 0, against snprintf("%llu").  "ok N"
//   fmt_g host          rawdtw_aln_text_host on a few jobs against snprintf, exact-size buffers (the sanitizer watches their ends).  "ok N"
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rawdtw.h"
#include "rawdtw_fmt_g.h"

using namespace rawdtw;

static bool check_bits(uint32_t bits)
{
    float x;
    memcpy(&x, &bits, 4);
    char want[64], got[17];
    const int n = snprintf(want, sizeof want, "%g", (double)x);
    const fmtg::Text t = fmtg::fmt_g(bits);
    if (t.len > 16) return false;
    fmtg::text_put(got, t);
    return (int)t.len == n && memcmp(want, got, (size_t)n) == 0;
}

static int report(uint32_t bits)
{
    float x;
    memcpy(&x, &bits, 4);
    char got[17] = {0};
    const fmtg::Text t = fmtg::fmt_g(bits);
    fmtg::text_put(got, t);
    printf("mismatch at 0x%08x: snprintf \"%g\", fmt_g \"%.*s\"\n", bits, (double)x, (int)t.len, got);
    return 1;
}

static int run_values(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { printf("cannot open %s\n", path); return 2; }
    std::vector<uint32_t> buf(1u << 16);
    unsigned long long n = 0;
    for (size_t got; (got = fread(buf.data(), 4, buf.size(), f)) > 0;)
        for (size_t k = 0; k < got; k++, n++)
            if (!check_bits(buf[k])) { fclose(f); return report(buf[k]); }
    fclose(f);
    printf("ok %llu\n", n);
    return 0;
}

static int run_all(int T)
{
    std::atomic<uint64_t> bad{~0ull};
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++)
        th.emplace_back([&, t] {
            const uint64_t lo = (1ull << 32) * (uint64_t)t / (uint64_t)T, hi = (1ull << 32) * (uint64_t)(t + 1) / (uint64_t)T;
            for (uint64_t b = lo; b < hi && bad.load(std::memory_order_relaxed) == ~0ull; b++)
                if (!check_bits((uint32_t)b)) bad = b;
        });
    for (std::thread &x : th) x.join();
    if (bad != ~0ull) return report((uint32_t)bad.load());
    printf("ok 4294967296\n");
    return 0;
}

static int run_u64()
{
    std::vector<uint64_t> v = {0, 1, 9, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 1, ~0ull, ~0ull - 1};
    uint64_t p = 1;
    for (int k = 0; k < 20; k++, p *= 10) { v.push_back(p - 1); v.push_back(p); v.push_back(p + 1); }
    for (uint64_t x : v) {
        char want[32];
        const int n = snprintf(want, sizeof want, "%llu", (unsigned long long)x);
        const uint32_t len = fmtg::u64_digits(x);
        std::vector<char> got(len); // (exactly len bytes)
        fmtg::u64_put(got.data(), x, len);
        if ((int)len != n || memcmp(want, got.data(), len)) { printf("mismatch at %llu\n", (unsigned long long)x); return 1; }
    }
    printf("ok %zu\n", v.size());
    return 0;
}

static int run_host()
{
    uint64_t seed = 0x9e3779b97f4a7c15ull;
    auto rnd = [&] { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    const uint32_t lens[] = {0, 1, 63, 64, 65, 129, 0, 4097};
    const uint64_t n = sizeof lens / sizeof lens[0];
    std::vector<uint64_t> off(n + 1, 0);
    for (uint64_t k = 0; k < n; k++) off[k + 1] = off[k] + lens[k];
    std::vector<uint8_t> step(off[n]);
    std::vector<float> d(off[n]);
    std::vector<rawdtw_aln_rec_t> recs(n);
    for (uint64_t k = 0; k < n; k++) {
        recs[k] = rawdtw_aln_rec_t{k == 3 ? (1ull << 32) - 30 : rnd() % 2000, k == 4 ? 995 : rnd() % (1ull << 33), (uint32_t)(k % 3) * 7u, (uint32_t)(k & 1), 0};
        for (uint32_t q = 0; q < lens[k]; q++) {
            step[off[k] + q] = q ? (uint8_t)(1 + rnd() % 3) : 0;
            const uint32_t bits = (uint32_t)rnd();
            memcpy(&d[off[k] + q], &bits, 4);
        }
    }
    std::string want;
    std::vector<uint64_t> want_off(n + 1, 0);
    for (uint64_t k = 0; k < n; k++) {
        unsigned long long pi = 0, pj = recs[k].j0;
        for (uint32_t q = 0; q < lens[k]; q++) {
            pi += step[off[k] + q] & 1u; pj += step[off[k] + q] >> 1;
            unsigned long long i = pi, j = pj;
            if (recs[k].mode) { i += recs[k].off_i; j += recs[k].off_j; }
            else if (q + 1 == lens[k]) { i += (unsigned long long)lens[k] * recs[k].off_i; j += (unsigned long long)lens[k] * recs[k].off_j; }
            char el[96];
            snprintf(el, sizeof el, "(%llu,%llu,%g)", i, j, (double)d[off[k] + q]);
            want += el;
        }
        want_off[k + 1] = want.size();
    }
    for (int threads = 1; threads <= 3; threads += 2) {
        std::vector<uint64_t> toff(n + 1, 77);
        uint64_t bytes = 0;
        if (rawdtw_aln_text_host(step.data(), d.data(), off.data(), lens, recs.data(), n, threads, toff.data(), nullptr, 0, &bytes) != RAWDTW_OK ||
            bytes != want.size() || toff != want_off) { printf("sizes differ\n"); return 1; }
        std::vector<char> text(bytes); // (exactly: a byte past it is the sanitizer's)
        if (rawdtw_aln_text_host(step.data(), d.data(), off.data(), lens, recs.data(), n, threads, toff.data(), text.data(), bytes, &bytes) != RAWDTW_OK ||
            memcmp(text.data(), want.data(), bytes)) { printf("text differs\n"); return 1; }
        std::vector<char> small(bytes - 1, 'x');
        if (rawdtw_aln_text_host(step.data(), d.data(), off.data(), lens, recs.data(), n, threads, toff.data(), small.data(), bytes - 1, &bytes) != RAWDTW_ERR_RANGE ||
            small != std::vector<char>(bytes - 1, 'x') || toff != want_off) { printf("short cap\n"); return 1; }
    }
    printf("ok %llu\n", (unsigned long long)n);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "values" && argc > 2) return run_values(argv[2]);
    if (mode == "all") return run_all(argc > 2 ? atoi(argv[2]) : 1);
    if (mode == "u64") return run_u64();
    if (mode == "host") return run_host();
    printf("usage: fmt_g values FILE | all THREADS | u64 | host\n");
    return 2;
}
