// rawdtw_fmt_g.h -- the text of a path element, "(i,j,%g)" (include/rawdtw.h, "aln text"), for the host restatement
// (rawdtw_aln_text.cpp) and the kernels (rawdtw_aln_text.hip) alike: one definition, no libc, integer arithmetic only.
//   fmt_g     float -> the bytes of snprintf("%g", (double)x) under the C locale (= ostream << float, rmap.cpp:580-592): six significant
//             digits, round-half-even on the EXACT value, total over all 2^32 bit patterns.  The text (at most 12 bytes) comes back
//             packed in two 64-bit words: nothing here indexes a local array at run time, so a kernel keeps it in registers.
//   u64_*     uint64_t -> decimal, up to 20 digits, written back to front at a known length.
//   elem_*    where element q of a job lies (the two offset quirks of rmap.cpp:230-233, 286-289), how long its text is, and the text.
// tests/abi/fmt_g.cpp holds fmt_g against snprintf over lattices of values; DESIGN 4.2 "aln:s: text" has the whole-space run.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RAWDTW_FMT_HD __host__ __device__ inline
#else
#define RAWDTW_FMT_HD inline
#endif

namespace rawdtw {
namespace fmtg {

// up to 16 bytes of text: byte k is bits 8k.. of lo (k < 8) or 8(k - 8).. of hi
struct Text {
    uint64_t lo, hi;
    uint32_t len;
};

// the low n bytes (1 <= n <= 8) of v behind what t holds
RAWDTW_FMT_HD void append(Text &t, uint64_t v, uint32_t n)
{
    if (n < 8) v &= (1ull << (8 * n)) - 1;
    const uint32_t p = t.len;
    if (p < 8) {
        t.lo |= v << (8 * p);
        if (p && p + n > 8) t.hi |= v >> (8 * (8 - p));
    } else
        t.hi |= v << (8 * (p - 8));
    t.len = p + n;
}

RAWDTW_FMT_HD uint32_t u64_digits(uint64_t v)
{
    uint32_t n = 1;
    if (v >= 10000000000000000ull) { v /= 10000000000000000ull; n += 16; }
    if (v >= 100000000ull) { v /= 100000000ull; n += 8; }
    if (v >= 10000ull) { v /= 10000ull; n += 4; }
    if (v >= 100ull) { v /= 100ull; n += 2; }
    if (v >= 10ull) n += 1;
    return n;
}

// v's n = u64_digits(v) digits at dst[0 .. n)
RAWDTW_FMT_HD void u64_put(char *dst, uint64_t v, uint32_t n)
{
    for (uint32_t k = n; k-- > 0;) {
        const uint64_t q = v / 10;
        dst[k] = (char)('0' + (uint32_t)(v - q * 10));
        v = q;
    }
}

RAWDTW_FMT_HD uint64_t pow10_u64(uint32_t p) // p <= 19
{
    uint64_t r = 1, b = 10;
    for (uint32_t k = 0; k < 5; k++) { // (square and multiply: five steps, no table)
        if (p & (1u << k)) r *= b;
        b *= b;
    }
    return r;
}

// The six significant digits D (100000 .. 999999) and the decimal exponent X of a value given as T * 10^drop plus, when `sticky`,
// something below T's last digit; T has at least seven digits, so the digit that decides the rounding is in T.
RAWDTW_FMT_HD void round6(uint64_t T, int drop, bool sticky, uint32_t &D, int &X)
{
    const uint32_t nd = u64_digits(T);
    const uint64_t pw = pow10_u64(nd - 6);
    uint64_t d = T / pw;
    const uint64_t rem = T - d * pw, half = pw >> 1;
    if (rem > half || (rem == half && (sticky || (d & 1)))) d++;
    X = (int)nd - 1 + drop;
    if (d == 1000000) { d = 100000; X++; }
    D = (uint32_t)d;
}

#define RAWDTW_FMT_DIV1E9(limb)                                  \
    do {                                                         \
        const uint64_t t_ = (r << 32) | (limb);                  \
        const uint64_t q_ = t_ / 1000000000ull;                  \
        r = t_ - q_ * 1000000000ull;                             \
        (limb) = q_;                                             \
    } while (0)
#define RAWDTW_FMT_MUL1E9(limb)                                  \
    do {                                                         \
        const uint64_t t_ = (uint64_t)(limb) * 1000000000ull + c; \
        (limb) = (uint32_t)t_;                                   \
        c = t_ >> 32;                                            \
    } while (0)

RAWDTW_FMT_HD Text fmt_g(uint32_t bits)
{
    Text t{0, 0, 0};
    if (bits >> 31) append(t, '-', 1);
    const uint32_t E = (bits >> 23) & 255u, mant = bits & 0x7fffffu;
    if (E == 255) {
        append(t, mant ? ('n' | 'a' << 8 | 'n' << 16) : ('i' | 'n' << 8 | 'f' << 16), 3);
        return t;
    }
    if (E == 0 && mant == 0) {
        append(t, '0', 1);
        return t;
    }
    // |x| = M * 2^e exactly
    const uint32_t M = E ? (mant | 0x800000u) : mant;
    const int e = E ? (int)E - 150 : -149;
    uint64_t T;
    int drop = 0;
    bool sticky = false;
    if (e >= 0 && e <= 40) { // an integer below 2^64
        T = (uint64_t)M << e;
    } else if (e > 40) { // an integer below 2^128: nine digits at a time off its low end until the rest fits a word
        uint64_t a3, a2, a1, a0;
        {
            const uint64_t lo = e < 64 ? (uint64_t)M << e : 0, hi = e < 64 ? (uint64_t)M >> (64 - e) : (uint64_t)M << (e - 64);
            a3 = hi >> 32; a2 = hi & 0xffffffffu; a1 = lo >> 32; a0 = lo & 0xffffffffu;
        }
        for (int k = 0; k < 3; k++) // (2^128 / 10^27 < 2^64)
            if (a3 | a2) {
                uint64_t r = 0;
                RAWDTW_FMT_DIV1E9(a3); RAWDTW_FMT_DIV1E9(a2); RAWDTW_FMT_DIV1E9(a1); RAWDTW_FMT_DIV1E9(a0);
                sticky = sticky || r != 0;
                drop += 9;
            }
        T = a1 << 32 | a0; // (at least 2^64 / 10^9: eleven digits)
    } else if (e >= -40) { // 2^-17 <= |x| < 2^24: M * 10^12 fits a word and floor(|x| * 10^12) has at least seven digits
        const uint64_t p = (uint64_t)M * 1000000000000ull;
        const uint32_t k = (uint32_t)-e;
        T = p >> k;
        sticky = (p & ((1ull << k) - 1)) != 0;
        drop = -12;
    } else { // below 2^-17, denormals included: a fixed-point fraction of 160 bits, nine digits at a time off its high end
        const uint32_t sh = (uint32_t)(160 + e); // M's lowest bit: 11 .. 119
        const uint32_t w = sh >> 5;
        const uint64_t v = (uint64_t)M << (sh & 31u);
        const uint32_t vl = (uint32_t)v, vh = (uint32_t)(v >> 32);
        uint32_t f0 = w == 0 ? vl : 0u, f1 = w == 1 ? vl : w == 0 ? vh : 0u, f2 = w == 2 ? vl : w == 1 ? vh : 0u,
                 f3 = w == 3 ? vl : w == 2 ? vh : 0u, f4 = w == 3 ? vh : 0u;
        T = 0;
        bool done = false;
        for (int k = 0; k < 6; k++) // (2^-149 > 10^-45: the fifth group of nine holds a digit at the latest)
            if (!done) {
                uint64_t c = 0;
                RAWDTW_FMT_MUL1E9(f0); RAWDTW_FMT_MUL1E9(f1); RAWDTW_FMT_MUL1E9(f2); RAWDTW_FMT_MUL1E9(f3); RAWDTW_FMT_MUL1E9(f4);
                drop -= 9;
                if (T) { T = T * 1000000000ull + c; done = true; } // the first group with a digit and the one behind it: ten digits or more
                else T = c;
            }
        sticky = (f0 | f1 | f2 | f3 | f4) != 0;
    }
    uint32_t D;
    int X;
    round6(T, drop, sticky, D, X);
    // D's digits as text, first digit in the low byte, and how many are left once the trailing zeros are gone
    const uint32_t d0 = D / 100000u, r0 = D - d0 * 100000u, d1 = r0 / 10000u, r1 = r0 - d1 * 10000u, d2 = r1 / 1000u, r2 = r1 - d2 * 1000u,
                   d3 = r2 / 100u, r3 = r2 - d3 * 100u, d4 = r3 / 10u, d5 = r3 - d4 * 10u;
    const uint64_t dg = 0x303030303030ull + ((uint64_t)d0 | (uint64_t)d1 << 8 | (uint64_t)d2 << 16 | (uint64_t)d3 << 24 | (uint64_t)d4 << 32 | (uint64_t)d5 << 40);
    const uint32_t P = d5 ? 6u : d4 ? 5u : d3 ? 4u : d2 ? 3u : d1 ? 2u : 1u;
    if (X < -4 || X >= 6) { // d[.ddddd]e+XX
        append(t, dg, 1);
        if (P > 1) { append(t, '.', 1); append(t, dg >> 8, P - 1); }
        const uint32_t ax = (uint32_t)(X < 0 ? -X : X); // (at most 45: two digits)
        append(t, 'e' | (uint32_t)(X < 0 ? '-' : '+') << 8 | ('0' + ax / 10u) << 16 | ('0' + ax % 10u) << 24, 4);
    } else if (X >= 0) { // the first X + 1 digits, a point and the rest if there is a rest
        const uint32_t il = (uint32_t)X + 1;
        append(t, dg, il);
        if (P > il) { append(t, '.', 1); append(t, dg >> (8 * il), P - il); }
    } else { // 0.[000]d...
        append(t, 0x303030302e30ull, 1u + (uint32_t)-X);
        append(t, dg, P);
    }
    return t;
}
#undef RAWDTW_FMT_DIV1E9
#undef RAWDTW_FMT_MUL1E9

RAWDTW_FMT_HD void text_put(char *dst, const Text &t)
{
    for (uint32_t k = 0; k < t.len; k++) dst[k] = (char)((k < 8 ? t.lo >> (8 * k) : t.hi >> (8 * (k - 8))) & 255u);
}

// ---- the elements of a path (include/rawdtw.h, rawdtw_aln_rec_t) ----
// element q of a job of `len` elements whose walk stands at (pi, pj): mode 1 moves every element by the offsets, mode 0 only the last
// one, by len times the offsets (64-bit arithmetic that wraps, as the unsigned long long of the host writer does)
RAWDTW_FMT_HD void elem_ij(uint64_t off_i, uint64_t off_j, uint32_t mode, uint64_t pi, uint64_t pj, uint32_t q, uint32_t len, uint64_t &i, uint64_t &j)
{
    i = pi; j = pj;
    if (mode) { i += off_i; j += off_j; }
    else if (q + 1 == len) { i += (uint64_t)len * off_i; j += (uint64_t)len * off_j; }
}

RAWDTW_FMT_HD uint32_t elem_len(uint64_t i, uint64_t j, const Text &g)
{
    return 4u + u64_digits(i) + u64_digits(j) + g.len;
}

// "(i,j,g)" at dst; returns its length (at most 1 + 20 + 1 + 20 + 1 + 12 + 1 = 56)
RAWDTW_FMT_HD uint32_t elem_put(char *dst, uint64_t i, uint64_t j, const Text &g)
{
    const uint32_t ni = u64_digits(i), nj = u64_digits(j);
    dst[0] = '(';
    u64_put(dst + 1, i, ni);
    dst[1 + ni] = ',';
    u64_put(dst + 2 + ni, j, nj);
    dst[2 + ni + nj] = ',';
    text_put(dst + 3 + ni + nj, g);
    dst[3 + ni + nj + g.len] = ')';
    return 4u + ni + nj + g.len;
}

} // namespace fmtg
} // namespace rawdtw
