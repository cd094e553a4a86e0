// rawdtw_refsig.h -- what the host restatement (rawdtw_refsig_host.cpp) and the device build (rawdtw_refsig.hip) of ri_seq_to_sig
// (src/rsig.cpp:7-41) share: the base code, the k-mer of an output element, the exact step of the two double sums, the two scalars
// behind them, and where the build's arrays lie in its device block.  Internal: nothing here is part of the ABI.
//
// An output element j of a strand depends on k bases only: emission j is traversal step i = j + k - 1, its k-mer the codes of steps
// j .. j + k - 1 (the `& mask` drops everything older), step t reading base t (strand 0) or len - 1 - t with 3 ^ c (strand 1).  An
// ambiguous base shifts 00 in on either strand (rsig.cpp:24).
//
// The sums are sequential double additions by definition.  A step takes up to 64 addends.  With the running sum s = q * u in the
// binade [2^p, 2^(p+1)), u = 2^(p-52), an addend x = a * u + f (a = floor(x / u), 0 <= f < u) moves the exact sum to (q + a) * u + f,
// which rounds to (q + a) * u for f < u/2 and to (q + a + 1) * u for f > u/2 as long as the result stays inside the binade, where
// the spacing is u.  So while no f is a tie and q + D < 2^53 for D = sum of (a + [f > u/2]), the 64 roundings are one integer sum
// (addends are not negative, so every partial sum stays below the last).  Anything else -- a negative or non-finite addend, one too
// large, a tie, a binade crossing, s zero, negative, non-finite or too small for u/2 to be normal -- and the step is 64 dependent
// additions in emission order.  Correctness never rests on the fast path.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "rawdtw_layout.h"
#include "rawdtw_seed.h" // RAWDTW_HD

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rawdtw {
namespace refsig {

constexpr uint32_t kMaxK = 12;           // 4^12 floats: a 64 MiB model
constexpr uint32_t kStep = 64;           // addends a step: a wave
constexpr uint32_t kModelLdsMaxK = 6;    // 4^k * 4 bytes in LDS up to here (16 KiB), global memory above
constexpr uint32_t kStepsAhead = 8;      // steps whose levels a wave loads before it advances the sums through them

// seq_nt4_table (rutils.c:5-16): ACGT and acgt are 0..3, every other byte is 4
RAWDTW_HD inline uint32_t nt4(uint8_t b)
{
    switch (b) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

// the model slot of output element j of a strand (j < len - k + 1)
RAWDTW_HD inline uint32_t kmer_of(const uint8_t *bases, uint32_t len, uint32_t k, int strand, uint32_t j)
{
    uint32_t kmer = 0;
    for (uint32_t t = j; t < j + k; t++) {
        const uint32_t c = nt4(bases[strand ? len - 1 - t : t]);
        kmer = kmer << 2 | (c < 4 ? (strand ? 3u ^ c : c) : 0u);
    }
    return kmer; // (k <= 12: 24 bits, nothing to mask)
}

RAWDTW_HD inline uint64_t bits_of(double x)
{
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}
RAWDTW_HD inline double double_of(uint64_t b)
{
    double x;
    memcpy(&x, &b, 8);
    return x;
}

// may a step starting from s take the fast path at all?
RAWDTW_HD inline bool sum_fast_ready(uint64_t s_bits)
{
    const uint64_t E = s_bits >> 52; // (sign included: a negative s fails the range test)
    return E >= 64 && E < 0x7ff;
}

// one addend against the running sum: false where the step must walk slowly, else *d = a + [f > u/2] in units of u
RAWDTW_HD inline bool sum_addend_units(uint64_t s_bits, double x, uint64_t *d)
{
    const uint64_t xb = bits_of(x), E = s_bits >> 52;
    uint64_t Ex = xb >> 52, mx = xb & ((1ull << 52) - 1);
    *d = 0;
    if (Ex >= 0x7ff) return false; // negative (sign bit in Ex), infinite or NaN
    if (Ex == 0) {                 // zero or subnormal: below u/2 whatever s is (E >= 64)
        return true;
    }
    mx |= 1ull << 52;
    if (Ex > E) return false; // x >= 2^(p+1)
    const uint64_t sh = E - Ex;
    if (sh > 53) return true; // x < u/2
    if (sh == 0) { *d = mx; return true; }
    const uint64_t rem = mx & ((1ull << sh) - 1), half = 1ull << (sh - 1);
    if (rem == half) return false; // a tie: round-to-even needs q's parity at that addend
    *d = (mx >> sh) + (rem > half ? 1 : 0);
    return true;
}

// the sum behind a fast step, or false where it would leave the binade (D: the step's units, at most 64 * 2^53)
RAWDTW_HD inline bool sum_fast_finish(uint64_t s_bits, uint64_t D, uint64_t *out_bits)
{
    const uint64_t q = (s_bits & ((1ull << 52) - 1)) | 1ull << 52;
    if (q + D >= 1ull << 53) return false;
    *out_bits = (s_bits & ~((1ull << 52) - 1)) | ((q + D) & ((1ull << 52) - 1));
    return true;
}

// one step as the host takes it: n <= kStep addends in order; true where it went fast.  The device takes the same three
// functions above with a lane an addend (rawdtw_refsig.hip, wave_step).
inline bool sum_step(double *s, const double *x, uint32_t n)
{
    const uint64_t sb = bits_of(*s);
    bool ok = sum_fast_ready(sb);
    uint64_t D = 0, d, nb;
    for (uint32_t t = 0; ok && t < n; t++) {
        ok = sum_addend_units(sb, x[t], &d);
        D += d;
    }
    if (ok && sum_fast_finish(sb, D, &nb)) { *s = double_of(nb); return true; }
    double a = *s;
    for (uint32_t t = 0; t < n; t++) a += x[t];
    *s = a;
    return false;
}

// rsig.cpp:34-35 behind the sums, plain (one rounding an operation) or as an FMA build contracts it
RAWDTW_HD inline void mean_std(double sum, double sum2, uint32_t j, int contracted, double *mean, double *std_dev)
{
    const double n = (double)j; // (the reference divides by the int j)
    const double m = sum / n, q = sum2 / n;
    // (the library is built with -ffp-contract=off and the pragma above says it again: the plain form is two roundings.  f64 `/` and
    // sqrt lower to correctly rounded sequences on gfx950, as rawdtw_events.hip relies on too)
#if defined(__HIP_DEVICE_COMPILE__)
    *std_dev = sqrt(contracted ? __fma_rn(-m, m, q) : q - m * m);
#else
    *std_dev = std::sqrt(contracted ? std::fma(-m, m, q) : q - m * m);
#endif
    *mean = m;
}

RAWDTW_HD inline float normalised(float level, double mean, double std_dev)
{
    return (float)(((double)level - mean) / std_dev); // rsig.cpp:38
}

// ---- the build's device block (rawdtw_refsig.hip), byte offsets from (n_seq, total bases, 4^k) ----
//   bases   every sequence's bytes as they crossed, one behind the other          total bases
//   table   per sequence: base offset u64, arena offsets fwd / rev u64, len, s_len  n_seq * 32
//   sums    per (sequence, strand): sum, sum2 (double bits), mean, std_dev         2 n_seq * 32
//   steps   per (sequence, strand): fast and slow steps of sum, of sum2            2 n_seq * 32
//   model   the levels                                                             4^k * 4
struct SeqRow {
    uint64_t base_off, arena_fwd, arena_rev;
    uint32_t len, s_len;
};
static_assert(sizeof(SeqRow) == 32, "a row is 32 bytes");
struct StrandSums { double sum, sum2, mean, std_dev; };
struct StrandSteps { uint64_t fast[2], slow[2]; };

struct Layout {
    ws::Region bases, table, sums, steps, model;
    size_t need = 0;
};

inline Layout layout(uint64_t n_seq, uint64_t total_bases, uint64_t model_floats)
{
    Layout L;
    ws::Take take;
    L.bases = take(ws::al(total_bases + 16)); // (never empty: a build of empty sequences still has a block)
    L.table = take(ws::al(n_seq * sizeof(SeqRow)));
    L.sums = take(ws::al(2 * n_seq * sizeof(StrandSums)));
    L.steps = take(ws::al(2 * n_seq * sizeof(StrandSteps)));
    L.model = take(ws::al(model_floats * 4));
    L.need = take.p;
    return L;
}

// ri_seq_to_sig on the host: out has room for len - k + 1 floats; the steps of both sums are counted where asked
void seq_to_sig(const uint8_t *bases, uint32_t len, const float *pore_vals, uint32_t k, int strand, int contracted, float *out, uint32_t *s_len,
                uint64_t fast[2], uint64_t slow[2]);

} // namespace refsig
} // namespace rawdtw
