// rawdtw_seed_min.h -- one step of ri_sketch_min's window (src/rsketch.c:193-219) as a function of the hashes alone: what the seed table's
// device build (rawdtw_seed_build.hip, k_sb_min_count / k_sb_min_write) and its host restatement (rawdtw_seed_sketch_windowed,
// rawdtw_seed_host.cpp) share, as sum_step is shared for the reference sums.  No HIP include: a plain compiler takes it.
//
// The reference walks a strand's e-mers m = 0 .. M-1 with a carried minimum (`min`, `min_pos`).  That state is a function of the window:
//   S(m) = (the smallest hash among e-mers max(0, m-w+1) .. m, the NEWEST index that carries it)
// because both the `<=` of rsketch.c:201 and the `>=` of :206 prefer the later of two equal hashes.  With prev = S(m-1) (none for m = 0)
// step m emits, in this order:
//   1. m + 1 == w and prev exists: every i in 0 .. m-1 with h[i] == prev.h and i != prev.i, oldest first        (rsketch.c:194-198)
//   2. prev is none or h[m] <= prev.h: prev, when m >= w and prev exists                                        (rsketch.c:201-203)
//   3. else, m - prev.i == w (the minimum left the window): prev, then every i in m-w+1 .. m with h[i] == S(m).h and i != S(m).i,
//      oldest first                                                                                               (rsketch.c:204-214)
//   4. else nothing
//   5. m + 1 == M: S(m)                                                                                           (rsketch.c:220)
// So a step reads h[m-w .. m] and nothing that another step wrote.  An element is named by its e-mer's index; the caller turns it into
// (hash, position of the e-mer's first kept event).
#pragma once
#include <cstdint>

#ifndef RAWDTW_HD
#if defined(__HIPCC__)
#define RAWDTW_HD __host__ __device__
#else
#define RAWDTW_HD
#endif
#endif

namespace rawdtw {
namespace seed {

// M: the e-mers of a strand with `kept` kept events
RAWDTW_HD inline uint32_t strand_emers(uint32_t kept, uint32_t e)
{
    return kept >= e ? kept - e + 1 : 0;
}

// The hashes come as a pointer and the index of the e-mer that h[0] belongs to: h[i - base] is e-mer i's hash, for every i a step reads
// (max(0, m-w) .. m).  A kernel's staged tile and a whole strand's array are both that.
struct MinHashes {
    const uint32_t *h;
    uint32_t base;
    RAWDTW_HD uint32_t operator[](uint32_t i) const { return h[i - base]; }
};

// S(m)'s index: the newest e-mer among max(0, m-w+1) .. m with the smallest hash
RAWDTW_HD inline uint32_t min_window(const MinHashes &h, uint32_t m, uint32_t w)
{
    uint32_t best = m + 1 >= w ? m + 1 - w : 0;
    uint32_t hb = h[best];
    for (uint32_t i = best + 1; i <= m; i++) {
        const uint32_t x = h[i];
        if (x <= hb) { hb = x; best = i; }
    }
    return best;
}

// Step m of a strand of M e-mers under windows of w (1 .. 255): emit(i) for every element in order, i its e-mer's index.  Returns their number.
template <typename F> RAWDTW_HD inline uint32_t min_step_walk(const MinHashes &h, uint32_t m, uint32_t M, uint32_t w, F emit)
{
    uint32_t n = 0, now = m; // now: S(m)'s index
    if (m > 0) {
        const uint32_t pi = min_window(h, m - 1, w), ph = h[pi], hm = h[m];
        if (m + 1 == w)
            for (uint32_t i = 0; i < m; i++)
                if (h[i] == ph && i != pi) { emit(i); n++; }
        if (hm <= ph) {
            if (m >= w) { emit(pi); n++; }
        } else if (m - pi == w) {
            emit(pi); n++;
            now = min_window(h, m, w);
            const uint32_t hn = h[now];
            for (uint32_t i = m + 1 - w; i <= m; i++)
                if (h[i] == hn && i != now) { emit(i); n++; }
        } else now = pi;
    }
    if (m + 1 == M) { emit(now); n++; }
    return n;
}

// the two calls of a count-then-write pass: how many elements step m emits, and those elements' e-mer indices in order (out has room
// for min_step_count's answer)
RAWDTW_HD inline uint32_t min_step_count(const uint32_t *h, uint32_t base, uint32_t m, uint32_t M, uint32_t w)
{
    return min_step_walk(MinHashes{h, base}, m, M, w, [](uint32_t) {});
}

RAWDTW_HD inline uint32_t min_step_emit(const uint32_t *h, uint32_t base, uint32_t m, uint32_t M, uint32_t w, uint32_t *out)
{
    uint32_t k = 0;
    return min_step_walk(MinHashes{h, base}, m, M, w, [&](uint32_t i) { out[k++] = i; });
}

} // namespace seed
} // namespace rawdtw
