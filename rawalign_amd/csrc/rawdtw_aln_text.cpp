// rawdtw_aln_text.cpp -- the aln text's definition (include/rawdtw.h, "aln text") restated on host threads with the shared formatter
// (rawdtw_fmt_g.h), and the bound on a batch's text.  No HIP and no snprintf: a plain compiler takes this unit (tests/abi/fmt_g.cpp
// is built with it under AddressSanitizer).  The kernels: rawdtw_aln_text.hip.
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/rawdtw.h"
#include "rawdtw_fmt_g.h"

using namespace rawdtw;

namespace {

// job k's text at dst (null: measured only); returns its length
uint64_t job_text(const uint8_t *step, const float *d, uint32_t len, const rawdtw_aln_rec_t &rc, char *dst)
{
    uint64_t pi = 0, pj = rc.j0, bytes = 0;
    for (uint32_t q = 0; q < len; q++) {
        pi += step[q] & 1u; pj += (step[q] >> 1) & 1u;
        uint64_t i, j;
        fmtg::elem_ij(rc.off_i, rc.off_j, rc.mode, pi, pj, q, len, i, j);
        uint32_t bits;
        memcpy(&bits, d + q, 4);
        const fmtg::Text g = fmtg::fmt_g(bits);
        bytes += dst ? fmtg::elem_put(dst + bytes, i, j, g) : fmtg::elem_len(i, j, g);
    }
    return bytes;
}

template <typename F> void on_threads(int T, F fn)
{
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back([&fn, t] { fn(t); });
    fn(0);
    for (std::thread &x : th) x.join();
}

uint32_t digits_of_sum(uint64_t a, uint64_t b) // of a + b, 20 where the sum wraps
{
    const uint64_t s = a + b;
    return s < a ? 20u : fmtg::u64_digits(s);
}

} // namespace

extern "C" {

int rawdtw_aln_text_host(const uint8_t *path_step, const float *path_d, const uint64_t *path_off, const uint32_t *path_len,
                         const rawdtw_aln_rec_t *recs, uint64_t n_jobs, int threads, uint64_t *text_off, char *text, uint64_t text_cap,
                         uint64_t *text_bytes)
{
    if (!text_off || !text_bytes || (n_jobs && (!path_step || !path_d || !path_off || !path_len || !recs))) return RAWDTW_ERR_INVALID;
    for (uint64_t k = 0; k < n_jobs; k++)
        if (recs[k].mode > 1) return RAWDTW_ERR_INVALID;
    uint64_t elems = 0;
    for (uint64_t k = 0; k < n_jobs; k++) elems += path_len[k];
    int T = threads > 0 ? threads : (int)std::max(1u, std::thread::hardware_concurrency());
    T = (int)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)T, 16, elems / 4096 + 1, std::max<uint64_t>(n_jobs, 1)}));
    // measure, scan, write: as the device does it
    on_threads(T, [&](int t) {
        for (uint64_t k = n_jobs * (uint64_t)t / T; k < n_jobs * (uint64_t)(t + 1) / T; k++)
            text_off[k + 1] = job_text(path_step + path_off[k], path_d + path_off[k], path_len[k], recs[k], nullptr);
    });
    text_off[0] = 0;
    for (uint64_t k = 0; k < n_jobs; k++) text_off[k + 1] += text_off[k];
    *text_bytes = text_off[n_jobs];
    if (!text) return RAWDTW_OK;
    if (text_cap < *text_bytes) return RAWDTW_ERR_RANGE;
    on_threads(T, [&](int t) {
        for (uint64_t k = n_jobs * (uint64_t)t / T; k < n_jobs * (uint64_t)(t + 1) / T; k++)
            (void)job_text(path_step + path_off[k], path_d + path_off[k], path_len[k], recs[k], text + text_off[k]);
    });
    return RAWDTW_OK;
}

// A walk of at most n + m - 1 elements stands at most n + m - 2 steps from where it began, in either coordinate, whatever its step
// bytes are: that, not the shape of a valid path, is what the bound assumes.
uint64_t rawdtw_aln_text_bound(const rawdtw_job_t *jobs, const rawdtw_aln_rec_t *recs, uint64_t n_jobs)
{
    if (!jobs || !recs) return 0;
    uint64_t total = 0;
    for (uint64_t k = 0; k < n_jobs; k++) {
        const uint64_t elems = (uint64_t)jobs[k].n + jobs[k].m - 1;
        if (jobs[k].n == 0 || jobs[k].m == 0) continue;
        const uint64_t far = elems - 1;
        if (recs[k].mode) total += elems * (16u + digits_of_sum(far, recs[k].off_i) + digits_of_sum(far + recs[k].j0, recs[k].off_j));
        else // (the last element's products wrap: any 64-bit value)
            total += elems * (16u + fmtg::u64_digits(far) + fmtg::u64_digits(far + recs[k].j0)) + 40u;
    }
    return total;
}

} // extern "C"
