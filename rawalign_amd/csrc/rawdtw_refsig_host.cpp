// rawdtw_refsig_host.cpp -- the reference from bases on the host: PoreModel::Load (src/pore_model.cpp:50-84) as main.cpp:349-351 uses
// it, ri_seq_to_sig (src/rsig.cpp:7-41) restated with the exact step of its two sums (rawdtw_refsig.h), and that step alone for
// tests.  The CPU path and the comparator of the device build (rawdtw_refsig.hip).  Pure host code, no device.
#include <fstream>
#include <new>
#include <sstream>
#include <string>
#include <vector>

#include "rawdtw_refsig.h"

#pragma clang fp contract(off)

namespace rawdtw {
namespace refsig {

void seq_to_sig(const uint8_t *bases, uint32_t len, const float *pore_vals, uint32_t k, int strand, int contracted, float *out, uint32_t *s_len,
                uint64_t fast[2], uint64_t slow[2])
{
    const uint32_t n = len >= k ? len - k + 1 : 0;
    *s_len = n;
    double sum = 0, sum2 = 0, x[kStep], x2[kStep];
    for (uint32_t j0 = 0; j0 < n; j0 += kStep) {
        const uint32_t c = n - j0 < kStep ? n - j0 : kStep;
        for (uint32_t t = 0; t < c; t++) {
            const float v = pore_vals[kmer_of(bases, len, k, strand, j0 + t)];
            out[j0 + t] = v;
            x[t] = (double)v;
            x2[t] = x[t] * x[t]; // (exact: 48 bits)
        }
        const bool f1 = sum_step(&sum, x, c), f2 = sum_step(&sum2, x2, c);
        if (fast) { fast[0] += f1; fast[1] += f2; }
        if (slow) { slow[0] += !f1; slow[1] += !f2; }
    }
    if (!n) return;
    double mean, std_dev;
    mean_std(sum, sum2, n, contracted, &mean, &std_dev);
    for (uint32_t j = 0; j < n; j++) out[j] = normalised(out[j], mean, std_dev);
}

} // namespace refsig
} // namespace rawdtw

using namespace rawdtw::refsig;

extern "C" {

int rawdtw_pore_model_load(const char *path, uint32_t *k, float *level_mean, uint64_t cap)
{
    if (!path || !k) return RAWDTW_ERR_INVALID;
    *k = 0;
    std::ifstream in(path);
    if (!in) return RAWDTW_ERR_INVALID;
    std::string line;
    uint32_t kk = 0;
    std::vector<std::pair<uint32_t, float>> rows;
    try {
        while (std::getline(in, line)) {
            if (line.empty() || line[0] == '#' || line.compare(0, 4, "kmer") == 0) continue;
            std::istringstream ls(line);
            std::string kmer;
            float level = 0.0f;
            ls >> kmer;
            if (kmer.empty()) continue; // (a blank line: the reference asserts on it; nothing is lost by passing over it)
            if (!kk) kk = (uint32_t)kmer.size();
            if (kmer.size() != kk || kk > kMaxK) return RAWDTW_ERR_INVALID;
            ls >> level;
            uint32_t slot = 0; // GenerateSeedFromSequence (pore_model.cpp:31-47): N -> A, lower case accepted
            for (char ch : kmer) {
                const uint32_t c = nt4((uint8_t)ch);
                slot = slot << 2 | (c < 4 ? c : 0u);
            }
            rows.emplace_back(slot, level);
        }
    } catch (const std::bad_alloc &) { return RAWDTW_ERR_OOM; }
    if (!kk) return RAWDTW_ERR_INVALID; // no k-mer at all
    *k = kk;
    const uint64_t slots = 1ull << (2 * kk);
    if (cap < slots || !level_mean) return RAWDTW_ERR_RANGE;
    for (uint64_t i = 0; i < slots; i++) level_mean[i] = 0.0f;
    for (const auto &r : rows) level_mean[r.first] = r.second; // (a k-mer named twice: the later row, as the reference overwrites)
    return RAWDTW_OK;
}

int rawdtw_seq_to_sig_host(const char *bases, uint32_t len, const float *pore_vals, uint32_t k, int strand, int contracted, float *out,
                           uint32_t *s_len)
{
    if (!s_len || !pore_vals || k < 1 || k > kMaxK || (len && !bases) || len >= (1u << 31)) return RAWDTW_ERR_INVALID;
    if (len >= k && !out) return RAWDTW_ERR_INVALID;
    seq_to_sig((const uint8_t *)bases, len, pore_vals, k, strand != 0, contracted != 0, out, s_len, nullptr, nullptr);
    return RAWDTW_OK;
}

int rawdtw_seq_sums_restated(const float *values, uint64_t n, double *sum, double *sum2, uint64_t fast[2], uint64_t slow[2])
{
    if ((n && !values) || !sum || !sum2) return RAWDTW_ERR_INVALID;
    double s = 0, s2 = 0, x[kStep], x2[kStep];
    uint64_t f[2] = {0, 0}, sl[2] = {0, 0};
    for (uint64_t j0 = 0; j0 < n; j0 += kStep) {
        const uint32_t c = (uint32_t)(n - j0 < kStep ? n - j0 : kStep);
        for (uint32_t t = 0; t < c; t++) { x[t] = (double)values[j0 + t]; x2[t] = x[t] * x[t]; }
        const bool f1 = sum_step(&s, x, c), f2 = sum_step(&s2, x2, c);
        f[0] += f1; f[1] += f2; sl[0] += !f1; sl[1] += !f2;
    }
    *sum = s; *sum2 = s2;
    if (fast) { fast[0] = f[0]; fast[1] = f[1]; }
    if (slow) { slow[0] = sl[0]; slow[1] = sl[1]; }
    return RAWDTW_OK;
}

} // extern "C"
