// rawdtw_su.cpp -- sequence-until (RI_M_SEQUENCEUNTIL) as a state of its own (include/rawdtw.h, rawdtw_su_*).
//
// What it restates: the accounting of map_worker_pipeline's step 1 (src/rmap.cpp:918-944) over the pipeline's su_* fields
// (rmap.h:74-77, initialised once at rmap.cpp:1018-1027), with find_outlier (sequence_until.c:4-18) through
// rawdtw_find_outlier / rawdtw_find_outlier_contracted.  A few hundred host operations every ttest_freq mapped reads: no
// kernel.  rawdtw_mapper.cpp feeds one from the mapper's closed mini-batches; rawalign_amd.mapper.CSequenceUntil is the
// Python face of it, and rawalign_amd.mapping.SequenceUntil the plain-Python restatement the tests compare it with.
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/rawdtw.h"

struct rawdtw_su {
    rawdtw_su_opt_t opt{};
    uint32_t n_seq = 0;
    std::vector<uint32_t> c_estimations;   // su_c_estimations (uint32_t: wraps)
    std::vector<float> estimations;        // su_estimations, tn_samples rows of n_seq
    std::vector<const float *> rows;       // (the row pointers find_outlier takes)
    uint32_t nreads = 0, nestimations = 0, ab_count = 0, cur = 0;
    uint32_t stop = 0;                     // su_stop of the call that fired (0: not yet)
};

extern "C" {

int rawdtw_su_create(uint32_t n_seq, const rawdtw_su_opt_t *opt, rawdtw_su **out)
{
    if (!out) return RAWDTW_ERR_INVALID;
    *out = nullptr;
    const rawdtw_su_opt_t o = opt ? *opt : rawdtw_su_opt_t{1.5f, 5u, 500u, 500u, 0}; // roptions.c:43-46
    if (n_seq == 0 || o.tn_samples == 0 || o.ttest_freq == 0) return RAWDTW_ERR_INVALID;
    rawdtw_su *su = new (std::nothrow) rawdtw_su;
    if (!su) return RAWDTW_ERR_OOM;
    try {
        su->c_estimations.assign(n_seq, 0u);
        su->estimations.assign((size_t)o.tn_samples * n_seq, 0.0f);
        su->rows.resize(o.tn_samples);
    } catch (const std::bad_alloc &) {
        delete su;
        return RAWDTW_ERR_OOM;
    }
    for (uint32_t i = 0; i < o.tn_samples; i++) su->rows[i] = su->estimations.data() + (size_t)i * n_seq;
    su->opt = o;
    su->n_seq = n_seq;
    *out = su;
    return RAWDTW_OK;
}

int rawdtw_su_feed(rawdtw_su *su, uint32_t n, const uint8_t *mapped, const uint32_t *ref_id, const uint32_t *fragment_length, uint32_t *stop)
{
    if (!su || !stop || (n && (!mapped || !ref_id || !fragment_length))) return RAWDTW_ERR_INVALID;
    if (su->stop) { *stop = su->stop; return RAWDTW_OK; } // rmap.cpp:918: `&& !p->su_stop`
    const rawdtw_su_opt_t &o = su->opt;
    for (uint32_t k = 0; k < n; k++) {
        if (!mapped[k] || ref_id[k] >= su->n_seq) continue;
        su->c_estimations[ref_id[k]] += fragment_length[k];
        su->ab_count += fragment_length[k];
        su->nreads++;
        if (su->nreads > o.tmin_reads && !(su->nreads % o.ttest_freq)) {
            float *row = su->estimations.data() + (size_t)su->cur * su->n_seq;
            for (uint32_t ce = 0; ce < su->n_seq; ce++) row[ce] = (float)su->c_estimations[ce] / su->ab_count; // (float / uint32 -> float)
            if (++su->cur >= o.tn_samples) su->cur = 0;
            if (su->nestimations++ >= o.tn_samples) {
                const float d = o.contracted ? rawdtw_find_outlier_contracted(su->rows.data(), su->n_seq, o.tn_samples)
                                             : rawdtw_find_outlier(su->rows.data(), su->n_seq, o.tn_samples);
                if (d <= o.t_threshold) { su->stop = k + 1; break; }
            }
        }
    }
    *stop = su->stop;
    return RAWDTW_OK;
}

int rawdtw_su_state(const rawdtw_su *su, uint32_t *n_reads, uint32_t *n_estimations, uint32_t *ab_count, uint32_t *c_estimations)
{
    if (!su) return RAWDTW_ERR_INVALID;
    if (n_reads) *n_reads = su->nreads;
    if (n_estimations) *n_estimations = su->nestimations;
    if (ab_count) *ab_count = su->ab_count;
    if (c_estimations)
        for (uint32_t s = 0; s < su->n_seq; s++) c_estimations[s] = su->c_estimations[s];
    return RAWDTW_OK;
}

int rawdtw_su_destroy(rawdtw_su *su)
{
    delete su;
    return RAWDTW_OK;
}

} // extern "C"
