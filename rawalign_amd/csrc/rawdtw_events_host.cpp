// rawdtw_events_host.cpp -- detect_events (src/revent.c:190-210) restated on the host, one chunk or many on std::threads: the
// CPU baseline of event detection and the comparator of the device path (rawdtw_events.hip).  Pure host code, no device.
// rawdtw_detect_raw_host takes windows of int16 DAC samples instead: each is converted and filtered (rawdtw_rawsig.cpp) and then
// goes the same way.
//
// Every line below keeps the reference's order and types (include/rawdtw.h lists what the bits depend on); the library is
// built with -ffp-contract=off, so the plain form has one rounding per operation, and the contracted form names its
// fused operations with std::fmaf / std::fma where GCC -O3 -march=native fuses them in revent.c on an FMA host.
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "../../include/rawdtw.h"
#include "rawdtw_events.h"

namespace {

// comp_prefix_prefixsq (revent.c:22-32)
void prefix_sums(const float *x, uint32_t n, float *ps, float *pss, bool fused)
{
    ps[0] = 0.0f;
    pss[0] = 0.0f;
    for (uint32_t i = 0; i < n; ++i) {
        ps[i + 1] = ps[i] + x[i];
        pss[i + 1] = fused ? std::fmaf(x[i], x[i], pss[i]) : pss[i] + x[i] * x[i];
    }
}

// comp_tstat (revent.c:34-75): t has s_len + 1 entries
void tstat(const float *ps, const float *pss, uint32_t n, uint32_t w, bool fused, float *t)
{
    std::memset(t, 0, ((size_t)n + 1) * sizeof(float));
    if (n < 2 * w || w < 2) return;
    const float wf = (float)w;
    for (uint32_t i = w; i <= n - w; ++i) {
        float s1 = ps[i], q1 = pss[i];
        if (i > w) {
            s1 -= ps[i - w];
            q1 -= pss[i - w];
        }
        const float s2 = ps[i + w] - ps[i], q2 = pss[i + w] - pss[i];
        const float m1 = s1 / wf, m2 = s2 / wf;
        float cv = fused ? std::fmaf(-m2, m2, std::fmaf(-m1, m1, q1 / wf) + q2 / wf) : q1 / wf - m1 * m1 + q2 / wf - m2 * m2;
        cv = std::fmax(cv, FLT_MIN);
        t[i] = (float)(std::fabs((double)(m2 - m1)) / std::sqrt((double)(cv / wf)));
    }
}

struct Detector {
    const float *sig;
    float threshold;
    uint32_t window_length, masked_to;
    int peak_pos;
    float peak_value;
    int valid_peak;
};

// gen_peaks (revent.c:77-138)
uint32_t gen_peaks(Detector &sd, Detector &ld, float peak_height, uint32_t n, uint32_t *peaks)
{
    uint32_t cur = 0;
    Detector *det[2] = {&sd, &ld};
    for (uint32_t i = 0; i < n; i++) {
        for (int k = 0; k < 2; k++) {
            Detector &d = *det[k];
            if (d.masked_to >= i) continue;
            const float v = d.sig[i];
            if (d.peak_pos == -1) {
                if (v < d.peak_value) d.peak_value = v;
                else if (v - d.peak_value > peak_height) { d.peak_value = v; d.peak_pos = (int)i; }
            } else {
                if (v > d.peak_value) { d.peak_value = v; d.peak_pos = (int)i; }
                if (k == 0 && d.peak_value > d.threshold) {
                    ld.masked_to = (uint32_t)d.peak_pos + d.window_length;
                    ld.peak_pos = -1;
                    ld.peak_value = FLT_MAX;
                    ld.valid_peak = 0;
                }
                if (d.peak_value - v > peak_height && d.peak_value > d.threshold) d.valid_peak = 1;
                if (d.valid_peak && (i - (uint32_t)d.peak_pos) > d.window_length / 2) {
                    peaks[cur++] = (uint32_t)d.peak_pos;
                    d.peak_pos = -1;
                    d.peak_value = v;
                    d.valid_peak = 0;
                }
            }
        }
    }
    return cur;
}

// gen_events (revent.c:140-188); returns n_ev
uint32_t gen_events(const uint32_t *peaks, uint32_t n_peaks, const float *ps, uint32_t n, bool fused, float *ev)
{
    uint32_t n_ev = 1;
    for (uint32_t i = 1; i < n_peaks; ++i)
        if (peaks[i] > 0 && peaks[i] < n) n_ev++;
    double sum = 0, sum2 = 0;
    float l_ps = 0, l_peak = 0;
    for (uint32_t pi = 0; pi + 1 < n_ev; pi++) {
        const float e = (ps[peaks[pi]] - l_ps) / ((float)peaks[pi] - l_peak);
        ev[pi] = e;
        const float e2 = e * e; // (the float product, widened)
        sum += e;
        sum2 += e2;
        l_ps = ps[peaks[pi]];
        l_peak = (float)peaks[pi];
    }
    const float e = (ps[n] - l_ps) / ((float)n - l_peak);
    ev[n_ev - 1] = e;
    const float e2 = e * e;
    sum += e;
    sum2 += e2;
    const double mean = sum / n_ev;
    const double std_dev = std::sqrt(fused ? std::fma(-mean, mean, sum2 / n_ev) : sum2 / n_ev - mean * mean);
    for (uint32_t i = 0; i < n_ev; ++i) ev[i] = (float)(((double)ev[i] - mean) / std_dev);
    return n_ev;
}

// scratch of one chunk, reused across a thread's chunks
struct Scratch {
    std::vector<float> ps, pss, t1, t2, pa; // (pa: the raw entry's converted window)
    std::vector<uint32_t> peaks;
    void fit(uint32_t n)
    {
        if (ps.size() < (size_t)n + 1) {
            ps.resize((size_t)n + 1); pss.resize((size_t)n + 1); t1.resize((size_t)n + 1); t2.resize((size_t)n + 1);
            peaks.resize(n);
        }
    }
};

uint32_t detect_one(const rawdtw_event_opt_t &o, uint32_t n, const float *sig, float *ev, Scratch &s)
{
    s.fit(n);
    const bool fused = o.contracted != 0;
    prefix_sums(sig, n, s.ps.data(), s.pss.data(), fused);
    tstat(s.ps.data(), s.pss.data(), n, o.window_length1, fused, s.t1.data());
    tstat(s.ps.data(), s.pss.data(), n, o.window_length2, fused, s.t2.data());
    Detector sd{s.t1.data(), o.threshold1, o.window_length1, 0, -1, FLT_MAX, 0};
    Detector ld{s.t2.data(), o.threshold2, o.window_length2, 0, -1, FLT_MAX, 0};
    const uint32_t n_peaks = gen_peaks(sd, ld, o.peak_height, n, s.peaks.data());
    return n_peaks ? gen_events(s.peaks.data(), n_peaks, s.ps.data(), n, fused, ev) : 0; // revent.c:206
}

// many chunks on `threads` threads: one(k, ev, scratch) writes chunk k's events at ev and returns how many.  Each chunk's events
// land in a staging array at the chunk's own offset (never more events than samples), then move to their place once every
// count is known.
template <class One>
int detect_many(uint32_t n_chunks, const uint64_t *off, uint64_t *event_off, float *events, uint64_t events_cap, int threads, One one)
{
    std::vector<float> stage;
    std::vector<uint32_t> count;
    try {
        stage.resize(off[n_chunks] - off[0]);
        count.resize(n_chunks);
    } catch (const std::bad_alloc &) {
        return RAWDTW_ERR_OOM;
    }
    const int T = std::max(1, std::min(threads, 256));
    std::atomic<uint32_t> next{0};
    std::atomic<int> oom{0};
    auto work = [&]() {
        try {
            Scratch s;
            for (uint32_t k; (k = next.fetch_add(1)) < n_chunks;) count[k] = one(k, stage.data() + (off[k] - off[0]), s);
        } catch (const std::bad_alloc &) {
            oom = 1;
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back(work);
    work();
    for (auto &x : th) x.join();
    if (oom) return RAWDTW_ERR_OOM;
    uint64_t tot = 0;
    for (uint32_t k = 0; k < n_chunks; k++) { event_off[k] = tot; tot += count[k]; }
    event_off[n_chunks] = tot;
    if (tot > events_cap) return RAWDTW_ERR_RANGE;
    for (uint32_t k = 0; k < n_chunks; k++)
        if (count[k]) std::memcpy(events + event_off[k], stage.data() + (off[k] - off[0]), (size_t)count[k] * sizeof(float));
    return RAWDTW_OK;
}

} // namespace

namespace rawdtw {
namespace events {

int resolve_opt(const rawdtw_event_opt_t *opt, rawdtw_event_opt_t *out)
{
    *out = opt ? *opt : rawdtw_event_opt_t{3u, 6u, 4.30265f, 2.57058f, 1.0f, 0}; // roptions.c:37-41
    return out->window_length1 > kMaxWindow || out->window_length2 > kMaxWindow ? RAWDTW_ERR_INVALID : RAWDTW_OK;
}

int check_offsets(uint32_t n_chunks, const uint64_t *sig_off)
{
    for (uint32_t k = 0; k < n_chunks; k++)
        if (sig_off[k + 1] <= sig_off[k] || sig_off[k + 1] - sig_off[k] > 0xffffffffull) return RAWDTW_ERR_INVALID;
    return RAWDTW_OK;
}

} // namespace events
} // namespace rawdtw

extern "C" {

int rawdtw_detect_events(const rawdtw_event_opt_t *opt, uint32_t s_len, const float *sig, float *events, uint32_t *n)
{
    rawdtw_event_opt_t o;
    if (!n || !sig || !events || s_len == 0 || rawdtw::events::resolve_opt(opt, &o) != RAWDTW_OK) return RAWDTW_ERR_INVALID;
    try {
        Scratch s;
        *n = detect_one(o, s_len, sig, events, s);
    } catch (const std::bad_alloc &) {
        return RAWDTW_ERR_OOM;
    }
    return RAWDTW_OK;
}

int rawdtw_detect_events_host(const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *sig_off, const float *sig,
                              uint64_t *event_off, float *events, uint64_t events_cap, int threads)
{
    rawdtw_event_opt_t o;
    if (!sig_off || !event_off || (n_chunks && (!sig || !events))) return RAWDTW_ERR_INVALID;
    if (rawdtw::events::resolve_opt(opt, &o) != RAWDTW_OK || rawdtw::events::check_offsets(n_chunks, sig_off) != RAWDTW_OK)
        return RAWDTW_ERR_INVALID;
    return detect_many(n_chunks, sig_off, event_off, events, events_cap, threads, [&](uint32_t k, float *ev, Scratch &s) {
        return detect_one(o, (uint32_t)(sig_off[k + 1] - sig_off[k]), sig + sig_off[k], ev, s);
    });
}

int rawdtw_detect_raw_host(const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *raw_off, const int16_t *raw,
                           const rawdtw_channel_t *chan, uint32_t *s_len, uint64_t *event_off, float *events, uint64_t events_cap,
                           int threads)
{
    rawdtw_event_opt_t o;
    if (!raw_off || !event_off || (n_chunks && (!raw || !chan || !s_len || !events))) return RAWDTW_ERR_INVALID;
    if (rawdtw::events::resolve_opt(opt, &o) != RAWDTW_OK || rawdtw::events::check_raw_offsets(n_chunks, raw_off) != RAWDTW_OK)
        return RAWDTW_ERR_INVALID;
    return detect_many(n_chunks, raw_off, event_off, events, events_cap, threads, [&](uint32_t k, float *ev, Scratch &s) {
        const uint64_t n = raw_off[k + 1] - raw_off[k];
        if (s.pa.size() < n) s.pa.resize(n);
        const uint32_t l = (uint32_t)rawdtw::events::to_pa(chan[k], n, raw + raw_off[k], s.pa.data()); // rsig.cpp:216-224
        s_len[k] = l;
        return l ? detect_one(o, l, s.pa.data(), ev, s) : 0u; // nothing kept: no events
    });
}

} // extern "C"
