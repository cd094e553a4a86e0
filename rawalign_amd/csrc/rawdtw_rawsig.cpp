// rawdtw_rawsig.cpp -- the int16 DAC samples of a signal file to pA and the outlier filter of ri_read_sig
// (src/rsig.cpp:216-224) restated on the host, and the one pass that finds where map_worker_for's chunks (rmap.cpp:685-690)
// begin in raw positions.  Pure host code, no device; the device path is k_raw_count / k_raw_compact in rawdtw_events.hip.
//
// The bits: scale = range / digitisation, pA = ((float)raw + offset) * scale, kept iff pA > 30 && pA < 200 -- one fp32
// division, one add, one multiply, two ordered compares.  The library is built with -ffp-contract=off -fno-fast-math, and an
// add followed by a multiply has nothing to contract, so there is one form.
#include <algorithm>
#include <cstdint>

#include "../../include/rawdtw.h"
#include "rawdtw_events.h"

namespace {

inline float pa_of(int16_t r, float offset, float scale) { return ((float)r + offset) * scale; }
inline bool kept(float pa) { return pa > 30.0f && pa < 200.0f; }

// the kept samples of raw[0 .. n): a loop without writes or branches, which the compiler vectorises
inline uint32_t count_kept(const int16_t *raw, uint32_t n, float offset, float scale)
{
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; i++) c += kept(pa_of(raw[i], offset, scale)) ? 1u : 0u;
    return c;
}

} // namespace

namespace rawdtw {
namespace events {

uint64_t to_pa(const rawdtw_channel_t &ch, uint64_t n, const int16_t *raw, float *pa)
{
    const float scale = ch.range / ch.digitisation, offset = ch.offset;
    uint64_t l = 0;
    if (!pa) {
        for (uint64_t i = 0; i < n; i += 1u << 20) l += count_kept(raw + i, (uint32_t)std::min<uint64_t>(1u << 20, n - i), offset, scale);
        return l;
    }
    for (uint64_t i = 0; i < n; i++) {
        const float x = pa_of(raw[i], offset, scale);
        if (kept(x)) pa[l++] = x; // (only the first l_sig slots are written)
    }
    return l;
}

int check_raw_offsets(uint32_t n_chunks, const uint64_t *raw_off)
{
    for (uint32_t k = 0; k < n_chunks; k++)
        if (raw_off[k + 1] < raw_off[k] || raw_off[k + 1] - raw_off[k] > 0xffffffffull) return RAWDTW_ERR_INVALID;
    return RAWDTW_OK;
}

} // namespace events
} // namespace rawdtw

extern "C" {

int rawdtw_signal_to_pa(const rawdtw_channel_t *ch, uint64_t n_raw, const int16_t *raw, float *pa, uint64_t *l_sig)
{
    if (!ch || !l_sig || (n_raw && !raw)) return RAWDTW_ERR_INVALID;
    *l_sig = rawdtw::events::to_pa(*ch, n_raw, raw, pa);
    return RAWDTW_OK;
}

int rawdtw_signal_chunk_table(const rawdtw_channel_t *ch, uint64_t n_raw, const int16_t *raw, uint32_t chunk_size,
                              uint32_t max_num_chunk, uint64_t *l_sig, uint32_t *n_chunks, uint64_t *raw_start)
{
    if (!ch || !l_sig || !n_chunks || !raw_start || (n_raw && !raw) || chunk_size == 0) return RAWDTW_ERR_INVALID;
    const float scale = ch->range / ch->digitisation, offset = ch->offset;
    const uint64_t cap = (uint64_t)chunk_size * max_num_chunk; // kept samples that land in a chunk
    // Blocks of kBlock samples are counted without a branch; only a block that holds a chunk's first kept sample, or the last
    // kept sample below `cap`, is walked sample by sample.
    constexpr uint32_t kBlock = 512;
    uint64_t l = 0, end = 0;
    raw_start[0] = 0;
    for (uint64_t i0 = 0; i0 < n_raw; i0 += kBlock) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(kBlock, n_raw - i0);
        const uint32_t c = count_kept(raw + i0, nb, offset, scale);
        if (c && l < cap) {
            // kept samples number l .. l + c - 1 are here: a multiple of chunk_size among them, or number cap - 1?
            const uint64_t next_start = (l + chunk_size - 1) / chunk_size * chunk_size;
            if (next_start < std::min(l + c, cap) || l + c >= cap) {
                uint64_t q = l;
                for (uint32_t i = 0; i < nb && q < cap; i++)
                    if (kept(pa_of(raw[i0 + i], offset, scale))) {
                        if (q % chunk_size == 0) raw_start[q / chunk_size] = i0 + i;
                        if (q == cap - 1) end = i0 + i + 1;
                        q++;
                    }
            }
        }
        l += c;
    }
    const uint32_t nc = (uint32_t)std::min<uint64_t>(max_num_chunk, (l + chunk_size - 1) / chunk_size);
    if (l < cap) // the last chunk ends at the read's last kept sample
        for (end = n_raw; end > 0 && !kept(pa_of(raw[end - 1], offset, scale)); end--) {}
    if (nc) raw_start[nc] = end;
    *l_sig = l;
    *n_chunks = nc;
    return RAWDTW_OK;
}

} // extern "C"
