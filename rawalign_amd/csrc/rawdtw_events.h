// rawdtw_events.h -- what the host restatement (rawdtw_events_host.cpp) and the device path (rawdtw_events.hip) of event
// detection share.  Internal: nothing here is part of the ABI.
#pragma once
#include <cstdint>

#include "../../include/rawdtw.h"

namespace rawdtw {
namespace events {

// our own bound on the windows: near 2^31 the reference's 2 * w_len wraps and its loop runs off the array (revent.c:46,50)
constexpr uint32_t kMaxWindow = 65535;

// the options, NULL = roptions.c:37-41 with contracted 0; RAWDTW_ERR_INVALID for a window above kMaxWindow
int resolve_opt(const rawdtw_event_opt_t *opt, rawdtw_event_opt_t *out);
// RAWDTW_ERR_INVALID unless every chunk is non-empty (revent.c:24 asserts) and shorter than 2^32
int check_offsets(uint32_t n_chunks, const uint64_t *sig_off);
// the raw entries' rule: an empty window is allowed (a read whose tail is all outliers has one)
int check_raw_offsets(uint32_t n_chunks, const uint64_t *raw_off);

// rsig.cpp:216-224 (rawdtw_rawsig.cpp): the kept pA samples of raw[0 .. n) into pa (n slots, or null: count only); returns how many
uint64_t to_pa(const rawdtw_channel_t &ch, uint64_t n, const int16_t *raw, float *pa);

} // namespace events
} // namespace rawdtw
