// rawdtw_layout.h -- what the layouts of the begin / end workspaces (rawdtw_seed_layout.h, rawdtw_events_layout.h) are made of: a region
// of a block as byte offsets, the device block's 256-byte rounding, and the walk that hands regions out one behind the other.  No HIP
// include: a plain compiler takes it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rawdtw {
namespace ws {

struct Region { size_t at = 0, bytes = 0; };

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// the next `bytes` bytes of a block; an empty region's `at` is where the next one starts
struct Take {
    size_t p = 0;
    Region operator()(size_t bytes) { const Region r{p, bytes}; p += bytes; return r; }
};

} // namespace ws
} // namespace rawdtw
