// What the layout programs (seed_layout.cpp, events_layout.cpp) check alike: a block's regions are aligned, inside the block, pairwise
// disjoint, at least what their kernels index, and empty where the kind does not use them.
#pragma once
#include <cstdio>
#include <vector>

#include "rawdtw_layout.h"

struct Named { const char *name; rawdtw::ws::Region r; size_t least; bool used; };

inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }

inline bool regions_ok(const char *block, const std::vector<Named> &rs, size_t total, size_t align)
{
    for (size_t i = 0; i < rs.size(); i++) {
        const Named &a = rs[i];
        if (!a.used && a.r.bytes) { printf("FAIL %s: %s is not used but has %zu bytes\n", block, a.name, a.r.bytes); return false; }
        if (a.used && a.r.bytes < a.least) { printf("FAIL %s: %s has %zu bytes, needs %zu\n", block, a.name, a.r.bytes, a.least); return false; }
        if (a.r.at % align) { printf("FAIL %s: %s at %zu is not aligned to %zu\n", block, a.name, a.r.at, align); return false; }
        if (!a.r.bytes) continue;
        if (a.r.at > total || a.r.bytes > total - a.r.at) { printf("FAIL %s: %s [%zu, +%zu) leaves the block of %zu\n", block, a.name, a.r.at, a.r.bytes, total); return false; }
        for (size_t j = 0; j < i; j++) {
            const Named &b = rs[j];
            if (b.r.bytes && a.r.at < b.r.at + b.r.bytes && b.r.at < a.r.at + a.r.bytes) { printf("FAIL %s: %s and %s overlap\n", block, a.name, b.name); return false; }
        }
    }
    return true;
}
