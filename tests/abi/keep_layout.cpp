// The store of kept chains (rawalign_amd/csrc/rawdtw_keep_layout.h) as a plain C++ program: the header needs no HIP.
// n_slots in {1, 3} x N in {1, 64, 65}:
//   every half's count is a 4-byte word on a 4-byte boundary inside the counts region; every half's seeds start on a 64-byte boundary
//   (12-byte records of 4-byte words: aligned), hold N * 12 bytes and lie inside the block; no two halves' seeds overlap, no two counts
//   overlap, no count overlaps any seeds; address(slot, half) = slot * 2 + half runs over 0 .. 2 * n_slots - 1 once; the total is the
//   counts region rounded up to 256 plus 2 * n_slots strides, restated here.
// Prints "ok <cases>"; the first failure otherwise.
#include "layout_check.h"
#include "rawdtw_keep_layout.h"

using namespace rawdtw::keep;

int main()
{
    unsigned long long cases = 0;
    for (uint64_t n_slots : {1ull, 3ull})
        for (uint64_t N : {1ull, 64ull, 65ull}) {
            const Layout L = layout(n_slots, N);
            cases++;
            if (L.halves() != 2 * n_slots) { printf("FAIL halves\n"); return 1; }
            std::vector<Named> rs;
            std::vector<bool> seen(2 * n_slots, false);
            for (uint32_t s = 0; s < n_slots; s++)
                for (uint32_t h = 0; h < 2; h++) {
                    const uint32_t a = Layout::address(s, h);
                    if (a != s * 2 + h || a >= L.halves() || seen[a]) { printf("FAIL address(%u, %u) = %u\n", s, h, a); return 1; }
                    seen[a] = true;
                    rs.push_back(Named{"count", rawdtw::ws::Region{L.count_at(a), 4}, 4, true});
                    if (L.count_at(a) + 4 > L.counts_bytes) { printf("FAIL a count leaves the counts region\n"); return 1; }
                }
            if (!regions_ok("counts", rs, L.need, 4)) return 1;
            const size_t n_counts = rs.size();
            for (uint32_t a = 0; a < 2 * n_slots; a++) rs.push_back(Named{"seeds", rawdtw::ws::Region{L.seeds_at(a), (size_t)N * kSeedBytes}, (size_t)N * kSeedBytes, true});
            for (size_t i = n_counts; i < rs.size(); i++)
                if (rs[i].r.at % 64 || rs[i].r.at < L.counts_bytes) { printf("FAIL a half's seeds are not aligned, or inside the counts\n"); return 1; }
            std::vector<Named> all(rs.begin() + (long)n_counts, rs.end()); // (disjoint from each other and from the counts: regions_ok compares every pair)
            all.insert(all.end(), rs.begin(), rs.begin() + (long)n_counts);
            if (!regions_ok("store", all, L.need, 4)) return 1;
            const size_t stride = ((size_t)N * 12 + 63) / 64 * 64, need = al256(n_slots * 2 * 4) + n_slots * 2 * stride;
            if (L.stride != stride || L.need != need) { printf("FAIL need %zu (stride %zu), restated %zu (%zu)\n", L.need, L.stride, need, stride); return 1; }
        }
    printf("ok %llu\n", cases);
    return 0;
}
