// The device-planned batch's workspace layout (rawalign_amd/csrc/rawdtw_stream_layout.h) as a plain C++ program: the header needs no
// HIP.  Every kind (plain, compact, chunk round) over na in {1, 511, 512, 513, 8191, 8192, 8193, 100 000} (the tile's, the scan unit's
// and the compact stride's edges) x nc in {1, 2, 255, 257, na} (nc <= na) x nr in {1, nc} x pass_pool in {-1, 0, 3}; a compact batch also
// over n_wide in {0, 5}, a chunk round over n_full in {na, 2 na + 7}:
//   device block  every region starts on a 256-byte boundary and lies inside `need`; no two non-empty regions overlap; a region the
//                 kind does not use is empty; a region is at least what its kernels index -- taken from rawdtw_runs.hip and the fold:
//                 a pass entry (16 bytes) a slot, kStreamRecStride records (8 bytes) a tile, 2 kStreamMaxSeg copy orders (16 bytes) a
//                 slot, three statistics words a scan unit of 8 192 anchors, a cost an anchor, the steps in whole units ...; `need` is
//                 the sum batch_create_stream used to write out, restated here
//   results       cnt at 0, score and keep behind it with only padding between, res_bytes = keep.at + nc: one copy brings all three home
//   pinned block  cnt, score, keep at the device block's offsets, pin_need the sum as it was
//   counts        n_tiles, n_slots, others_cap, n_units equal their formulas
// Then rawdtw_events_append's staging (append_layout) over n_new x n_segments the same way.  Prints "ok <cases>"; the first failure otherwise.
#include <algorithm>

#include "layout_check.h"
#include "rawdtw_stream_layout.h"

using namespace rawdtw::stream;

static bool batch_case(Kind kind, uint64_t nr, uint64_t nc, uint64_t na, uint64_t n_full, uint64_t n_wide, int pass_pool)
{
    const bool compact = kind == Kind::compact, round = kind == Kind::round;
    const Layout L = layout({nr, nc, na, n_full, kind, n_wide, pass_pool});
    // the derived counts
    const uint64_t n_tiles = (na + 511) / 512, n_slots = pass_pool >= 0 ? n_tiles + (uint64_t)pass_pool : 4 * n_tiles + 64;
    const uint64_t others_cap = std::min<uint64_t>(na, na / 4 + 4096), n_units = (na + 8191) / 8192;
    if (L.n_tiles != n_tiles || L.n_slots != n_slots || L.others_cap != others_cap || L.n_units != n_units) { printf("FAIL a derived count\n"); return false; }
    const std::vector<Named> dev = {
        {"cnt", L.cnt, 192 * 8, true},                        {"score", L.score, nc * 4, true},               {"keep", L.keep, nc, true},
        {"anchor_off", L.anchor_off, (nc + 1) * 8, true},     {"anchors", L.anchors, na * 8, true},           {"ref_base", L.ref_base, nc * 8, true},
        {"read_base", L.read_base, nc * 4, true},             {"chain_off", L.chain_off, (nr + 1) * 8, true}, {"tlist", L.tlist, n_tiles * 8, true},
        {"todo", L.todo, n_slots * 16, true},                 {"recs", L.recs, n_tiles * 576 * 8, true},      {"runtab", L.runtab, n_slots * 2 * 32 * 16, true},
        {"tile_stats", L.tile_stats, n_units * 3 * 8, true},  {"omix", L.omix, others_cap * 32, true},        {"ojobs", L.ojobs, others_cap * 32, true},
        {"ocls", L.ocls, others_cap, true},                   {"chains", L.chains, nc * 24, true},            {"fold_order", L.fold_order, nc * 4, true},
        {"full", L.full, nc * 4, true},                       {"gate", L.gate, nc * 4, true},                 {"out", L.out, na * 4, true},
        {"heads", L.heads, nc * 8, compact},                  {"unit_abs", L.unit_abs, n_units * 8, compact}, {"steps", L.steps, n_units * 8192 * 2, compact},
        {"wide", L.wide, n_wide * 12, compact},               {"carry", L.carry, nc * 24, round},             {"full_off", L.full_off, (nc + 1) * 8, round},
        {"out_full", L.out_full, n_full * 4, round}};
    if (!regions_ok("device", dev, L.need, 256)) return false;
    for (size_t i = 1; i < dev.size(); i++) // the order the offsets were handed out in: each region right behind the one before
        if (dev[i].r.at != dev[i - 1].r.at + dev[i - 1].r.bytes) { printf("FAIL device: %s does not follow %s\n", dev[i].name, dev[i - 1].name); return false; }
    // batch_create_stream's own sums, as they stood
    auto al = al256;
    const size_t compact_bytes = compact ? al(nc * 8) + al(n_units * 8) + al(n_units * 8192 * 2) + al(n_wide * 12) : 0;
    const size_t round_bytes = round ? al(nc * 24) + al((nc + 1) * 8) + al(n_full * 4) : 0;
    const size_t need = compact_bytes + round_bytes + al(192 * 8) + al((nc + 1) * 8) + al(na * 8) + al(nc * 8) + al(nc * 4) + al((nr + 1) * 8) +
                        al(n_tiles * 8) + al(n_slots * 16) + al(n_tiles * 24) + al(n_tiles * 576 * 8) + al(n_slots * 2 * 32 * 16) +
                        2 * al(others_cap * 32) + al(others_cap) + al(nc * 24) + 4 * al(nc * 4) + al(nc) + al(na * 4);
    const size_t pin_need = al(192 * 8) + al(nc * 4) + al(nc);
    if (L.need != need) { printf("FAIL need %zu, the sum was %zu\n", L.need, need); return false; }
    if (L.pin_need != pin_need) { printf("FAIL pin_need %zu, the sum was %zu\n", L.pin_need, pin_need); return false; }
    // the results: one copy from cnt brings the counters, the scores and the keep flags home
    if (L.cnt.at != 0 || L.score.at != al(192 * 8) || L.keep.at != L.score.at + al(nc * 4) || L.res_bytes != L.keep.at + nc || L.res_bytes > L.pin_need) {
        printf("FAIL the results do not lie one behind the other from 0\n");
        return false;
    }
    const std::vector<Named> pin = {{"p_cnt", L.p_cnt, 192 * 8, true}, {"p_score", L.p_score, nc * 4, true}, {"p_keep", L.p_keep, nc, true}};
    if (!regions_ok("pinned", pin, L.pin_need, 256)) return false;
    if (L.p_cnt.at != L.cnt.at || L.p_score.at != L.score.at || L.p_keep.at != L.keep.at) { printf("FAIL a pinned region is not at its device region's offset\n"); return false; }
    return true;
}

static bool append_case(uint64_t n_new, uint32_t n_segments)
{
    const AppendLayout L = append_layout(n_new, n_segments);
    const std::vector<Named> dev = {{"ev", L.ev, n_new * 4, true}, {"src", L.src, ((size_t)n_segments + 1) * 8, true}, {"dst", L.dst, (size_t)n_segments * 4, true}};
    if (!regions_ok("append", dev, L.need, 256)) return false;
    const size_t need = al256(n_new * 4) + al256(((size_t)n_segments + 1) * 8) + al256((size_t)n_segments * 4); // rawdtw_events_append's sum, as it stood
    if (L.need != need || L.ev.at != 0 || L.src.at != al256(n_new * 4)) { printf("FAIL append: need %zu, the sum was %zu\n", L.need, need); return false; }
    return true;
}

int main()
{
    unsigned long long cases = 0;
    for (Kind kind : {Kind::plain, Kind::compact, Kind::round})
        for (uint64_t na : {1ull, 511ull, 512ull, 513ull, 8191ull, 8192ull, 8193ull, 100000ull}) {
            std::vector<uint64_t> ncs;
            for (uint64_t nc : {1ull, 2ull, 255ull, 257ull, (unsigned long long)na})
                if (nc <= na && std::find(ncs.begin(), ncs.end(), nc) == ncs.end()) ncs.push_back(nc);
            for (uint64_t nc : ncs)
                for (uint64_t nr : nc == 1 ? std::vector<uint64_t>{1} : std::vector<uint64_t>{1, nc})
                    for (int pass_pool : {-1, 0, 3})
                        for (uint64_t n_wide : kind == Kind::compact ? std::vector<uint64_t>{0, 5} : std::vector<uint64_t>{0})
                            for (uint64_t n_full : kind == Kind::round ? std::vector<uint64_t>{na, 2 * na + 7} : std::vector<uint64_t>{na}) {
                                if (!batch_case(kind, nr, nc, na, n_full, n_wide, pass_pool)) {
                                    printf("  at kind %d nr %llu nc %llu na %llu n_full %llu n_wide %llu pass_pool %d\n", (int)kind, (unsigned long long)nr,
                                           (unsigned long long)nc, (unsigned long long)na, (unsigned long long)n_full, (unsigned long long)n_wide, pass_pool);
                                    return 1;
                                }
                                cases++;
                            }
        }
    for (uint64_t n_new : {0ull, 1ull, 63ull, 64ull, 65ull, 100000ull})
        for (uint32_t n_segments : {1u, 31u, 32u, 33u, 1000u}) {
            if (!append_case(n_new, n_segments)) { printf("  at n_new %llu n_segments %u\n", (unsigned long long)n_new, n_segments); return 1; }
            cases++;
        }
    printf("ok %llu\n", cases);
    return 0;
}
