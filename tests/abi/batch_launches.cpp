// A batch's launch table (rawalign_amd/csrc/rawdtw_launches.h) as a plain C++ program: the header needs no HIP.  The device-planned
// form, and every job-list launch list made of up to one launch each of kKindBandLane, kKindBandWreg with param -16, -8, 0 and 4,
// kKindBandWave, kKindFullWave and kKindBandLaneHi (2^8 lists), each in two orders, each under the 16 combinations of "merge_small",
// "tile_threads" (256 / 512), side streams (0 / 2) and "serial_launches":
//   length       the DTW launches plus 2, fold and select last
//   merged       the tile launch is reported as kKindBandMerged, and the register-wave launches of param -16, -8 and 0 as carried, exactly
//                when: merge_small, 256 tile threads, no side streams unless the launches are serial, a tile launch, and one of the three
//                -- the condition as merge_of stated it, restated here
//   once         every plan launch is one entry, its own or a carried one, in plan order, under its own kind and parameter otherwise
//   event slots  the pairs of distinct (run, launch) never overlap and stay below runs * 2 * nl
//   launch word  the merged entry's is kKindBandMerged | param << 8 (the device-planned form's entry 1: the image's floats as param)
// and the table of wave classes: five classes of 1, 2, 4, 8, 8 rows a lane on 1, 1, 1, 1, kFullWgWaves waves, reported as
// 1, 2, 4, 8, 264; class -> parameter -> class round-trips, and a parameter that no class reports is rejected.
// Prints "ok <cases>"; the first failure otherwise.
#include <cstdio>
#include <vector>

#include "rawdtw_launches.h"

using namespace rawdtw;

#define CHECK(cond, what)                                                       \
    do {                                                                        \
        if (!(cond)) { printf("FAIL %s: %s\n", what, #cond); return false; }    \
    } while (0)

static bool tail_ok(const std::vector<BatchLaunch> &t, size_t n_dtw, const char *what)
{
    CHECK(t.size() == n_dtw + 2, what);
    const BatchLaunch &f = t[n_dtw], &s = t[n_dtw + 1];
    CHECK(f.kind == kKindChainFold && s.kind == kKindReadSelect && f.plan == -1 && s.plan == -1 && !f.carried && !s.carried, what);
    CHECK(f.word() == 6u && s.word() == 7u, what);
    return true;
}

static bool slots_ok(uint32_t nl, const char *what)
{
    const uint32_t runs = 3;
    std::vector<char> used((size_t)runs * 2 * nl, 0);
    for (uint32_t r = 0; r < runs; r++)
        for (uint32_t i = 0; i < nl; i++) {
            const size_t s = event_slot(r, i, nl);
            CHECK(s + 1 < used.size() && !used[s] && !used[s + 1], what);
            used[s] = used[s + 1] = 1;
        }
    CHECK(event_slot(0, 0, nl) == 0 && event_slot(1, 0, nl) == 2 * (size_t)nl, what); // (a run's pairs lie one behind the other: run_all_launches takes ev[2 * i])
    return true;
}

static bool stream_case(uint32_t lds)
{
    const std::vector<BatchLaunch> t = batch_launches(lds, nullptr, MergeSel{});
    if (!tail_ok(t, 2, "stream") || !slots_ok((uint32_t)t.size(), "stream")) return false;
    CHECK(t[0].kind == kKindBandWreg && t[0].param == 0 && t[0].word() == 8u, "stream");
    CHECK(t[1].kind == kKindBandMerged && t[1].word() == (10u | lds << 8), "stream");
    CHECK(t[0].plan == -1 && t[1].plan == -1 && !t[0].carried && !t[1].carried, "stream");
    return true;
}

static bool joblist_case(const std::vector<Launch> &ls, bool merge_small, int tile_threads, int n_side, bool serial)
{
    const char *what = "job list";
    const MergeSel mg = merge_select(merge_small, tile_threads, n_side, serial, ls);
    const std::vector<BatchLaunch> t = batch_launches(0, &ls, mg);
    if (!tail_ok(t, ls.size(), what) || !slots_ok((uint32_t)t.size(), what)) return false;
    auto small = [](const Launch &L) { return L.kind == kKindBandWreg && (L.param == -16 || L.param == -8 || L.param == 0); };
    bool has_tile = false, has_small = false;
    for (const Launch &L : ls) { has_tile |= L.kind == kKindBandLane; has_small |= small(L); }
    const bool merged = merge_small && tile_threads == 256 && !(n_side > 0 && !serial) && has_tile && has_small;
    CHECK(mg.on() == merged, what);
    for (size_t i = 0; i < ls.size(); i++) {
        const Launch &L = ls[i];
        const BatchLaunch &E = t[i];
        CHECK(E.plan == (int)i && E.param == L.param, what); // every plan launch once, in plan order
        CHECK(E.carried == (merged && small(L)), what);
        if (merged && L.kind == kKindBandLane) CHECK(E.kind == kKindBandMerged && E.word() == (10u | (uint32_t)L.param << 8), what);
        else CHECK(E.kind == L.kind && E.word() == (L.kind | (uint32_t)L.param << 8), what);
    }
    return true;
}

static bool wave_class_case()
{
    const char *what = "wave classes";
    const int rows[5] = {1, 2, 4, 8, 8}, waves[5] = {1, 1, 1, 1, kFullWgWaves}, params[5] = {1, 2, 4, 8, 264};
    CHECK(kWaveClasses == 5 && kFullWgWaves == 4, what);
    for (int c = 0; c < kWaveClasses; c++) {
        CHECK(kWaveClass[c].rows == rows[c] && kWaveClass[c].waves == waves[c], what);
        CHECK(wave_class_param(c) == params[c] && wave_class_of(wave_class_param(c)) == c, what);
        CHECK(launch_word(kKindSemiWave, wave_class_param(c)) == (11u | (uint32_t)params[c] << 8), what);
    }
    for (int32_t p = -300; p <= 600; p++) {
        bool known = false;
        for (int c = 0; c < 5; c++) known |= p == params[c];
        if (!known) CHECK(wave_class_of(p) == -1, what);
    }
    return true;
}

int main()
{
    unsigned long cases = 0;
    if (!stream_case(5800)) return 1;
    cases++;
    if (!wave_class_case()) return 1; // (not counted: "ok <cases>" counts launch tables)
    const Launch pool[8] = {{kKindBandLane, 6144, 0, 900}, {kKindBandWreg, -16, 900, 70}, {kKindBandWreg, -8, 970, 50},   {kKindBandWreg, 0, 1020, 40},
                            {kKindBandWreg, 4, 1060, 30},  {kKindBandWave, 9000, 1090, 5}, {kKindFullWave, 2, 1095, 3},   {kKindBandLaneHi, 14336, 1098, 20}};
    for (unsigned set = 0; set < 256; set++)
        for (int reversed = 0; reversed < 2; reversed++) {
            std::vector<Launch> ls;
            for (int k = 0; k < 8; k++) {
                const int q = reversed ? 7 - k : k;
                if (set >> q & 1) ls.push_back(pool[q]);
            }
            for (unsigned s = 0; s < 16; s++) {
                if (!joblist_case(ls, s & 1, s & 2 ? 256 : 512, s & 4 ? 2 : 0, (s & 8) != 0)) {
                    printf("  launches 0x%02x%s, settings %u\n", set, reversed ? " reversed" : "", s);
                    return 1;
                }
                cases++;
            }
        }
    printf("ok %lu\n", cases);
    return 0;
}
