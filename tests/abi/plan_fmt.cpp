// The packed records of a device-planned batch (rawalign_amd/csrc/rawdtw_plan_fmt.h) and their host reader
// (rawdtw_plan_check.cpp) as a plain C++ program: neither needs HIP.
//   round trip  every format packed and read back field by field: each field over its whole range with the other fields at
//               every combination of their extremes (the copy order's 64-bit source offset: every single bit, set and
//               cleared, and its low 20 bits swept under four high words); sort_bin against the order it stands for --
//               radius 3 before 2 before 1, longer side first, sides >= 63 alike.
//   checker     a hand-built plan of one tile -- two parts of radius 2 (one with the reference window the longer), two of
//               radius 1 (one exclude_last), one of radius 3, one on the side list; one pass, one run per arena -- is
//               accepted with the statistics the jobs add up to; twelve single corruptions of it are each rejected.
// Prints "ok <round-trip cases> <plans checked>"; the first failure otherwise.
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "rawdtw_plan_check.h"

using namespace rawdtw;

static unsigned long long g_cases = 0;

// every field f over [0, max[f]], the others at every combination of 0 and their maximum
static bool sweep(const std::vector<uint32_t> &max, const std::function<bool(const std::vector<uint32_t> &)> &check)
{
    const size_t nf = max.size();
    std::vector<uint32_t> v(nf);
    for (size_t f = 0; f < nf; f++)
        for (uint32_t ext = 0; ext < (1u << nf); ext++) {
            if ((ext >> f) & 1u) continue; // (the swept field has no extreme of its own)
            for (size_t o = 0; o < nf; o++) v[o] = (ext >> o) & 1u ? max[o] : 0u;
            for (uint64_t x = 0; x <= max[f]; x++) {
                v[f] = (uint32_t)x;
                g_cases++;
                if (!check(v)) {
                    printf("FAIL round trip: field %zu of %zu, values", f, nf);
                    for (uint32_t q : v) printf(" %u", q);
                    printf("\n");
                    return false;
                }
            }
        }
    return true;
}

static bool round_trips()
{
    // job record
    if (!sweep({127, 127, 3, 1, kStreamTile - 1}, [](const std::vector<uint32_t> &v) {
            const uint32_t shape = rec_shape(v[0], v[1], v[2], v[3]), y = rec_with_item(shape, v[4]);
            // (k_plan hands rec_with_item its item word: the bits above the shape do not reach the record)
            const uint32_t word = shape | 1u << kItemSwapped | 1u << kItemRunStart | 1u << kItemRunEnd | 1u << kItemTile;
            return rec_n(y) == v[0] && rec_m(y) == v[1] && rec_radius(y) == v[2] && rec_excl(y) == v[3] && rec_item(y) == v[4] &&
                   rec_with_item(word, v[4]) == y && rec_n(word) == v[0] && rec_m(word) == v[1] && rec_radius(word) == v[2] && (shape & ~kRecShapeMask) == 0;
        })) return false;
    if (!sweep({0xffff, 0xffff}, [](const std::vector<uint32_t> &v) {
            const uint32_t x = rec_windows(v[0], v[1]);
            return rec_long(x) == v[0] && rec_short(x) == v[1];
        })) return false;
    // pass entry
    if (!sweep({0xffff, 63, 1023}, [](const std::vector<uint32_t> &v) {
            const uint32_t z = pass_counts(v[0], v[1], v[2]);
            return pass_jobs(z) == v[0] && pass_runs(z) == v[1] && pass_n_hi(z) == v[2];
        })) return false;
    if (!sweep({0xffff, 0xffff}, [](const std::vector<uint32_t> &v) {
            const uint32_t w = pass_place(v[0], v[1]);
            return pass_region(w) == v[0] && pass_rec0(w) == v[1];
        })) return false;
    // copy order: the source offset
    auto src_ok = [](long long src) { g_cases++; return order_src(order_src_lo(src), order_src_hi(src)) == src; };
    for (int b = 0; b < 64; b++) {
        const unsigned long long bit = 1ull << b;
        if (!src_ok((long long)bit) || !src_ok((long long)~bit) || !src_ok(-(long long)(bit >> 1)) || !src_ok((long long)(bit - 1))) { printf("FAIL copy order source, bit %d\n", b); return false; }
    }
    for (unsigned long long hi : {0ull, 0x7fffffffull, 0x80000000ull, 0xffffffffull})
        for (unsigned long long lo = 0; lo < (1ull << 20); lo++) {
            const long long src = (long long)(hi << 32 | lo << 12 | lo >> 8);
            if (!src_ok(src) || order_src_lo(src) != (uint32_t)(lo << 12 | lo >> 8) || order_src_hi(src) != (uint32_t)hi) { printf("FAIL copy order source %lld\n", src); return false; }
        }
    // the lanes' order
    if (sort_bin(1, 127) != kSortBinRadius1 || sort_bin(1, 63) != kSortBinRadius1) { printf("FAIL kSortBinRadius1\n"); return false; }
    for (uint32_t Ra = 1; Ra <= 3; Ra++)
        for (uint32_t Na = 0; Na <= 127; Na++)
            for (uint32_t Rb = 1; Rb <= 3; Rb++)
                for (uint32_t Nb = 0; Nb <= 127; Nb++) {
                    g_cases++;
                    const uint32_t la = Na < 63 ? Na : 63, lb = Nb < 63 ? Nb : 63, ba = sort_bin(Ra, Na), bb = sort_bin(Rb, Nb);
                    const bool a_first = Ra > Rb || (Ra == Rb && la > lb), b_first = Rb > Ra || (Ra == Rb && lb > la);
                    if (ba >= kSortBins || (ba < bb) != a_first || (bb < ba) != b_first || (Ra >= 2) != (ba < kSortBinRadius1)) {
                        printf("FAIL sort_bin: radius %u side %u bin %u against radius %u side %u bin %u\n", Ra, Na, ba, Rb, Nb, bb);
                        return false;
                    }
                }
    return true;
}

// ---- the hand-built plan ----
struct Plan {
    std::vector<rawdtw_job_t> jobs;
    std::vector<uint64_t> anchor_off;
    std::vector<PassEntry> todo;
    std::vector<JobRec> recs;
    std::vector<CopyOrder> runtab;
    std::vector<DevJob> side;
    StreamPlanView v;
    const StreamPlanView &view()
    {
        v.n_anchors = anchor_off.back(); v.n_chains = anchor_off.size() - 1;
        v.n_tiles = 1; v.n_slots = 4; v.lds_floats = 2048; v.lane_max_n = 73; v.lane_max_radius = 3;
        v.n_first = 1; v.n_pool = todo.size() - 1; v.n_other = side.size(); v.n_reused = 0;
        v.todo = todo.data(); v.recs = recs.data(); v.runtab = runtab.data(); v.side = side.data(); v.anchor_off = anchor_off.data();
        return v;
    }
};

constexpr uint64_t kEvBase = 1000, kRefBase = 5000000000ull; // where the image's two regions come from in the arenas

static Plan good_plan()
{
    Plan p;
    // three chains of 4, 3 and 2 anchors: job k of chain c's part q lives at anchor (chain end - 2 - q)
    p.anchor_off = {0, 4, 7, 9};
    struct J { uint32_t n, m; int r0; uint32_t excl, anchor; };
    const J js[6] = {{10, 9, 1, 0, 2},   // radius 2
                     {12, 12, 1, 0, 1},  // radius 1
                     {6, 6, 1, 1, 0},    // radius 1, exclude_last
                     {20, 15, 2, 0, 5},  // radius 3
                     {7, 8, 1, 0, 4},    // radius 2, the reference window the longer
                     {30, 30, 4, 0, 7}}; // radius 4: the side list's
    const int order[5] = {3, 0, 4, 1, 2}; // the tile-class jobs as the lanes take them: radius 3, radius 2 (sides 10, 8), radius 1 (sides 12, 6)
    uint32_t ev = 0, rf = 0;
    for (int k : order) { ev += js[k].n; rf += js[k].m; }
    const uint32_t region = (ev + 3u) & ~3u;
    p.jobs.resize(6);
    p.recs.assign(kStreamRecStride, JobRec{0, 0});
    uint32_t at_ev = 0, at_rf = region, r = 0;
    for (int k : order) {
        const J &j = js[k];
        p.jobs[k] = rawdtw_job_t{kRefBase + at_rf, (uint32_t)(kEvBase + at_ev), j.n, j.m, j.r0, j.excl, 0};
        const bool swap = j.n < j.m;
        const uint32_t N = swap ? j.m : j.n, M = swap ? j.n : j.m;
        p.recs[r++] = JobRec{rec_windows(swap ? at_rf : at_ev, swap ? at_ev : at_rf),
                             rec_with_item(rec_shape(N, M, (uint32_t)slanted_radius(j.n, j.m, j.r0), j.excl), kStreamTile - 1 - j.anchor)};
        at_ev += j.n; at_rf += j.m;
    }
    p.jobs[5] = rawdtw_job_t{77777, 4242, js[5].n, js[5].m, js[5].r0, js[5].excl, 0};
    p.side = {DevJob{77777, 4242, js[5].n, js[5].m, slanted_radius(js[5].n, js[5].m, js[5].r0), 0, js[5].anchor}};
    p.runtab.assign(2 * kStreamMaxSeg, CopyOrder{0, 0, 0, 0});
    p.runtab[0] = CopyOrder{0, region / 4, order_src_lo((long long)kEvBase), order_src_hi((long long)kEvBase)};
    p.runtab[1] = CopyOrder{region / 4, (region + rf + 3u) / 4, order_src_lo((long long)kRefBase), order_src_hi((long long)kRefBase)};
    p.todo = {PassEntry{0, 0, pass_counts(5, 1, 3), pass_place(region, 0)}};
    return p;
}

static int g_plans = 0;
static bool expect(Plan p, bool good, const char *what)
{
    StreamPlanStats st;
    const std::string e = check_stream_plan(p.view(), p.jobs.data(), p.jobs.size(), &st);
    g_plans++;
    if (good != e.empty()) { printf("FAIL %s: %s\n", what, good ? e.c_str() : "accepted"); return false; }
    if (good) {
        StreamPlanStats want;
        for (size_t k = 0; k < p.jobs.size(); k++) {
            const bool side = k == 5;
            want.tile_jobs += !side;
            (side ? want.other_bytes : want.tile_bytes) += 4ull * (p.jobs[k].n + p.jobs[k].m) + 36;
        }
        if (st.tile_jobs != want.tile_jobs || st.tile_bytes != want.tile_bytes || st.other_bytes != want.other_bytes) { printf("FAIL %s: statistics\n", what); return false; }
    } else fprintf(stderr, "%s: %s\n", what, e.c_str());
    return true;
}

static bool checker()
{
    const Plan g = good_plan();
    auto with = [&](const std::function<void(Plan &)> &change) { Plan p = g; change(p); return p; };
    auto set_y = [](JobRec &rc, uint32_t N, uint32_t M, uint32_t R, uint32_t ex, uint32_t item) { rc.y = rec_with_item(rec_shape(N, M, R, ex), item); };
    auto y_of = [&](Plan &p, int r, int dN, uint32_t R_xor, uint32_t ex_xor, int item_from) {
        JobRec &rc = p.recs[r];
        set_y(rc, rec_n(rc.y) + dN, rec_m(rc.y), rec_radius(rc.y) ^ R_xor, rec_excl(rc.y) ^ ex_xor, item_from < 0 ? rec_item(rc.y) : rec_item(p.recs[item_from].y));
    };
    auto entry = [](Plan &p, int d_n_hi) {
        PassEntry &t = p.todo[0];
        t.z = pass_counts(pass_jobs(t.z), pass_runs(t.z), pass_n_hi(t.z) + d_n_hi);
    };
    return expect(g, true, "the plan") &&
           expect(with([&](Plan &p) { y_of(p, 1, 1, 0, 0, -1); }), false, "1 a record's N") &&
           expect(with([&](Plan &p) { y_of(p, 0, 0, 1, 0, -1); }), false, "2 a record's radius") &&
           expect(with([&](Plan &p) { y_of(p, 4, 0, 0, 1, -1); }), false, "3 a record's excl") &&
           expect(with([&](Plan &p) { y_of(p, 1, 0, 0, 0, 2); }), false, "4 a record's item, pointing at another job") &&
           expect(with([&](Plan &p) { p.recs[3].x = rec_windows(pass_region(p.todo[0].w), rec_short(p.recs[3].x)); }), false, "5 a window outside every copy order") &&
           expect(with([&](Plan &p) { p.runtab[0].y++; }), false, "6 a copy order reaching over the region") &&
           expect(with([&](Plan &p) { entry(p, -1); }), false, "7 n_hi one too low") &&
           expect(with([&](Plan &p) { entry(p, 1); }), false, "8 n_hi one too high") &&
           expect(with([&](Plan &p) { std::swap(p.recs[0], p.recs[1]); }), false, "9 two records out of bin order") &&
           // (a second, empty pass of the pool is fine at its own slot, and not at the first pass's)
           expect(with([&](Plan &p) { p.todo.push_back(PassEntry{0, 1, 0, 0}); p.runtab.resize(4 * kStreamMaxSeg); }), true, "an empty second pass") &&
           expect(with([&](Plan &p) { p.todo.push_back(PassEntry{0, 0, 0, 0}); p.runtab.resize(4 * kStreamMaxSeg); }), false, "10 a slot used by two entries") &&
           expect(with([&](Plan &p) { p.side[0].R++; }), false, "11 a side-list record's radius") &&
           expect(with([&](Plan &p) { // (the pass's last record leaves for the side list)
               const rawdtw_job_t &j = p.jobs[2];
               p.side.push_back(DevJob{j.ref_off, j.read_off, j.n, j.m, slanted_radius(j.n, j.m, j.band_radius), kFlagExcludeLast, 0});
               p.todo[0].z = pass_counts(4, 1, 3);
           }), false, "12 a tile-class job on the side list");
}

int main()
{
    if (!round_trips() || !checker()) return 1;
    printf("ok %llu %d\n", g_cases, g_plans);
    return 0;
}
