// rawdtw_launches.h -- the launches of a plan and of a batch as they are named, counted and timed: the launch kinds, a plan's launch
// record, which of a plan's launches travel as one k_band_merged launch (merge_select), and the table of a batch's reported launches
// (batch_launches) with the slots of their event pairs (event_slot).  No HIP include: a plain compiler takes it
// (tests/abi/batch_launches.cpp).  The table is the ONLY place where a batch's launches are counted and named: rawdtw_batch.cpp's
// enqueue, collect, timed runs and rawdtw_batch_launch_stats read it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rawdtw {

// launch kinds (also reported by rawdtw_plan_run_timed)
enum LaunchKind : uint32_t {
    kKindBandLane = 1,  // lane-per-job banded DP inside the tile kernel (one launch for all eligible jobs)
    kKindBandWave = 2,  // wave-per-job banded kernel
    kKindFullWave = 3,  // wave-per-job full-matrix wavefront (score only)
    kKindFullTb = 4,    // same, writing packed directions
    kKindTbWalk = 5,    // traceback walk
    kKindChainFold = 6, // per-chain fold of the part costs (align_chain)
    kKindReadSelect = 7, // per-read accept/cut loop (gen_chains DTW block)
    kKindBandWreg = 8,   // wave-per-job banded kernel, band in registers (param = registers per lane per buffer)
    kKindBandLaneHi = 9, // tile kernel instance for the wider bands (radius 4..8)
    kKindBandMerged = 10, // reporting only: the tile launch when it also carries the two small banded classes (k_band_merged)
    kKindSemiWave = 11   // wave-per-job semiglobal fill of a local batch (param = rows per lane, + 256 for the pipelined-strip class)
};

struct Launch {
    uint32_t kind;
    int32_t param;      // band tile: LDS floats ; wreg: registers per lane ; full: rows per lane ; band wave: LDS floats
    uint64_t first;     // first plan-order job
    uint64_t count;     // jobs in this launch
};

// a launch as the timed entry points report it: the kind in the low byte, the parameter's low 24 bits above it
inline uint32_t launch_word(uint32_t kind, int32_t param) { return kind | ((uint32_t)param << 8); }

// The wave classes of the wavefront kernels (full-matrix and semiglobal: kKindFullWave, kKindFullTb, kKindSemiWave): rows a lane,
// waves a job, and the parameter a launch of the class reports -- rows a lane, + 256 for the pipelined class.  The launchers take
// the class; a Launch carries the parameter.
constexpr int kFullWgWaves = 4; // waves a job of the pipelined-strip class
struct WaveClass { int rows, waves; int32_t param; };
constexpr int kWaveClasses = 5;
constexpr WaveClass kWaveClass[kWaveClasses] = {{1, 1, 1}, {2, 1, 2}, {4, 1, 4}, {8, 1, 8}, {8, kFullWgWaves, 8 + 256}};
inline int32_t wave_class_param(int cls) { return kWaveClass[cls].param; }
inline int wave_class_of(int32_t param) // -1: no class reports it
{
    for (int c = 0; c < kWaveClasses; c++)
        if (kWaveClass[c].param == param) return c;
    return -1;
}

// Which launches of a plan travel as one k_band_merged launch (indices into the plan's launches, -1 = none).
struct MergeSel { int tile = -1, grp16 = -1, grp8 = -1, wreg = -1; bool on() const { return tile >= 0; } };
inline MergeSel merge_select(bool merge_small, int tile_threads, int n_side, bool serial_launches, const std::vector<Launch> &launches)
{
    MergeSel m;
    if (!merge_small || tile_threads != 256 || (n_side > 0 && !serial_launches)) return m;
    int tile = -1;
    for (size_t i = 0; i < launches.size(); i++) {
        const Launch &L = launches[i];
        if (L.kind == kKindBandLane) tile = (int)i;
        else if (L.kind == kKindBandWreg && L.param == -16) m.grp16 = (int)i;
        else if (L.kind == kKindBandWreg && L.param == -8) m.grp8 = (int)i;
        else if (L.kind == kKindBandWreg && L.param == 0) m.wreg = (int)i;
    }
    if (tile >= 0 && (m.grp16 >= 0 || m.grp8 >= 0 || m.wreg >= 0)) m.tile = tile;
    else m = MergeSel{};
    return m;
}

// One reported launch of a batch.
struct BatchLaunch {
    uint32_t kind;   // as reported: kKindBandMerged for the launch that carries others
    int32_t param;
    int plan;        // index into the plan's launches; -1: none (the device-planned form's launches, fold, select)
    bool carried;    // travels inside the merged launch: no launch of its own, and rawdtw_batch_launch_stats reports it with nothing of its own
    uint32_t word() const { return launch_word(kind, param); }
};

// The reported launches of a batch, in order.  `launches` null: the device-planned form -- the side list's launch (k_wide), then the
// tiles' passes (k_runs) under the merged kind with the image's floats.  Else the job-list form: the plan's launches in plan order under
// `mg`.  Either way the chain fold and the read select are the last two entries.
inline std::vector<BatchLaunch> batch_launches(uint32_t stream_lds, const std::vector<Launch> *launches, const MergeSel &mg)
{
    std::vector<BatchLaunch> t;
    if (!launches) {
        t.push_back({kKindBandWreg, 0, -1, false});
        t.push_back({kKindBandMerged, (int32_t)stream_lds, -1, false});
    } else
        for (int i = 0; i < (int)launches->size(); i++) {
            const Launch &L = (*launches)[i];
            const bool carried = mg.on() && (i == mg.grp16 || i == mg.grp8 || i == mg.wreg);
            t.push_back({mg.on() && i == mg.tile ? (uint32_t)kKindBandMerged : L.kind, L.param, i, carried});
        }
    t.push_back({kKindChainFold, 0, -1, false});
    t.push_back({kKindReadSelect, 0, -1, false});
    return t;
}

// Event pairs of timed runs: run r, launch i of nl has its start event at this slot and its stop event at the next.
inline size_t event_slot(uint32_t r, uint32_t i, uint32_t nl) { return ((size_t)r * nl + i) * 2; }

} // namespace rawdtw
