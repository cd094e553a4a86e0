// rawdtw_options.h -- the context options (rawdtw_set_option / rawdtw_get_option, RAWDTW_OPTS, rawdtw_plan_dry_run's options): their
// one definition.  A row of RAWDTW_OPTIONS gives an option's name -- which is also its field in the record `Options` that rawdtw_ctx and
// the planner's PlanCfg derive from --, the field's type and default, the rule a value passes through on its way in, and flags.  The
// setter, the getter, the dry run and the environment all go through set() and get() below.  To add an option, add its row here and its
// line in the option block of include/rawdtw.h (tests/test_options_cpu.py holds the two lists against each other): nothing else.
// No HIP include: a plain C++ test program takes this header (tests/abi/options.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/rawdtw.h"
#include "rawdtw_plan_fmt.h" // kMaxLaneRadius, kLaneMaxN, kStreamMaxImageFloats

namespace rawdtw {

// tile kernel of the job-list path: a tile = consecutive lane-eligible jobs whose windows fit this much LDS (8 workgroups per CU) ...
constexpr uint32_t kTileLdsFloats = 4800;
constexpr uint32_t kTileMaxJobs = 1024; // ... at most this many jobs ...
constexpr uint32_t kTileMaxSpans = 96;  // ... out of at most this many spans of the arenas

namespace opt {

// The rule a value passes through: kind, a, b, c, the message of a refusal.
enum Kind : uint8_t { kFlag, kClamp, kRefuse, kSnap, kRaw };
#define RAWDTW_OPT_FLAG rawdtw::opt::kFlag, 0, 0, 0, nullptr                          /* value != 0 */
#define RAWDTW_OPT_CLAMP(lo, hi) rawdtw::opt::kClamp, (lo), (hi), 0, nullptr          /* clamped to [lo, hi] */
#define RAWDTW_OPT_REFUSE(lo, hi, msg) rawdtw::opt::kRefuse, (lo), (hi), 0, (msg)     /* RAWDTW_ERR_INVALID outside [lo, hi]: nothing is stored */
#define RAWDTW_OPT_STRICT01(msg) RAWDTW_OPT_REFUSE(0, 1, msg)                         /* (an opt-in: a value that is neither is not read as "on") */
#define RAWDTW_OPT_SNAP(a, b, c) rawdtw::opt::kSnap, (a), (b), (c), nullptr           /* c from c on, b from b on, else a */
#define RAWDTW_OPT_RAW rawdtw::opt::kRaw, 0, 0, 0, nullptr                            /* as given, cut to the field's width (the debug masks) */
enum Flags : uint32_t {
    kReadOnly = 1,   // computed by the library: rawdtw_get_option answers, every setter refuses the name
    kPlanner = 2,    // read by the host planner: rawdtw_plan_dry_run takes it
    kMarksTileLds = 4 // "tile_lds_floats": setting it also sets Options::tile_lds_set
};

// X(name, type, default, rule, flags)
#define RAWDTW_OPTIONS(X) \
    /* -- the job-list planner (rawdtw_planner.cpp) -- */ \
    X(lane_max_radius, int, kMaxLaneRadius, RAWDTW_OPT_CLAMP(0, kMaxLaneRadius), kPlanner) /* radii above this go to the register-resident wave kernel */ \
    X(lane_max_n, uint32_t, kLaneMaxN, RAWDTW_OPT_CLAMP(8, kLaneMaxN), kPlanner)  /* ... and longer sides than this off the tile kernel */ \
    X(lane_hi, bool, false, RAWDTW_OPT_FLAG, kPlanner)                 /* radii 4..8 on the second tile-kernel instance (else on k_band_wreg<1>) */ \
    X(lane_hi_max_n, uint32_t, 96, RAWDTW_OPT_CLAMP(8, 200), kPlanner) /* ... for sides up to this */ \
    X(micro_max_n, int, 8, RAWDTW_OPT_SNAP(0, 4, 8), kPlanner)         /* shapes with longer side <= this use the micro paths (0: none, 4: micro4 only) */ \
    X(grp16, bool, true, RAWDTW_OPT_FLAG, kPlanner)                    /* bands of at most 16 offsets: four jobs per wave (else one job per wave) */ \
    X(grp8, bool, true, RAWDTW_OPT_FLAG, kPlanner)                     /* ... and of at most 8 offsets: eight jobs per wave */ \
    X(full_wg, bool, true, RAWDTW_OPT_FLAG, kPlanner)                  /* full-matrix jobs with >= 3 strips: four waves per job, pipelined strips */ \
    X(tile_lds_floats, uint32_t, kTileLdsFloats, RAWDTW_OPT_CLAMP(1024, kStreamMaxImageFloats), kPlanner | kMarksTileLds) \
    X(tile_max_jobs, uint32_t, kTileMaxJobs, RAWDTW_OPT_CLAMP(64, 65535), kPlanner) \
    X(tile_max_spans, uint32_t, kTileMaxSpans, RAWDTW_OPT_CLAMP(8, 4096), kPlanner) \
    /* Optional: tile-eligible jobs that are rare inside a tile (long, or of a radius few neighbours share) leave the job order and are tiled by */ \
    /* shape instead: longer side >= sort_n, radius 1 with longer side >= sort_r1_n, radius 3 (0 = never).  Measured on the bench workload with */ \
    /* sort_n = 17: the tile kernel's VALU work drops 40 % (full waves of one shape), but every such job then fetches its own cache lines */ \
    /* (+130 MB of scattered reads per batch); alone the kernel breaks even, with several batches in flight throughput falls 5-15 %. */ \
    X(sort_n, uint32_t, 0, RAWDTW_OPT_CLAMP(0, 255), kPlanner) \
    X(sort_r1_n, uint32_t, 0, RAWDTW_OPT_CLAMP(0, 255), kPlanner) \
    X(sort_r3, uint32_t, 0, RAWDTW_OPT_FLAG, kPlanner) \
    X(sorted_tile_jobs, uint32_t, 64, RAWDTW_OPT_CLAMP(16, 1024), kPlanner) \
    X(plan_threads, int, 0, RAWDTW_OPT_CLAMP(0, 64), 0)                /* planner threads (0: from the job count and the machine, at most 16) */ \
    /* -- the job-list path's launches -- */ \
    X(serial_launches, bool, false, RAWDTW_OPT_FLAG, 0)                /* with side streams, a batch's launches in sequence anyway */ \
    X(merge_small, bool, true, RAWDTW_OPT_FLAG, 0)                     /* tile + 16-lane-row + register-wave launches of a batch as one launch (k_band_merged) */ \
    X(tile_threads, int, 256, RAWDTW_OPT_SNAP(256, 512, 1024), 0)      /* workgroup size of the tile kernel */ \
    /* 0: wave per chain, 1/2: lane per chain (16/32 parts per round; 30x less VALU work), 3: lanes + a wave for each long chain, */ \
    /* 4: sync-free batches fold and select in one launch, a read a lane (k_fold_select), job-list batches as 3 */ \
    X(fold_mode, int, 4, RAWDTW_OPT_CLAMP(0, 4), 0) \
    X(fold_long_parts, uint32_t, 768, RAWDTW_OPT_CLAMP(1, 1 << 30), 0) /* fold_mode 3: chains of at least this many parts are folded a wave each */ \
    X(debug_skip_kinds, uint32_t, 0, RAWDTW_OPT_RAW, 0)                /* timing experiments: launches of these kinds are not issued (results are then wrong) */ \
    X(debug_skip_tail, uint32_t, 0, RAWDTW_OPT_RAW, 0)                 /* ... on the sync-free path: 1 no fold launch, 2 no select launch (results are then wrong) */ \
    /* -- device-planned batches (rawdtw_batch.cpp, rawdtw_runs.hip) -- */ \
    X(device_plan, bool, true, RAWDTW_OPT_FLAG, 0)                     /* rawdtw_batch_create takes the sync-free stream path for sparse + banded batches */ \
    X(device_plan_min_jobs, uint64_t, 0, RAWDTW_OPT_CLAMP(0, INT64_MAX), 0) /* smaller batches go through the job list */ \
    X(stream_tile_radius, int, 3, RAWDTW_OPT_CLAMP(1, kMaxLaneRadius), 0) /* the tiles' radius limit */ \
    X(stream_threads, int, 256, RAWDTW_OPT_SNAP(256, 256, 512), 0)     /* workgroup size of k_runs */ \
    X(stream_blocks_per_cu, int, 4, RAWDTW_OPT_CLAMP(0, 16), 0)        /* 0: what the occupancy query gives; else at most this many (leaves room for other streams' kernels) */ \
    X(stream_debug, uint32_t, 0, RAWDTW_OPT_RAW, 0)                    /* StreamArgs::debug */ \
    X(pass_pool, int, -1, RAWDTW_OPT_CLAMP(-1, 1 << 24), 0)            /* copy-order slots beyond one a tile (tests: a batch that runs out is redone through the job list); -1: 3 a tile + 64 */ \
    X(wide_blocks, uint32_t, 256, RAWDTW_OPT_CLAMP(1, 65535), 0)       /* workgroups (four waves each) of the side list's launch */ \
    X(wide_at_create, int, 0, RAWDTW_OPT_FLAG, 0)                      /* 1: that launch also after a plain rawdtw_batch_create (the caller leaves the arenas alone until the run) */ \
    X(wide_order, int, 0, RAWDTW_OPT_CLAMP(0, 2), 0)                   /* 0: k_wide between the scan and the pass planning (first run), 1: in front of k_runs, 2: behind it */ \
    X(wide_beside, int, 0, RAWDTW_OPT_FLAG, 0)                         /* 1: on the context's second stream, beside the tiles' launch (measured: the fork and join cost the fresh-batch pipeline 8 % and the PCIe loop 17 %) */ \
    X(resident_arrays, bool, false, RAWDTW_OPT_FLAG, 0)                /* rawdtw_batch_create: anchors / ref_base / read_base are DEVICE pointers (used in place) */ \
    X(time_plan, bool, false, RAWDTW_OPT_FLAG, 0)                      /* record an event pair around a batch's planning kernels (rawdtw_batch_plan_ms) */ \
    /* -- traceback -- */ \
    X(tb_workspace_mb, uint64_t, 0, RAWDTW_OPT_CLAMP(0, 1 << 30), 0)   /* direction-buffer budget of a traceback sub-batch in MiB (0: RAWDTW_TB_WORKSPACE_MB, else 16 GiB) */ \
    /* -- seeding, chaining and the mapper's rounds (opt-ins) -- */ \
    X(seed_minimizer, bool, false, RAWDTW_OPT_FLAG, 0)                 /* rawdtw_seed.hip seeds a w > 0 table on the device (k_seed_min) rather than refusing it */ \
    X(chain_long_seeds, uint32_t, 0, RAWDTW_OPT_CLAMP(0, 1 << 20), 0)  /* reads above the cap with at most this many seeds are chained by rawdtw_chain.hip's long path (0: declined) */ \
    /* a read with up to this many chains, ties or not, is ordered on the device by rawdtw_sort_order.h (0: 32 chains, 16 with ties); a count that */ \
    /* sizes device arrays: a value outside its range is refused, not clamped */ \
    X(chain_max_chains, uint32_t, 0, RAWDTW_OPT_REFUSE(0, 4096, "\"chain_max_chains\" is 0 (off) or 1 .. 4096"), 0) \
    /* a read the device chaining cannot take is declined alone (rawdtw_chain_round_declined), not its round */ \
    X(chain_decline_reads, bool, false, RAWDTW_OPT_STRICT01("\"chain_decline_reads\" is 0 (off) or 1"), 0) \
    X(device_round_end, bool, false, RAWDTW_OPT_FLAG, 0)               /* a mapper created with this context ends its device-chained rounds on the device */ \
    X(resident_chains, uint32_t, 0, RAWDTW_OPT_CLAMP(0, 1 << 20), 0)   /* ... and keeps a resident round's primary chains on the device, at most this many seeds a read (0: no) */ \
    /* a mapper created with this context takes --dtw-output-cigar through its rounds from signal; its finish reads the arena */ \
    X(signal_cigar, bool, false, RAWDTW_OPT_STRICT01("\"signal_cigar\" is 0 (off) or 1"), 0) \
    X(signal_events_cap, uint64_t, 0, RAWDTW_OPT_CLAMP(0, INT64_MAX), 0) /* the events_cap of a round from signal's first try (rawdtw_mapper.cpp; 0: the mapper's guess) */

// X(name): what rawdtw_get_option computes from the context, by a function of that name in rawdtw::capi (rawdtw_capi.cpp lists them)
#define RAWDTW_COMPUTED_OPTIONS(X) \
    X(tb_sub_batches)       /* sub-batches of the most recent traceback call, known before its first plan is built */ \
    X(round_end_kernel_us)  /* the most recent fetched round end's launch, from its event pair */ \
    X(round_keep_kernel_us) /* the most recent fetched keep launch, from its event pair */

} // namespace opt

// the options as a context and a plan hold them
struct Options {
#define X(name, type, dflt, rule, flags) type name = dflt;
    RAWDTW_OPTIONS(X)
#undef X
    bool tile_lds_set = false; // "tile_lds_floats" was given: it also sizes the device-planned batches' tiles
};

namespace opt {

struct Row {
    const char *name;
    Kind kind;
    int64_t a, b, c;
    const char *refusal;
    uint32_t flags;
    void (*store)(Options &, int64_t); // (null for a computed row)
    int64_t (*load)(const Options &);
};

namespace field {
#define X(name, type, dflt, rule, flags)                                     \
    inline void store_##name(Options &o, int64_t v) { o.name = (type)v; }  \
    inline int64_t load_##name(const Options &o) { return (int64_t)o.name; }
RAWDTW_OPTIONS(X)
#undef X
} // namespace field

inline const Row kRows[] = {
#define X(name, type, dflt, rule, flags) {#name, rule, flags, field::store_##name, field::load_##name},
    RAWDTW_OPTIONS(X)
#undef X
#define X(name) {#name, kRaw, 0, 0, 0, nullptr, kReadOnly, nullptr, nullptr},
    RAWDTW_COMPUTED_OPTIONS(X)
#undef X
};
#define X(name) +1
constexpr size_t kNumRows = sizeof(kRows) / sizeof(kRows[0]), kNumSettable = kNumRows - (0 RAWDTW_COMPUTED_OPTIONS(X)); // (the computed rows come last)
#undef X

inline const Row *find(const char *name)
{
    for (const Row &r : kRows)
        if (!strcmp(r.name, name)) return &r;
    return nullptr;
}

// `value` through the row of `name` into `o`.  RAWDTW_ERR_INVALID and `err` for a name that is not a row, is read-only or lacks one of the
// flags in `need`, and for a value the row's rule refuses: `o` is then as it was.
inline int set(Options &o, const char *name, int64_t value, std::string &err, uint32_t need = 0)
{
    const Row *r = find(name);
    if (!r || (r->flags & kReadOnly) || (r->flags & need) != need) { err = std::string("unknown option ") + name; return RAWDTW_ERR_INVALID; }
    switch (r->kind) {
    case kFlag: value = value != 0; break;
    case kClamp: value = value < r->a ? r->a : (value > r->b ? r->b : value); break;
    case kRefuse: if (value < r->a || value > r->b) { err = r->refusal; return RAWDTW_ERR_INVALID; } break;
    case kSnap: value = value >= r->c ? r->c : (value >= r->b ? r->b : r->a); break;
    case kRaw: break;
    }
    r->store(o, value);
    if (r->flags & kMarksTileLds) o.tile_lds_set = true;
    return RAWDTW_OK;
}

// the stored value of a settable option; RAWDTW_ERR_INVALID for any other name (a computed one needs its context: rawdtw_get_option)
inline int get(const Options &o, const char *name, int64_t *value)
{
    const Row *r = find(name);
    if (!r || !r->load) return RAWDTW_ERR_INVALID;
    *value = r->load(o);
    return RAWDTW_OK;
}

} // namespace opt
} // namespace rawdtw
