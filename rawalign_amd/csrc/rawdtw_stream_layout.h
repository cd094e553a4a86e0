// rawdtw_stream_layout.h -- where the arrays of a device-planned batch lie in its pooled workspace (rawdtw_batch.cpp: StreamWs): the
// device block and the page-locked host block, as byte offsets from the batch's shape (reads, chains, the device lists' anchors, the
// full lists' anchors, the kind, "pass_pool").  No HIP include: a plain compiler takes it (tests/abi/stream_layout.cpp).
// Two consumers: batch_create_stream takes `layout`, and rawdtw_events_append (rawdtw_capi.cpp) takes `append_layout` at the end of
// this header, the staging block of a round's new events -- host-side like the batch's and read by no kernel source, which is why it
// sits here and not in rawdtw_events_layout.h (that one rawdtw_events.hip includes).  DESIGN.md 3 and 4.1 say what the arrays are.
// A chunk round's device lists are the SHORT ones (na anchors); n_full counts the full lists', which only the fold walks.
//
//   device region   bytes (each rounded up to 256)            written by                          read by
//   cnt         kCounterBytes                                 uploaded (initial values), k_scan, k_plan, k_runs ...   every kernel; comes home
//   score keep  nc * 4, nc                                    k_fold_select / the select                             come home (with cnt: res_bytes)
//   anchor_off  (nc + 1) * 8                                  uploaded (a round: the short lists')                    k_scan, k_plan, k_gather, the fold
//   anchors     na * 8                                        uploaded; compact: k_scan decodes into it              k_scan, k_plan      (resident arrays: unused)
//   ref_base read_base  nc * 8, nc * 4                        uploaded                                               k_scan, k_plan      (resident arrays: unused)
//   chain_off   (nr + 1) * 8                                  uploaded                                               the select
//   tlist       n_tiles * 8                                   k_scan                                                 k_plan
//   todo        n_slots * 16        pass entries              k_plan                                                 k_runs
//   recs        n_tiles * kStreamRecStride * 8  job records   k_plan                                                 k_runs
//   runtab      n_slots * kSlotOrders * 16      copy orders   k_plan                                                 k_runs
//   tile_stats  n_tiles * 24  (3 words a scan unit are used)  k_scan                                                 the statistics' sum
//   omix ojobs  others_cap * sizeof(DevJob) each  side list   k_scan, k_side                                         k_side, k_wide
//   ocls        others_cap                                    k_scan                                                 k_side
//   chains      nc * kChainDescBytes                          k_scan                                                 k_gather, the fold
//   fold_order full gate  nc * 4 each                         k_scan, the fold                                       the fold, the select
//   out         na * 4        a cost an anchor of the device lists   k_runs, k_wide                                  the fold (a round: k_gather)
//   heads unit_abs  compact: nc * 8, n_units * 8              uploaded                                               k_scan
//   steps       compact: n_units * RAWDTW_COMPACT_STRIDE * 2  uploaded (na of them: k_scan loads whole units)        k_scan
//   wide        compact: n_wide * sizeof(rawdtw_wide_step_t)  uploaded                                               k_scan
//   carry full_off  a chunk round: nc * 24, (nc + 1) * 8      uploaded                                               k_scan, k_gather, the fold
//   out_full    a chunk round: n_full * 4  a cost an anchor of the full lists   k_gather                             the fold, the next round's k_gather
//   pinned region   cnt score keep at the device block's offsets: the counters' initial values go up from cnt, and one copy of
//                   res_bytes brings all three home
// A region the kind does not use has `bytes` 0 (its `at` is where the next one starts).
#pragma once
#include "rawdtw_layout.h"
#include "rawdtw_plan_fmt.h"

#include "../../include/rawdtw.h"

namespace rawdtw {
namespace stream {

using ws::Region;

enum class Kind { plain, compact, round };

// (what lives behind hip_runtime.h, named here and pinned where both are visible: rawdtw_batch.cpp)
constexpr size_t kCounterBytes = 192 * 8; // kStreamCounters words
constexpr size_t kChainDescBytes = 24;    // sizeof(ChainDesc)
constexpr size_t kSlotOrders = 2 * kStreamMaxSeg; // copy orders of a slot: a run of each arena

struct Shape {
    uint64_t nr = 0, nc = 0, na = 0, n_full = 0; // reads, chains, anchors of the device lists, anchors of the full lists (a round: na <= n_full)
    Kind kind = Kind::plain;
    uint64_t n_wide = 0; // compact: the escape list's entries
    int pass_pool = -1;  // copy-order slots beyond one a tile; -1: 3 a tile + 64
};

struct Layout {
    // the derived counts.  n_slots: a tile over the image budget or the run table takes further passes, a slot of copy orders each -- rare
    // in a mapper's batch, the rule for tiles of very short chains
    uint32_t n_tiles = 0, n_slots = 0;
    uint64_t others_cap = 0, n_units = 0; // the side list's capacity; units of RAWDTW_COMPACT_STRIDE anchors
    Region cnt, score, keep, anchor_off, anchors, ref_base, read_base, chain_off, tlist, todo, recs, runtab, tile_stats, omix, ojobs, ocls,
        chains, fold_order, full, gate, out, heads, unit_abs, steps, wide, carry, full_off, out_full; // the device block, in this order
    size_t need = 0, res_bytes = 0; // res_bytes: from cnt to the end of keep's nc bytes
    Region p_cnt, p_score, p_keep;  // the pinned block
    size_t pin_need = 0;
};

inline Layout layout(const Shape &s)
{
    const uint64_t nc = s.nc, na = s.na;
    const bool compact = s.kind == Kind::compact, round = s.kind == Kind::round;
    Layout L;
    L.n_tiles = (uint32_t)((na + kStreamTile - 1) / kStreamTile);
    L.n_slots = s.pass_pool >= 0 ? L.n_tiles + (uint32_t)s.pass_pool : 4 * L.n_tiles + 64;
    L.others_cap = na < na / 4 + 4096 ? na : na / 4 + 4096;
    L.n_units = (na + RAWDTW_COMPACT_STRIDE - 1) / RAWDTW_COMPACT_STRIDE;
    ws::Take walk;
    auto take = [&](size_t bytes) { return walk(ws::al(bytes)); };
    L.cnt = take(kCounterBytes); L.score = take(nc * 4); L.keep = take(nc);
    L.anchor_off = take((nc + 1) * 8); L.anchors = take(na * sizeof(rawdtw_anchor_t)); L.ref_base = take(nc * 8); L.read_base = take(nc * 4);
    L.chain_off = take((s.nr + 1) * 8);
    L.tlist = take((size_t)L.n_tiles * 8); L.todo = take((size_t)L.n_slots * 16);
    L.recs = take((size_t)L.n_tiles * kStreamRecStride * 8); L.runtab = take((size_t)L.n_slots * kSlotOrders * 16);
    L.tile_stats = take((size_t)L.n_tiles * 24);
    L.omix = take(L.others_cap * sizeof(DevJob)); L.ojobs = take(L.others_cap * sizeof(DevJob)); L.ocls = take(L.others_cap);
    L.chains = take(nc * kChainDescBytes); L.fold_order = take(nc * 4); L.full = take(nc * 4); L.gate = take(nc * 4);
    L.out = take(na * 4);
    L.heads = take(compact ? nc * sizeof(rawdtw_anchor_t) : 0); L.unit_abs = take(compact ? L.n_units * sizeof(rawdtw_anchor_t) : 0);
    L.steps = take(compact ? L.n_units * RAWDTW_COMPACT_STRIDE * 2 : 0); L.wide = take(compact ? s.n_wide * sizeof(rawdtw_wide_step_t) : 0);
    L.carry = take(round ? nc * sizeof(rawdtw_carry_t) : 0); L.full_off = take(round ? (nc + 1) * 8 : 0); L.out_full = take(round ? s.n_full * 4 : 0);
    L.need = walk.p;
    L.res_bytes = L.keep.at + nc;
    L.p_cnt = L.cnt; L.p_score = L.score; L.p_keep = L.keep;
    L.pin_need = L.keep.at + L.keep.bytes;
    return L;
}

// rawdtw_events_append's staging block (rawdtw_capi.cpp, grow-only): the round's new events and the two segment tables
struct AppendLayout {
    Region ev, src, dst; // n_new * 4 uploaded; (n_segments + 1) * 8, n_segments * 4 uploaded: k_events_scatter reads all three
    size_t need = 0;
};

inline AppendLayout append_layout(uint64_t n_new, uint32_t n_segments)
{
    AppendLayout L;
    ws::Take walk;
    L.ev = walk(ws::al(n_new * 4)); L.src = walk(ws::al(((size_t)n_segments + 1) * 8)); L.dst = walk(ws::al((size_t)n_segments * 4));
    L.need = walk.p;
    return L;
}

} // namespace stream
} // namespace rawdtw
