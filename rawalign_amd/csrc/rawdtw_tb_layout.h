// rawdtw_tb_layout.h -- the traceback driver's blocks (rawdtw_tb_driver.cpp) as byte offsets, and its split.  Three grow-only blocks of
// the context are cut in two SLOTS each (sub-batch k uses slot k & 1): the device path block, the page-locked landing zone and, for
// the text form, the text block.  No HIP include: a plain compiler takes it (tests/abi/tb_layout.cpp).  A slot serves cnt jobs whose
// paths hold acc = the sum of (n + m - 1) elements; every region is rounded up to 256 bytes.
//   paths    recs (what the path keeps on the device for its launches: `recs` below; none for the full matrix), poff cnt * 8 and plen
//            cnt * 4 by position, extra cnt * 4 if the path has one more word a job (j0), ti tj (i, j) end-first acc * 4 each: the walk's
//            scratch, pd acc * 4 and mv acc: distances and step bytes, start-first
//   landing  pd mv as above (the text form: none, no path crosses home), cost cnt * 4 inside the stretch, plen and extra cnt * 4 by
//            position, the text form's toff (cnt + 1) * 8
//   text     rec cnt * 32 (AlnDevRec), tot cnt * 8, toff (cnt + 1) * 8, text bound + 16
#pragma once
#include <vector>

#include "rawdtw_layout.h"

namespace rawdtw {
namespace tb {

using ws::Region;

// a block of two slots that holds `need` bytes a slot with an eighth to spare; slot 1 starts at half of it, on a 256-byte boundary
inline size_t block_bytes(size_t need) { return 2 * ws::al(need + need / 8); }
inline size_t slot_at(size_t block, int slot) { return (size_t)slot * (block / 2); }

// every region of a walk rounded up to 256
struct Take256 {
    ws::Take take;
    Region operator()(size_t bytes) { return take(ws::al(bytes)); }
};

struct Paths { Region recs, poff, plen, extra, ti, tj, pd, mv; size_t need; };
inline Paths paths(uint64_t cnt, uint64_t acc, bool extra, size_t rec_bytes)
{
    Take256 t;
    Paths L{t(rec_bytes), t(cnt * 8), t(cnt * 4), t(extra ? cnt * 4 : 0), t(acc * 4), t(acc * 4), t(acc * 4), t(acc), 0}; // (a braced list is evaluated in order)
    L.need = t.take.p;
    return L;
}

struct Landing { Region pd, mv, cost, plen, extra, toff; size_t need; };
inline Landing landing(uint64_t cnt, uint64_t acc, bool extra, bool text)
{
    Take256 t;
    Landing L{t(text ? 0 : acc * 4), t(text ? 0 : acc), t(cnt * 4), t(cnt * 4), t(extra ? cnt * 4 : 0), t(text ? (cnt + 1) * 8 : 0), 0};
    L.need = t.take.p;
    return L;
}

constexpr size_t kAlnRecBytes = 32; // sizeof(AlnDevRec)
struct Text { Region rec, tot, toff, text; size_t need; };
inline Text text(uint64_t cnt, uint64_t bound)
{
    Take256 t;
    Text L{t(cnt * kAlnRecBytes), t(cnt * 8), t((cnt + 1) * 8), t(bound + 16), 0};
    L.need = t.take.p;
    return L;
}

// What the banded and the semiglobal path keep in a slot: a job record and an aux record a job (their sizes: the caller's sizeof),
// the costs (indexed inside the stretch) and, semiglobal only, the end columns and the boundary rows.  The semiglobal cost and span
// forms (one pass, no paths) lay their call's block out by the same walk; j0 is the span form's start columns.
struct Recs { Region jobs, aux, cost, endj, j0, bnd; size_t need = 0; };
inline Recs recs(uint64_t cnt, size_t job_bytes, size_t aux_bytes, bool endj, bool j0, uint64_t bnd_floats)
{
    Take256 t;
    Recs L{t(cnt * job_bytes), t(cnt * aux_bytes), t(cnt * 4), t(endj ? cnt * 4 : 0), t(j0 ? cnt * 4 : 0), t(bnd_floats * 4), 0};
    L.need = t.take.p;
    return L;
}

// The split: a job joins the current sub-batch unless that passes the budget (a job over the budget goes alone).  Sub-batches hold
// whole jobs in job order.
struct Cut { uint64_t begin, cnt; };
inline std::vector<Cut> split(const uint64_t *job_bytes, uint64_t n_jobs, uint64_t budget)
{
    std::vector<Cut> cuts;
    for (uint64_t begin = 0; begin < n_jobs;) {
        uint64_t end = begin, bytes = 0;
        while (end < n_jobs) {
            if (end > begin && bytes + job_bytes[end] > budget) break;
            bytes += job_bytes[end];
            end++;
        }
        cuts.push_back(Cut{begin, end - begin});
        begin = end;
    }
    return cuts;
}

} // namespace tb
} // namespace rawdtw
