// rawdtw_aln_text.h -- the aln text's launches (rawdtw_aln_text.hip) as the units behind the C ABI enqueue them: rawdtw_aln_text_steps
// there, and the traceback's text form (rawdtw_traceback.cpp) behind a sub-batch's walk.  Internal.
#pragma once
#include "rawdtw_capi.h"

namespace rawdtw {
namespace capi {

// What the kernels read of a path, one record a path in the order the paths' other arrays are in (a traceback sub-batch: plan order):
// the caller's rec, whether the path's last element is dropped before the text is made (exclude_last), and which job of the text the
// path is -- totals and text offsets are in JOB order whatever order the paths are in.
struct AlnDevRec {
    uint64_t off_i, off_j;
    uint32_t j0;
    uint32_t flags; // bit 0: mode, bit 8: drop the last element
    uint64_t job;
};
static_assert(sizeof(AlnDevRec) == sizeof(rawdtw_aln_rec_t), "a device record is the caller's with its pad put to use");

inline AlnDevRec aln_dev_rec(const rawdtw_aln_rec_t &r, bool drop_last, uint64_t job)
{
    return AlnDevRec{r.off_i, r.off_j, r.j0, (r.mode & 1u) | (drop_last ? 0x100u : 0u), job};
}

// All arrays on the device.  Path p is the plen[p] (less one under bit 8) step bytes and distances from poff[p] on.
// count: totals[recs[p].job] = the bytes of path p's text.  scan: text_off[0 .. n] = the exclusive sums of totals[0 .. n).
// write: path p's text at text + text_off[recs[p].job]; it writes exactly the bytes count measured and nothing else.
hipError_t launch_aln_count(const uint8_t *step, const float *d, const uint64_t *poff, const uint32_t *plen, const AlnDevRec *recs, uint64_t n,
                            uint64_t *totals, hipStream_t s);
hipError_t launch_aln_scan(const uint64_t *totals, uint64_t n, uint64_t *text_off, hipStream_t s);
hipError_t launch_aln_write(const uint8_t *step, const float *d, const uint64_t *poff, const uint32_t *plen, const AlnDevRec *recs, uint64_t n,
                            const uint64_t *text_off, char *text, hipStream_t s);

} // namespace capi
} // namespace rawdtw
