// rawdtw_plan_check.cpp -- the host's readers of a device-planned batch's plan (rawdtw_plan_check.h): the self-check behind
// rawdtw_batch_verify_plan and the chunk profile behind rawdtw_batch_chunk_profile, over the arrays rawdtw_batch.cpp
// downloaded.  The records' formats: rawdtw_plan_fmt.h.  No HIP here: tests/abi/plan_fmt.cpp links this file alone.
#include "rawdtw_plan_check.h"

#include <algorithm>
#include <vector>

#include "rawdtw_chunks.h"

namespace rawdtw {

// What the scan left behind for the DTW launch, against the job list the host builds from the same chains
// (rawdtw_batch_build_jobs): every job either of the tile class by the class rule, then in exactly one pass's records
// with its shape, radius, flag and windows, or in the side list exactly once with the job's windows, shape, slanted
// radius and flag.
std::string check_stream_plan(const StreamPlanView &v, const rawdtw_job_t *jobs, uint64_t n_jobs, StreamPlanStats *expect)
{
    auto S = [](uint64_t x) { return std::to_string(x); };
    const uint64_t na = v.n_anchors, n_todo = v.n_todo();
    if (!v.fits_slots()) return "work list longer than the slots";
    // job k of chain c's part p lives at anchor index a1 - 2 - p
    std::vector<uint64_t> slot_job(na, ~0ull);
    {
        uint64_t k = 0;
        for (uint64_t c = 0; c < v.n_chains; c++) {
            const uint64_t a0 = v.anchor_off[c], a1 = v.anchor_off[c + 1];
            for (uint64_t pidx = 0; a1 > a0 && pidx + 1 < a1 - a0 && a1 - 2 - pidx < na; pidx++) slot_job[a1 - 2 - pidx] = k++;
        }
        if (k != n_jobs) return "job count";
    }
    StreamPlanStats st;
    std::vector<uint8_t> is_tile(n_jobs, 0);
    for (uint64_t k = 0; k < n_jobs; k++) {
        const rawdtw_job_t &j = jobs[k];
        const int R = slanted_radius(j.n, j.m, j.band_radius);
        const uint32_t N = std::max(j.n, j.m);
        is_tile[k] = R <= v.lane_max_radius && N <= v.lane_max_n;
        st.tile_jobs += is_tile[k];
        (is_tile[k] ? st.tile_bytes : st.other_bytes) += 4ull * ((uint64_t)j.n + j.m) + 36ull;
    }
    std::vector<uint8_t> oseen(n_jobs, 0);
    for (uint64_t q = 0; q < v.n_other; q++) {
        const DevJob &d = v.side[q];
        const uint64_t k = d.aux < na ? slot_job[d.aux] : ~0ull;
        if (k == ~0ull || oseen[k] || is_tile[k]) return "side-list entry " + S(q) + " (anchor " + S(d.aux) + ") duplicated, of the tile class or no job at all";
        if (d.n != jobs[k].n || d.m != jobs[k].m || d.ref_off != jobs[k].ref_off || d.read_off != jobs[k].read_off ||
            d.R != slanted_radius(d.n, d.m, jobs[k].band_radius) || ((d.flags & kFlagExcludeLast) != 0) != (jobs[k].exclude_last != 0))
            return "side-list record of job " + S(k) + " differs from the job";
        oseen[k] = 1;
    }
    for (uint64_t k = 0; k < n_jobs; k++)
        if (!is_tile[k] && !oseen[k]) return "job " + S(k) + " is in no launch";
    // Every pass: its entry sits at its slot; its records name tile-class jobs of its tile, each job once over all passes,
    // with the job's shape, slanted radius and flag, in the order the lanes take them (radius class, longer side); a record's
    // windows lie in the image, inside one of the pass's copy orders, and that order maps them onto the job's windows in the
    // arenas.
    std::vector<uint8_t> tseen(n_jobs, 0);
    for (uint64_t q = 0; q < n_todo; q++) {
        const PassEntry t = v.todo[q];
        const uint32_t nj = pass_jobs(t.z), nr = pass_runs(t.z), n_hi = pass_n_hi(t.z), region = pass_region(t.w), rec0 = pass_rec0(t.w);
        // (a slot other than the entry's own is one used twice, or one k_runs never reads the entry of)
        if (t.x >= v.n_tiles || t.y != v.slot_of(q) || nj > kStreamTile || nr > kStreamMaxSeg || (nj && !nr) || n_hi > nj || (rec0 & 1u) || rec0 + nj > kStreamRecStride)
            return "work list entry " + S(q) + ": tile " + S(t.x) + ", slot " + S(t.y) + ", " + S(nj) + " jobs, " + S(nr) + " runs, first radius-1 record " + S(n_hi);
        if (!nj) continue;
        const JobRec *recs = v.recs + (uint64_t)t.x * kStreamRecStride + rec0;
        const CopyOrder *ords = v.runtab + q * (2 * kStreamMaxSeg);
        for (uint32_t o = 0; o < 2 * nr; o++) {
            const CopyOrder &od = ords[o];
            const bool evs = (o & 1u) == 0;
            if (od.x >= od.y || 4ull * od.y > v.lds_floats || (evs ? 4ull * od.y > region : 4ull * od.x < region))
                return "pass " + S(q) + " (tile " + S(t.x) + ", " + S(nj) + " jobs, " + S(nr) + " runs, event region " + S(region) + " of " + S(v.lds_floats) +
                       " floats): copy order " + S(o) + " = pieces [" + S(od.x) + ", " + S(od.y) + ") outside its region of the image";
        }
        uint32_t prev_bin = 0, n_wide = 0; // (n_wide: the pass's records of radius >= 2 -- the entry's n_hi, where the chunks of k_runs change class)
        for (uint32_t r = 0; r < nj; r++) {
            const JobRec rc = recs[r];
            const uint32_t N = rec_n(rc.y), M = rec_m(rc.y), R = rec_radius(rc.y), ex = rec_excl(rc.y), u = rec_item(rc.y);
            const uint64_t i = ((uint64_t)t.x + 1) * kStreamTile - 1 - u;
            const uint64_t k = i < na ? slot_job[i] : ~0ull;
            const std::string who = "pass " + S(q) + " record " + S(r) + " (anchor " + S(i) + ")";
            if (k == ~0ull || !is_tile[k] || tseen[k]) return who + ": no job, not of the tile class, or in two passes";
            const rawdtw_job_t &j = jobs[k];
            const bool swap = j.n < j.m;
            if (N != std::max(j.n, j.m) || M != std::min(j.n, j.m) || (int)R != slanted_radius(j.n, j.m, j.band_radius) || (ex != 0) != (j.exclude_last != 0))
                return who + ": shape, radius or flag differ from job " + S(k);
            const uint32_t bin = sort_bin(R, N);
            if (bin < prev_bin) return who + ": out of the lanes' order";
            prev_bin = bin;
            if (R >= 2u) n_wide++;
            else if (r < n_hi) return who + ": radius 1 ahead of the pass's first radius-1 record " + S(n_hi);
            if (r >= n_hi && R != 1u) return who + ": radius " + S(R) + " at or behind the pass's first radius-1 record " + S(n_hi);
            const uint32_t p_ev = swap ? rec_short(rc.x) : rec_long(rc.x), p_rf = swap ? rec_long(rc.x) : rec_short(rc.x);
            for (int w = 0; w < 2; w++) {
                const uint32_t pw = w ? p_rf : p_ev, len = w ? j.m : j.n;
                const uint64_t want = w ? j.ref_off : (uint64_t)j.read_off;
                bool ok = false;
                for (uint32_t g = 0; g < nr && !ok; g++) {
                    const CopyOrder &od = ords[2 * g + w];
                    ok = 4ull * od.x <= pw && (uint64_t)pw + len <= 4ull * od.y && (long long)pw + order_src(od.z, od.w) == (long long)want;
                }
                if (!ok) return who + ": its " + (w ? "reference" : "event") + " window is in no copy order of the pass";
            }
            tseen[k] = 1;
        }
        if (n_wide != n_hi) return "pass " + S(q) + ": " + S(n_wide) + " records of radius >= 2, its entry says " + S(n_hi);
    }
    if (v.n_reused == 0) // (a round that took costs over leaves the carried parts out)
        for (uint64_t k = 0; k < n_jobs; k++)
            if (is_tile[k] && !tseen[k]) return "tile-class job " + S(k) + " is in no pass";
    if (expect) *expect = st;
    return "";
}

bool stream_chunk_profile(const StreamPlanView &v, bool flat_map, uint64_t w[21])
{
    std::fill(w, w + 21, 0ull);
    if (!v.fits_slots()) return false;
    for (uint64_t q = 0; q < v.n_todo(); q++) {
        const PassEntry t = v.todo[q];
        const uint32_t nj = pass_jobs(t.z), rec0 = pass_rec0(t.w);
        if (t.x >= v.n_tiles || nj > kStreamTile || rec0 + nj > kStreamRecStride || pass_n_hi(t.z) > nj) return false;
        if (!nj) continue;
        const JobRec *rc = v.recs + (size_t)t.x * kStreamRecStride + rec0;
        uint32_t n3 = 0;
        for (uint32_t r = 0; r < nj && r < 64u; r++) n3 += rec_radius(rc[r].y) == 3u;
        const uint32_t n_hi = flat_map ? nj : std::max(pass_n_hi(t.z), n3);
        const uint32_t n_chunks = chunk_map_count(n3, n_hi, nj);
        for (uint32_t c = 0; c < n_chunks; c++) {
            const ChunkRange cr = chunk_map_range(n3, n_hi, nj, c);
            uint32_t n_max = 0, radii = 0;
            uint64_t cols = 0;
            for (uint32_t r = cr.first; r < cr.end; r++) {
                const uint32_t N = rec_n(rc[r].y);
                n_max = std::max(n_max, N); cols += N; radii |= 1u << rec_radius(rc[r].y);
            }
            const uint32_t cls = cr.quad ? 0u : radii == 4u ? 1u : radii == 2u ? 3u : !(radii & ~6u) ? 2u : 4u;
            w[4 * cls] += cr.end - cr.first; w[4 * cls + 1]++; w[4 * cls + 2] += n_max; w[4 * cls + 3] += cols;
        }
        w[20]++;
    }
    return true;
}

} // namespace rawdtw
