// rawdtw_local.hip -- k_local_jobs: the job records of a local batch (include/rawdtw.h, "local border") whose anchor arrays are on the
// device.  A local chain is ONE semiglobal job over the window between its end anchors, so of a chain's anchors only the first and the
// last entry matter: one thread a chain reads those two, the chain's two bases, and writes the chain's 32-byte record in chain order.
// The host plans the launches' classes from the records (rawdtw_semiglobal.cpp): 32 bytes a chain come home instead of 8 bytes an anchor.
// Memory-bound and tiny: two scattered 8-byte loads a thread, everything else coalesced; the record goes out as two 16-byte stores.
#include "rawdtw_capi.h"

namespace rawdtw {
namespace {

static_assert(sizeof(rawdtw_job_t) == 32 && sizeof(rawdtw_anchor_t) == 8, "a job record is two 16-byte stores, an anchor one 8-byte load");

__global__ __launch_bounds__(256) void k_local_jobs(const uint64_t *__restrict__ anchor_off, const rawdtw_anchor_t *__restrict__ anchors,
                                                    const uint64_t *__restrict__ ref_base, const uint32_t *__restrict__ read_base,
                                                    uint64_t n_chains, uint4 *__restrict__ jobs_out)
{
    const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x; // (64-bit throughout: offsets, bases and the chain index)
    if (c >= n_chains) return;
    const uint64_t a0 = anchor_off[c], a1 = anchor_off[c + 1];
    uint64_t ref_off = 0;
    uint32_t read_off = 0, n = 0, m = 0;
    if (a1 > a0) { // (an empty chain: n = m = 0, no anchor is read)
        const rawdtw_anchor_t s = anchors[a1 - 1], e = anchors[a0]; // end-first: the chain's start is its list's last entry
        ref_off = ref_base[c] + (uint64_t)s.target_position;
        read_off = read_base[c] + s.query_position;            // uint32, as rawdtw_chain_build_jobs
        m = e.target_position - s.target_position + 1u;
        n = e.query_position - s.query_position + 1u;
    }
    // rawdtw_job_t: {ref_off, read_off, n} {m, band_radius = RAWDTW_FULL, exclude_last = 0, reserved = 0}
    jobs_out[2 * c] = make_uint4((uint32_t)ref_off, (uint32_t)(ref_off >> 32), read_off, n);
    jobs_out[2 * c + 1] = make_uint4(m, (uint32_t)RAWDTW_FULL, 0u, 0u);
}

} // namespace

namespace capi {
hipError_t launch_local_jobs(const uint64_t *anchor_off, const rawdtw_anchor_t *anchors, const uint64_t *ref_base, const uint32_t *read_base,
                             uint64_t n_chains, rawdtw_job_t *jobs_out, hipStream_t s)
{
    if (n_chains == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_local_jobs, dim3((uint32_t)((n_chains + 255) / 256)), dim3(256), 0, s, anchor_off, anchors, ref_base, read_base, n_chains,
                       reinterpret_cast<uint4 *>(jobs_out));
    return hipGetLastError();
}
} // namespace capi
} // namespace rawdtw
