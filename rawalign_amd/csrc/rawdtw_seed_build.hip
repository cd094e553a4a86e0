// rawdtw_seed_build.hip -- the seed index of ri_idx_add / ri_idx_sort (src/rawindex.cpp:91-97, 194-246) built from the context's reference
// arena on the device: equal to what rawdtw_seed_index_build (rawdtw_seed_host.cpp) makes from the same arrays -- for w = 0 by
// rawdtw_seed_index_build_device, for any w by rawdtw_seed_index_build_device_min.
//
//   k_sb_filter   rsketch.c:242-247, the kept-event recurrence: serial a strand, so a wave a (sequence, strand).  64 events a step come
//                 in with one load; the recurrence runs over them out of scalar registers (v_readlane), alike in every lane; lane t then
//                 writes event t's position and code at its rank among the kept ones.
//   k_sb_emit     a thread a kept event with e - 1 kept events in front of it: the packed codes' hash32 and
//                 y = seq << 32 | pos << 1 | strand (rsketch.c:253; forward carries strand bit 1, rawindex.cpp:141-147).
//   w > 0         instead of k_sb_emit: k_sb_hash (a thread an e-mer: its hash), k_sb_min_count (a workgroup a tile of 256 e-mers of a
//                 strand, the hashes m0 - w .. m0 + 255 in LDS, a thread a step of rawdtw_seed_min.h, a count a tile), rocPRIM's exclusive
//                 scan of the tile counts (the total comes home and sizes the entries), k_sb_min_write (the same tiling; the elements at
//                 the tile's offset plus an in-block scan, y from the e-mer's FIRST kept event).  The filter runs without the mask test.
//   the sort      rocPRIM's device radix sort, twice: stable by y, then stable by hash -- the order of by_hash_then_position.
//   home          the sorted entries come home and fill_table (rawdtw_seed_host.cpp) builds the slots, as for every other index.
// skipped, code_of and hash32 are rawdtw_seed.h's: one definition.
//
// The device block: per strand a row (below); per event of the arena a kept position and a kept code (4 bytes each); per entry a hash
// and a y, twice over for the sort's double buffer, and rocPRIM's temporary storage.  w > 0 adds a hash per event of the arena (4 bytes),
// a count and an offset a tile (8 bytes each), the scan's temporary storage and the word the write counts in.
#include "rawdtw_capi.h"
#include "rawdtw_seed.h"
#include "rawdtw_seed_min.h"

#include <algorithm>
#include <chrono>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace rawdtw {
namespace {

using namespace seed;

struct StrandRow {
    uint64_t arena_off; // where the strand starts in the arena
    uint64_t kept_base; // ... in the kept arrays
    uint64_t entry_base; // ... in the entries (filled behind the filter)
    uint32_t len, kept;
};

// kMask: the w == 0 rule (rsketch.c:243); without it ri_sketch_min's (rsketch.c:172), which keeps a masked value -- as k_seed_filter's.
template <bool kMask>
__global__ __launch_bounds__(64) void k_sb_filter(const float *__restrict__ arena, StrandRow *__restrict__ rows, uint32_t q, uint32_t lq,
                                                  uint32_t *__restrict__ kept_pos, uint32_t *__restrict__ kept_code)
{
    const uint32_t pair = blockIdx.x, lane = threadIdx.x;
    const StrandRow row = rows[pair];
    const float *s = arena + row.arena_off;
    const uint32_t n = row.len;
    uint32_t kept = 0;
    float last = n ? s[0] : 0.0f; // (s[last] with last = 0, as rsketch.c starts)
    float x_next = n ? (lane < n ? s[lane] : 0.0f) : 0.0f; // (a step's load is under way while the step before it runs)
    for (uint64_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t c = (uint32_t)(n - i0 < 64 ? n - i0 : 64);
        const float x = x_next;
        x_next = i0 + 64 + lane < n ? s[i0 + 64 + lane] : 0.0f;
        const int xb = __float_as_int(x);
        uint64_t mask = 0;
#pragma unroll
        for (uint32_t t = 0; t < 64; t++) {
            const float xt = __int_as_float(__builtin_amdgcn_readlane(xb, t));
            const bool skip = kMask ? skipped(xt, last, i0 + t == 0) : skipped_min(xt, last, i0 + t == 0);
            if (t < c && !skip) { last = xt; mask |= 1ull << t; }
        }
        if (mask >> lane & 1) {
            const uint64_t at = row.kept_base + kept + __popcll(mask & ((1ull << lane) - 1));
            kept_pos[at] = (uint32_t)(i0 + lane);
            kept_code[at] = code_of((uint32_t)xb, q, lq);
        }
        kept += __popcll(mask);
    }
    if (lane == 0) rows[pair].kept = kept;
}

__global__ __launch_bounds__(256) void k_sb_emit(const StrandRow *__restrict__ rows, const uint32_t *__restrict__ kept_pos,
                                                 const uint32_t *__restrict__ kept_code, uint32_t e, uint32_t quant_bit,
                                                 uint32_t *__restrict__ hash_out, uint64_t *__restrict__ y_out)
{
    const uint32_t pair = blockIdx.x;
    const StrandRow row = rows[pair];
    const uint32_t n = row.kept >= e ? row.kept - e + 1 : 0, strand = (pair & 1) ? 0u : 1u;
    const uint64_t mask_events = (1ULL << (quant_bit * e)) - 1, seq = pair >> 1;
    for (uint64_t t = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.y * blockDim.x) {
        uint64_t quant = 0;
        for (uint32_t a = 0; a < e; a++) quant = quant << quant_bit | kept_code[row.kept_base + t + a];
        quant &= mask_events;
        const uint32_t i = kept_pos[row.kept_base + t + e - 1];
        hash_out[row.entry_base + t] = hash32((uint32_t)quant);
        y_out[row.entry_base + t] = seq << 32 | (uint32_t)(i << 1) | strand;
    }
}

// ---- w > 0: the minimizer windows over whole strands.  rawdtw_seed_min.h's step makes every e-mer's elements a function of the hashes
// m - w .. m alone, so the selection is a count, a scan and a write with no serial part.  In these launches a row's entry_base is the
// strand's first tile among all strands' tiles.
constexpr uint32_t kMinTile = 256;                // e-mers a workgroup takes at a time; also the block size
constexpr uint32_t kMinStage = kMinTile + 256;    // the tile's hashes and the w <= 255 in front of them

__global__ __launch_bounds__(256) void k_sb_hash(const StrandRow *__restrict__ rows, const uint32_t *__restrict__ kept_code, uint32_t e,
                                                 uint32_t quant_bit, uint32_t *__restrict__ h_out)
{
    const StrandRow row = rows[blockIdx.x];
    const uint32_t n = row.kept >= e ? row.kept - e + 1 : 0;
    const uint64_t mask_events = (1ULL << (quant_bit * e)) - 1;
    for (uint64_t t = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.y * blockDim.x) {
        uint64_t quant = 0;
        for (uint32_t a = 0; a < e; a++) quant = quant << quant_bit | kept_code[row.kept_base + t + a];
        h_out[row.kept_base + t] = hash32((uint32_t)(quant & mask_events)); // (an array of its own: e-mer t reads codes t .. t + e - 1)
    }
}

// the hashes max(0, m0 - w) .. min(m0 + kMinTile, M) - 1 of a strand into LDS; returns the e-mer that sh[0] belongs to
__device__ inline uint32_t min_stage(const uint32_t *__restrict__ h, uint32_t M, uint32_t m0, uint32_t w, uint32_t *sh)
{
    const uint32_t base = m0 >= w ? m0 - w : 0, end = M - m0 < kMinTile ? M : m0 + kMinTile;
    for (uint32_t i = base + threadIdx.x; i < end; i += kMinTile) sh[i - base] = h[i];
    return base;
}

// the sum of v over the block's 256 threads, in every thread (part: 4 words of LDS; a barrier on either side)
__device__ inline uint32_t block_sum(uint32_t v, uint32_t *part)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void k_sb_min_count(const StrandRow *__restrict__ rows, const uint32_t *__restrict__ h, uint32_t e, uint32_t w,
                                                      uint64_t *__restrict__ tile_count)
{
    __shared__ uint32_t sh[kMinStage], part[4];
    const StrandRow row = rows[blockIdx.x];
    const uint32_t M = row.kept >= e ? row.kept - e + 1 : 0, tiles = (M + kMinTile - 1) / kMinTile;
    for (uint32_t t = blockIdx.y; t < tiles; t += gridDim.y) {
        const uint32_t m0 = t * kMinTile, m = m0 + threadIdx.x;
        const uint32_t base = min_stage(h + row.kept_base, M, m0, w, sh);
        __syncthreads();
        const uint32_t c = m < M ? min_step_count(sh, base, m, M, w) : 0; // (the strand's last e-mer: the end's one is in its count)
        const uint32_t sum = block_sum(c, part);
        if (threadIdx.x == 0) tile_count[row.entry_base + t] = sum;
        __syncthreads(); // (the next tile's staging writes sh and part)
    }
}

__global__ __launch_bounds__(256) void k_sb_min_write(const StrandRow *__restrict__ rows, const uint32_t *__restrict__ h,
                                                      const uint32_t *__restrict__ kept_pos, uint32_t e, uint32_t w,
                                                      const uint64_t *__restrict__ tile_off, uint64_t n_entries, uint32_t *__restrict__ hash_out,
                                                      uint64_t *__restrict__ y_out, unsigned long long *__restrict__ written)
{
    __shared__ uint32_t sh[kMinStage], scan[kMinTile], part[4];
    const uint32_t pair = blockIdx.x, strand = (pair & 1) ? 0u : 1u;
    const StrandRow row = rows[pair];
    const uint32_t M = row.kept >= e ? row.kept - e + 1 : 0, tiles = (M + kMinTile - 1) / kMinTile;
    const uint64_t seq = pair >> 1;
    uint32_t done = 0;
    for (uint32_t t = blockIdx.y; t < tiles; t += gridDim.y) {
        const uint32_t m0 = t * kMinTile, m = m0 + threadIdx.x;
        const uint32_t base = min_stage(h + row.kept_base, M, m0, w, sh);
        __syncthreads();
        const uint32_t c = m < M ? min_step_count(sh, base, m, M, w) : 0;
        scan[threadIdx.x] = c; // the thread's place: an inclusive scan of the counts, less its own
        __syncthreads();
        for (uint32_t d = 1; d < kMinTile; d <<= 1) {
            const uint32_t v = threadIdx.x >= d ? scan[threadIdx.x - d] : 0;
            __syncthreads();
            scan[threadIdx.x] += v;
            __syncthreads();
        }
        uint64_t at = tile_off[row.entry_base + t] + (scan[threadIdx.x] - c);
        if (c)
            min_step_walk(MinHashes{sh, base}, m, M, w, [&](uint32_t i) {
                if (at < n_entries) { // (the scan's total sized the arrays: a place past them would be a fault of this file, told by `written`)
                    hash_out[at] = sh[i - base];
                    y_out[at] = seq << 32 | (uint32_t)(kept_pos[row.kept_base + i] << 1) | strand;
                    done++;
                }
                at++;
            });
        __syncthreads(); // (the next tile's staging writes sh and scan)
    }
    const uint32_t sum = block_sum(done, part);
    if (threadIdx.x == 0 && sum) atomicAdd(written, (unsigned long long)sum);
}

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

} // namespace
} // namespace rawdtw

using namespace rawdtw;
using namespace rawdtw::capi;
using namespace rawdtw::seed;

// Both entries: the checks, the filter, then the entries -- k_sb_emit for w == 0, the hash / count / scan / write launches for w > 0
// (min_ok: the entry takes them) -- the two sorts, the entries' way home and fill_table.
static int build_device(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out, bool min_ok)
{
    if (!ctx || !out) return RAWDTW_ERR_INVALID;
    *out = nullptr;
    if (check_pars(pars) != RAWDTW_OK) return fail(ctx, RAWDTW_ERR_INVALID, "bad seed parameters");
    if (!ctx->d_ref || 2 * ctx->ref_len.size() != ctx->ref_off.size() || (ctx->ref_len.empty() && !ctx->ref_hold))
        return fail(ctx, RAWDTW_ERR_INVALID, "the context holds no reference with a sequence table");
    if (pars->w > 0 && !min_ok) return fail(ctx, RAWDTW_ERR_UNSUPPORTED, "w > 0: minimizer windows over whole strands are built on the host");
    const bool windowed = pars->w > 0;
    const uint32_t n_seq = (uint32_t)ctx->ref_len.size();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<StrandRow> rows;
    uint64_t total_len = 0, max_len = 0;
    try { rows.resize(2ull * n_seq); } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    for (uint32_t s = 0; s < n_seq; s++)
        for (int slot = 0; slot < 2; slot++) { // slot 0: forward (strand 1)
            rows[2 * s + slot] = StrandRow{ctx->ref_off[2 * s + slot], total_len, 0, ctx->ref_len[s], 0};
            total_len += ctx->ref_len[s];
            max_len = std::max<uint64_t>(max_len, ctx->ref_len[s]);
        }
    rawdtw_seed_index *six = new (std::nothrow) rawdtw_seed_index;
    if (!six) return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    six->pars = *pars; six->n_seq = n_seq; six->serial = next_serial();
    StrandRow *d_rows = nullptr;
    uint32_t *d_kpos = nullptr, *d_kcode = nullptr, *d_hash[2] = {nullptr, nullptr};
    uint64_t *d_y[2] = {nullptr, nullptr};
    void *d_tmp = nullptr;
    // w > 0: the e-mers' hashes, a count a tile (and a 0 behind the last), their exclusive scan (the total behind the last), the word
    // k_sb_min_write counts its elements in, the scan's temporary storage
    uint32_t *d_h = nullptr;
    uint64_t *d_cnt = nullptr, *d_off = nullptr;
    unsigned long long *d_written = nullptr;
    void *d_scan_tmp = nullptr;
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // filter | emit | sort; w > 0: hash | count + scan, write
    float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, min_ms[3] = {0.f, 0.f, 0.f};
    int st = RAWDTW_OK;
    std::vector<uint32_t> h_hash;
    std::vector<uint64_t> h_y;
    std::vector<Entry> all;
    uint64_t N = 0, emers = 0;
    hipError_t e = hipSuccess;
    auto hip_ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
    size_t tmp_a = 0, tmp_b = 0;
    uint32_t seq_bits = 0;
    while (seq_bits < 32 && (1ull << seq_bits) < n_seq) seq_bits++;
    // the entry arrays for N entries, twice over, and the sorts' temporary storage
    auto sort_arrays = [&]() {
        for (int i = 0; i < 2; i++) { hip_ok(hipMalloc((void **)&d_hash[i], N * 4)); hip_ok(hipMalloc((void **)&d_y[i], N * 8)); }
        if (e == hipSuccess) hip_ok(rocprim::radix_sort_pairs(nullptr, tmp_a, d_y[0], d_y[1], d_hash[0], d_hash[1], (size_t)N, 0u, 32u + seq_bits, ctx->stream));
        if (e == hipSuccess) hip_ok(rocprim::radix_sort_pairs(nullptr, tmp_b, d_hash[1], d_hash[0], d_y[1], d_y[0], (size_t)N, 0u, 32u, ctx->stream));
        if (e == hipSuccess) hip_ok(hipMalloc(&d_tmp, std::max<size_t>(std::max(tmp_a, tmp_b), 16)));
    };
    // the entries in d_hash[0] / d_y[0]: stable by y, then stable by hash, then home (from: the event at the sorts' start, done: at their end)
    auto sort_and_home = [&](hipEvent_t from, hipEvent_t done) {
        if (e == hipSuccess) hip_ok(rocprim::radix_sort_pairs(d_tmp, tmp_a, d_y[0], d_y[1], d_hash[0], d_hash[1], (size_t)N, 0u, 32u + seq_bits, ctx->stream));
        if (e == hipSuccess) hip_ok(rocprim::radix_sort_pairs(d_tmp, tmp_b, d_hash[1], d_hash[0], d_y[1], d_y[0], (size_t)N, 0u, 32u, ctx->stream));
        if (e == hipSuccess) hip_ok(hipEventRecord(done, ctx->stream));
        if (e == hipSuccess) hip_ok(hipEventSynchronize(done));
        const double t0 = now_ms();
        try { h_hash.resize(N); h_y.resize(N); } catch (const std::bad_alloc &) { st = RAWDTW_ERR_OOM; }
        if (st == RAWDTW_OK && e == hipSuccess) {
            hip_ok(hipMemcpyAsync(h_hash.data(), d_hash[0], N * 4, hipMemcpyDeviceToHost, ctx->stream));
            hip_ok(hipMemcpyAsync(h_y.data(), d_y[0], N * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        hip_ok(hipStreamSynchronize(ctx->stream));
        if (e == hipSuccess && st == RAWDTW_OK) {
            (void)hipEventElapsedTime(&ms[2], from, done);
            ms[3] = (float)(now_ms() - t0);
        }
    };
    for (int i = 0; i < 8; i++) hip_ok(hipEventCreate(&ev[i]));
    if (n_seq && total_len) {
        hip_ok(hipMalloc((void **)&d_rows, rows.size() * sizeof(StrandRow)));
        hip_ok(hipMalloc((void **)&d_kpos, total_len * 4));
        hip_ok(hipMalloc((void **)&d_kcode, total_len * 4));
        if (e == hipSuccess) hip_ok(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(StrandRow), hipMemcpyHostToDevice, ctx->stream));
        if (e == hipSuccess) hip_ok(hipEventRecord(ev[0], ctx->stream));
        if (e == hipSuccess) {
            if (windowed) hipLaunchKernelGGL(k_sb_filter<false>, dim3(2 * n_seq), dim3(64), 0, ctx->stream, ctx->d_ref, d_rows, pars->q, pars->lq, d_kpos, d_kcode);
            else hipLaunchKernelGGL(k_sb_filter<true>, dim3(2 * n_seq), dim3(64), 0, ctx->stream, ctx->d_ref, d_rows, pars->q, pars->lq, d_kpos, d_kcode);
            hip_ok(hipGetLastError());
        }
        if (e == hipSuccess) hip_ok(hipEventRecord(ev[1], ctx->stream));
        if (e == hipSuccess) hip_ok(hipMemcpyAsync(rows.data(), d_rows, rows.size() * sizeof(StrandRow), hipMemcpyDeviceToHost, ctx->stream));
        if (e == hipSuccess) hip_ok(hipStreamSynchronize(ctx->stream));
        if (e == hipSuccess && !windowed) {
            uint64_t max_n = 0;
            for (StrandRow &r : rows) {
                r.entry_base = N;
                const uint64_t n = r.kept >= pars->e ? r.kept - pars->e + 1 : 0;
                N += n; max_n = std::max(max_n, n);
            }
            if (N) {
                sort_arrays();
                if (e == hipSuccess) hip_ok(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(StrandRow), hipMemcpyHostToDevice, ctx->stream));
                if (e == hipSuccess) hip_ok(hipEventRecord(ev[2], ctx->stream));
                if (e == hipSuccess) {
                    const uint32_t gy = (uint32_t)std::min<uint64_t>((max_n + 255) / 256, 1024);
                    hipLaunchKernelGGL(k_sb_emit, dim3(2 * n_seq, gy), dim3(256), 0, ctx->stream, d_rows, d_kpos, d_kcode, pars->e, pars->lq + 2, d_hash[0],
                                       d_y[0]);
                    hip_ok(hipGetLastError());
                }
                if (e == hipSuccess) hip_ok(hipEventRecord(ev[3], ctx->stream));
                sort_and_home(ev[3], ev[4]);
                if (e == hipSuccess && st == RAWDTW_OK) (void)hipEventElapsedTime(&ms[1], ev[2], ev[3]);
            }
        }
        if (e == hipSuccess && windowed) {
            uint64_t n_tiles = 0, max_tiles = 0;
            for (StrandRow &r : rows) {
                r.entry_base = n_tiles; // (the strand's first tile)
                const uint64_t n = r.kept >= pars->e ? r.kept - pars->e + 1 : 0, tiles = (n + kMinTile - 1) / kMinTile;
                emers += n; n_tiles += tiles; max_tiles = std::max(max_tiles, tiles);
            }
            if (n_tiles) {
                size_t scan_bytes = 0;
                const uint32_t gy = (uint32_t)std::min<uint64_t>(max_tiles, 1024); // (a hash launch's blocks take kMinTile e-mers at a time too)
                hip_ok(hipMalloc((void **)&d_h, total_len * 4));
                hip_ok(hipMalloc((void **)&d_cnt, (n_tiles + 1) * 8));
                hip_ok(hipMalloc((void **)&d_off, (n_tiles + 1) * 8));
                hip_ok(hipMalloc((void **)&d_written, 8));
                if (e == hipSuccess) hip_ok(rocprim::exclusive_scan(nullptr, scan_bytes, d_cnt, d_off, (uint64_t)0, (size_t)(n_tiles + 1), rocprim::plus<uint64_t>(), ctx->stream));
                if (e == hipSuccess) hip_ok(hipMalloc(&d_scan_tmp, std::max<size_t>(scan_bytes, 16)));
                if (e == hipSuccess) hip_ok(hipMemsetAsync(d_cnt + n_tiles, 0, 8, ctx->stream));
                if (e == hipSuccess) hip_ok(hipMemsetAsync(d_written, 0, 8, ctx->stream));
                if (e == hipSuccess) hip_ok(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(StrandRow), hipMemcpyHostToDevice, ctx->stream));
                if (e == hipSuccess) hip_ok(hipEventRecord(ev[2], ctx->stream));
                if (e == hipSuccess) {
                    hipLaunchKernelGGL(k_sb_hash, dim3(2 * n_seq, gy), dim3(256), 0, ctx->stream, d_rows, d_kcode, pars->e, pars->lq + 2, d_h);
                    hip_ok(hipGetLastError());
                }
                if (e == hipSuccess) hip_ok(hipEventRecord(ev[3], ctx->stream));
                if (e == hipSuccess) {
                    hipLaunchKernelGGL(k_sb_min_count, dim3(2 * n_seq, gy), dim3(kMinTile), 0, ctx->stream, d_rows, d_h, pars->e, pars->w, d_cnt);
                    hip_ok(hipGetLastError());
                }
                if (e == hipSuccess) hip_ok(rocprim::exclusive_scan(d_scan_tmp, scan_bytes, d_cnt, d_off, (uint64_t)0, (size_t)(n_tiles + 1), rocprim::plus<uint64_t>(), ctx->stream));
                if (e == hipSuccess) hip_ok(hipEventRecord(ev[4], ctx->stream));
                // the total comes home and sizes the entry arrays exactly (no cap: more entries than e-mers is legal)
                if (e == hipSuccess) hip_ok(hipMemcpyAsync(&N, d_off + n_tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
                if (e == hipSuccess) hip_ok(hipStreamSynchronize(ctx->stream));
                if (e != hipSuccess) N = 0;
                if (N) {
                    unsigned long long written = 0;
                    sort_arrays();
                    if (e == hipSuccess) hip_ok(hipEventRecord(ev[5], ctx->stream));
                    if (e == hipSuccess) {
                        hipLaunchKernelGGL(k_sb_min_write, dim3(2 * n_seq, gy), dim3(kMinTile), 0, ctx->stream, d_rows, d_h, d_kpos, pars->e, pars->w, d_off, N,
                                           d_hash[0], d_y[0], d_written);
                        hip_ok(hipGetLastError());
                    }
                    if (e == hipSuccess) hip_ok(hipEventRecord(ev[6], ctx->stream));
                    if (e == hipSuccess) hip_ok(hipMemcpyAsync(&written, d_written, 8, hipMemcpyDeviceToHost, ctx->stream));
                    sort_and_home(ev[6], ev[7]);
                    if (e == hipSuccess && st == RAWDTW_OK) {
                        (void)hipEventElapsedTime(&min_ms[0], ev[2], ev[3]);
                        (void)hipEventElapsedTime(&min_ms[1], ev[3], ev[4]);
                        (void)hipEventElapsedTime(&min_ms[2], ev[5], ev[6]);
                        ms[1] = min_ms[0] + min_ms[1] + min_ms[2];
                        if (written != N) st = RAWDTW_ERR_INTERNAL; // the write did not put down what the count counted: no table
                    }
                }
            }
        }
        if (e == hipSuccess) (void)hipEventElapsedTime(&ms[0], ev[0], ev[1]);
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < 8; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
    for (int i = 0; i < 2; i++) { if (d_hash[i]) (void)hipFree(d_hash[i]); if (d_y[i]) (void)hipFree(d_y[i]); }
    if (d_tmp) (void)hipFree(d_tmp);
    if (d_scan_tmp) (void)hipFree(d_scan_tmp);
    if (d_written) (void)hipFree(d_written);
    if (d_off) (void)hipFree(d_off);
    if (d_cnt) (void)hipFree(d_cnt);
    if (d_h) (void)hipFree(d_h);
    if (d_kpos) (void)hipFree(d_kpos);
    if (d_kcode) (void)hipFree(d_kcode);
    if (d_rows) (void)hipFree(d_rows);
    if (e != hipSuccess) { delete six; return hip_fail(ctx, e, windowed ? "rawdtw_seed_index_build_device_min" : "rawdtw_seed_index_build_device"); }
    if (st == RAWDTW_ERR_INTERNAL) { delete six; return fail(ctx, st, "the write launch's element count is not the scan's total"); }
    const double t1 = now_ms();
    if (st == RAWDTW_OK) {
        try {
            all.resize(N);
            for (uint64_t i = 0; i < N; i++) all[i] = Entry{h_hash[i], h_y[i]};
            std::vector<uint32_t>().swap(h_hash);
            std::vector<uint64_t>().swap(h_y);
        } catch (const std::bad_alloc &) { st = RAWDTW_ERR_OOM; }
    }
    if (st == RAWDTW_OK) st = fill_table(six, all);
    ms[4] = (float)(now_ms() - t1);
    if (st != RAWDTW_OK) { delete six; return fail(ctx, st, "building the table failed"); }
    memcpy(ctx->seed_build_ms, ms, sizeof(ms));
    if (windowed) {
        ctx->seed_min_emers = emers; ctx->seed_min_entries = N;
        memcpy(ctx->seed_min_ms, min_ms, sizeof(min_ms));
    }
    *out = six;
    return RAWDTW_OK;
}

extern "C" {

int rawdtw_seed_index_build_device(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out)
{
    return build_device(ctx, pars, out, false);
}

int rawdtw_seed_index_build_device_min(rawdtw_ctx *ctx, const rawdtw_seed_pars_t *pars, rawdtw_seed_index **out)
{
    return build_device(ctx, pars, out, true);
}

int rawdtw_seed_index_build_min_stats(const rawdtw_ctx *ctx, uint64_t *emers, uint64_t *entries, float select_ms[3])
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (emers) *emers = ctx->seed_min_emers;
    if (entries) *entries = ctx->seed_min_entries;
    if (select_ms) memcpy(select_ms, ctx->seed_min_ms, sizeof(ctx->seed_min_ms));
    return RAWDTW_OK;
}

int rawdtw_seed_index_build_stats(const rawdtw_ctx *ctx, float phase_ms[5])
{
    if (!ctx || !phase_ms) return RAWDTW_ERR_INVALID;
    memcpy(phase_ms, ctx->seed_build_ms, sizeof(ctx->seed_build_ms));
    return RAWDTW_OK;
}

} // extern "C"
