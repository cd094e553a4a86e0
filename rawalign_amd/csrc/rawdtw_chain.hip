// rawdtw_chain.hip -- the anchor sort and the chaining DP of gen_chains on the device: what bounds the chunk-round
// mapper once the DTW block is on the GPU (rawdtw_mapper.cpp: 8 us a read and host thread, 60 % of a round on 16 threads).
//
//   src/rmap.cpp:396-401   every (sequence, strand) list of anchors sorted by (target, query)
//   src/rmap.cpp:430-507   the chaining DP: per anchor the best predecessor inside the band, the skip counter, the running maximum, the end
//                          candidates (score filter), the num_best_chains best ends
//   src/rmap.cpp:130-173   traceback_chains: predecessor walk with the `used` marks, the score of a chain that runs into a used anchor
//   src/rmap.cpp:512       the evaluation order: chaining score, descending
// as restated on the host by rawdtw_chain_anchors / rawdtw_sort_by_chaining_score (rawdtw_host.cpp), which the tests compare this with,
// chain by chain and bit for bit.
//
// A WAVE A READ.  The read's seeds (the previous chains' anchors and the chunk's hits, unsorted, as the caller has them) go into LDS and are
// sorted there (bitonic, key = (sequence * 2 + strand, target, query): equal seeds are indistinguishable, so any sort gives the array the
// reference's std::sort gives).  The DP runs anchor by anchor -- that order is the algorithm's -- with the predecessor loop of an anchor, the
// part that is long, taken 64 candidates at a time: whether a candidate is passed over, ends the loop or competes, and with which value,
// depends on the anchors and on scores that are final; what is sequential in the source -- `best` only ever grows, the skip counter moves
// by one a competing candidate, the loop ends at the first candidate past max_num_skips -- is a prefix maximum and a prefix sum over the
// lanes, and the loop's exit is the first lane whose prefix says so.  Ends, traceback and order are short and run on one lane.
// Results: per read its chains in evaluation order (records + anchors, end-first); a scan and a compaction launch lay all reads' chains out
// as ONE candidate batch in device memory -- chain_off / anchor_off / anchors / ref_base / read_base, exactly what rawdtw_batch_submit
// takes -- so the anchors never cross PCIe on their way into the DTW.
//
// What the device declines (the caller chains that round on the host, same results): a read with more seeds than the wave's piece of LDS
// holds (2 048), more than 32 chains, or more than 16 chains with two equal scores among them (std::sort's order of equal elements is its
// own beyond 16; up to 16 it is an insertion sort and stable).  With "chain_decline_reads" on it declines such a read alone and chains the
// rest of the round (DECLINING A READ, at k_chain_scan).
//
// THE LONG PATH ("chain_long_seeds", off by default).  A read above the wave's piece of LDS is chained with its state in device memory: a
// workgroup sorts its seeds into scratch (k_chain_sort_long), then a wave runs the same DP over them (k_chain_long) with the trailing window of
// candidates in an LDS ring and everything older read back from scratch.  Same results, same flags; with the option on only a read above the
// option's value still declines the round.
//
// MANY CHAINS A READ ("chain_max_chains" = N, off by default).  The two limits on chains are those of the order: 32 records in LDS, and an insertion
// sort that is std::sort only up to 16 elements.  With the option on the kernels run as k_chain<true> / k_chain_long<true>: a read's records go
// to its stretch of the round's workspace as they are generated, their scores to LDS, and the order is std::sort's own algorithm restated
// (rawdtw_sort_order.h) over a permutation that k_chain_compact reads the records through.  Only a read with more than N chains still
// declines the round.  The <false> instantiations are the kernels as they were.
//
// ONE DP BODY.  What restates the reference is written once, as inlined device functions both kernels call: list_end (where a list ends),
// chain_step (64 candidates of the predecessor loop, rmap.cpp:458-484), chain_ends (the best ends and traceback_chains, rmap.cpp:175-179, 130-173,
// 502-504) and chain_order (rmap.cpp:512, the tie flag, the read's records and counts).  A kernel supplies where the state lives: k_chain loads a
// candidate's (target, query, score) from LDS and writes an anchor's score, predecessor and flags there; k_chain_long loads them from its ring or
// from scratch behind it (counting the far steps), keeps a block's state in registers, flushes it to scratch, and asks chain_ends for the fences
// that marks in device memory need.  The anchor loop, the band's lower end, the running maximum and the end filter (rmap.cpp:486-493) stay in the
// kernels.  The round's workspace is described once too (ChainLayout): laid from 0 it gives the size, from the block's base the pointers.
#include "rawdtw_capi.h"
#include "rawdtw_chain_append.h"
#include "rawdtw_sort_order.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace rawdtw {
namespace {

constexpr uint32_t kChainMaxSeeds = 2048; // a read's seeds in LDS: 21 bytes each
constexpr uint32_t kChainCap = 32;        // chains a read
constexpr uint32_t kChainStable = 16;     // std::sort is an insertion sort up to here (libstdc++'s _S_threshold)

struct ChainRecDev { float score; uint32_t key, start, end, n, a_off; };
struct ChainCnt { uint32_t nc, na, flags, pad; };

struct ChainArgs {
    const uint64_t *seed_off;
    const rawdtw_seed_t *seeds;
    uint32_t n_reads, n2;
    rawdtw_chain_opt_t opt;
    rawdtw_anchor_t *tmp_anchors; // read r's chains, as generated: [seed_off[r], seed_off[r + 1])
    ChainRecDev *tmp_recs;        // [r * kChainCap ..): in evaluation order
    ChainCnt *cnt;
    // many chains a read ("chain_max_chains"; MANY CHAINS A READ below).  Off: cap = kChainCap, the rest 0.
    uint32_t cap;        // chains a read the round records
    uint32_t rec_div;    // max(1, min_num_anchors): a read of n seeds has at most n / rec_div chains
    uint32_t by_seeds;   // read r's records start at seed_off[r] / rec_div (0: at r * cap)
    uint32_t lds_chains; // k_chain's LDS behind the seeds holds the scores and the order of this many chains
    uint32_t *tmp_perm;  // the evaluation order: a permutation of the read's records, which stay in tmp_recs as generated
};
// where read r's records start in tmp_recs (and its order in tmp_perm)
__device__ __forceinline__ uint64_t rec_start(const ChainArgs &a, const uint32_t r) { return a.by_seeds ? a.seed_off[r] / a.rec_div : (uint64_t)r * a.cap; }

__device__ __forceinline__ void lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// inclusive scans over the wave in lane order (rows of 16 by row_shr, then the rows' last lanes into the rows behind them)
__device__ __forceinline__ int scan_add(int x)
{
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
    return x;
}
// (values are >= -1: as floats; a lane without a source takes -1)
__device__ __forceinline__ float scan_max(float v)
{
    const int neg = __builtin_bit_cast(int, -1.0f);
#define RAWDTW_SM(ctrl, rm) v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(neg, __builtin_bit_cast(int, v), ctrl, rm, 0xf, false)))
    RAWDTW_SM(0x111, 0xf); RAWDTW_SM(0x112, 0xf); RAWDTW_SM(0x114, 0xf); RAWDTW_SM(0x118, 0xf); RAWDTW_SM(0x142, 0xa); RAWDTW_SM(0x143, 0xc);
#undef RAWDTW_SM
    return v;
}
__device__ __forceinline__ uint32_t uni(const uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint32_t lane_of(const uint32_t x, const uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)uni(l)); }

// ---- what k_chain and k_chain_long share: rmap.cpp:430-507, 130-173 and 512 on a wave.  The arrays come as plain pointers -- LDS from k_chain,
// scratch from k_chain_long -- and every function is inlined into its kernel, where the compiler sees which of the two they are. ----
// the (sequence, strand) list of `key` that starts at g0: the first index whose key differs
__device__ __forceinline__ uint32_t list_end(const unsigned long long *K1, const uint32_t key, const uint32_t g0, const uint32_t n, const uint32_t lane)
{
    for (uint32_t i = g0; i < n; i += 64) {
        const uint32_t x = i + lane;
        const unsigned long long diff = __ballot(x < n && (uint32_t)(K1[x < n ? x : g0] >> 32) != key);
        if (diff) return i + (uint32_t)__builtin_ctzll(diff);
    }
    return n;
}
// 64 candidates of the predecessor loop of the anchor (ct, cq): lane l has candidate base - l, inside the band when `valid`, with its target, query
// and final score (pt, pq, sp) as the kernel loaded them from where it keeps them.  true: the loop ends among these.
__device__ __forceinline__ bool chain_step(const rawdtw_chain_opt_t &o, const int32_t ct, const int32_t cq, const int32_t base, const bool valid, const int32_t pt,
                                           const int32_t pq, const float sp, float &best, uint32_t &pred, int32_t &skips)
{
    const bool pass12 = pq == cq || pt == ct;                                   // rmap.cpp:458-459
    const bool stop_gap = valid && !pass12 && pt + o.max_target_gap_length < ct; // rmap.cpp:460
    const int32_t td = ct - pt, qd = cq - pq;
    const bool active = valid && !pass12 && !stop_gap && qd >= 0;               // rmap.cpp:467
    float cur = 0.0f;
    {
        const float matching = (float)min(min(td, qd), o.e);                    // rmap.cpp:469
        const int gap = abs(td - qd);
        const float scale = td > 0 ? __fdiv_rn((float)qd, (float)td) : 1.0f;
        if (gap < o.max_gap_length && scale < 5.0f && scale > 0.75f) cur = sp + matching; // rmap.cpp:474-476
    }
    const float cv = active ? cur : -1.0f;
    // the candidates before this one, in loop order = lane order: their largest value, and `best` as it stood at the loop's entry
    const float incl = scan_max(cv);
    const float before = fmaxf(best, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, -1.0f), __builtin_bit_cast(int, incl), 0x138, 0xf, 0xf, false)));
    const bool improver = active && cur > before;                               // rmap.cpp:478
    const int32_t moves = scan_add(improver ? -1 : (active ? 1 : 0));
    const bool stop_skip = active && !improver && skips + moves > o.max_num_skips; // rmap.cpp:482-484
    const unsigned long long stop = __ballot(!valid || stop_gap || stop_skip);
    const uint32_t first = stop ? (uint32_t)__builtin_ctzll(stop) : 64u;
    const unsigned long long live = first >= 64u ? ~0ull : ((1ull << first) - 1ull);
    const unsigned long long imp = __ballot(improver) & live;
    if (imp) { // (the improvers' values ascend: the last one stands)
        const uint32_t last = 63u - (uint32_t)__builtin_clzll(imp);
        best = __builtin_bit_cast(float, lane_of(__builtin_bit_cast(uint32_t, cur), last));
        pred = (uint32_t)(base - (int32_t)last);
    }
    if (first > 0) skips += (int32_t)lane_of((uint32_t)moves, first - 1u);
    return first < 64u;
}
// The num_best_chains best ends of the list [g0, g1) (rmap.cpp:175-179: score descending, then index descending) with traceback_chains on lane 0:
// the chains' anchors to tmp_anchors behind the read's `na` so far, their records to s_rec[nc ..].  kScratch: the arrays are device memory --
// a release and an acquire at agent scope stand between lane 0's marks and the wave's next look.
// kMany: s_rec is the read's stretch of tmp_recs, `room` entries of it are the read's, and a chain's score goes to m_score as well, for chain_order_many.
template <bool kScratch, bool kMany> __device__ __forceinline__ void chain_ends(const ChainArgs &a, const unsigned long long *K1, const uint32_t *Q, const float *SC, const uint32_t *PR, unsigned char *FL,
                                           const uint32_t key, const uint32_t g0, const uint32_t g1, const uint64_t s0, const float maxs, const uint32_t lane,
                                           ChainRecDev *s_rec, uint32_t &nc, uint32_t &na, uint32_t &flags, float *m_score = nullptr, const uint32_t many_room = 0)
{
    const uint32_t room = kMany ? many_room : kChainCap;
    const rawdtw_chain_opt_t &o = a.opt;
    for (int k = 0; k < o.num_best_chains; k++) {
        unsigned long long top = 0;
        for (uint32_t i = g0 + lane; i < g1; i += 64)
            if ((FL[i] & 6) == 2) top = max(top, (1ull << 63) | ((unsigned long long)__builtin_bit_cast(uint32_t, SC[i]) << 32) | i); // (scores are positive: their bits ascend with them)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(top >> 32), d), lw = (uint32_t)__shfl_xor((int)(uint32_t)top, d);
            top = max(top, ((unsigned long long)hi << 32) | lw);
        }
        if (!(top >> 63)) break;
        const uint32_t end = (uint32_t)top;
        bool below = false;
        if (lane == 0) {
            FL[end] |= 4;
            if (!(FL[end] & 1)) {
                const uint64_t out0 = s0 + na;
                uint32_t cur = end, len = 1;
                bool stop_at_used = false;
                a.tmp_anchors[out0] = rawdtw_anchor_t{(uint32_t)K1[cur], Q[cur]};
                if (PR[cur] != cur && (FL[PR[cur]] & 1)) stop_at_used = true;
                FL[cur] |= 1;
                while (PR[cur] != cur && !(FL[PR[cur]] & 1)) {
                    cur = PR[cur];
                    a.tmp_anchors[out0 + len] = rawdtw_anchor_t{(uint32_t)K1[cur], Q[cur]};
                    len++;
                    if (PR[cur] != cur && (FL[PR[cur]] & 1)) stop_at_used = true;
                    FL[cur] |= 1;
                }
                if (len >= (uint32_t)o.min_num_anchors) {
                    float adj = SC[end];
                    if (stop_at_used) adj -= SC[PR[cur]];
                    if (nc < room) {
                        s_rec[nc] = ChainRecDev{adj, key, (uint32_t)K1[cur], (uint32_t)K1[end], len, na};
                        if (kMany) m_score[nc] = adj;
                    } else flags |= 2u;
                    nc++; na += len;
                }
            }
            below = !o.disable_score_filtering && SC[end] < maxs / 2;                  // rmap.cpp:502-504
        }
        nc = uni(nc); na = uni(na); flags = uni(flags);
        if (kScratch) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        lds_sync();
        if (kScratch) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (uni(below ? 1u : 0u)) break;
    }
}
// rmap.cpp:512 on one lane: read r's chains by chaining score, descending; equal scores keep their order (std::sort up to 16 elements, the tie
// flag beyond); its records to tmp_recs in that order, its counts and flags to cnt
__device__ __forceinline__ void chain_order(const ChainArgs &a, const uint32_t r, const uint32_t nc, const uint32_t na, uint32_t flags, const ChainRecDev *s_rec, uint32_t *s_perm)
{
    const uint32_t m = min(nc, kChainCap);
    bool ties = false;
    for (uint32_t i = 0; i < m; i++) {
        const float v = s_rec[i].score;
        uint32_t j = i;
        while (j > 0 && v > s_rec[s_perm[j - 1]].score) { s_perm[j] = s_perm[j - 1]; j--; }
        if (j > 0 && v == s_rec[s_perm[j - 1]].score) ties = true;
        s_perm[j] = i;
    }
    if (nc > kChainStable && ties) flags |= 4u;
    for (uint32_t i = 0; i < m; i++) a.tmp_recs[(uint64_t)r * kChainCap + i] = s_rec[s_perm[i]];
    a.cnt[r] = ChainCnt{nc, na, flags, 0u};
}
// MANY CHAINS A READ ("chain_max_chains").  rmap.cpp:512 for a read of up to a.cap chains, ties or not: std::sort's own order, restated in
// rawdtw_sort_order.h, on lane 0 over the scores (m_score) and a permutation (m_perm) in LDS, `room` entries each; its right parts wait on
// s_stack.  The records stay where chain_ends put them, as generated; the permutation goes to the read's stretch of tmp_perm, which
// k_chain_compact reads them through.  Called by the whole wave.  room <= the read's stretch and <= the LDS arrays: nothing is stored past either.
__device__ __forceinline__ void chain_order_many(const ChainArgs &a, const uint32_t r, const uint32_t nc, const uint32_t na, uint32_t flags, const uint32_t room,
                                                 const float *m_score, uint32_t *m_perm, sort_order::Range *s_stack, const uint32_t lane)
{
    const uint32_t m = min(nc, room);
    for (uint32_t i = lane; i < m; i += 64) m_perm[i] = i;
    lds_sync();
    uint32_t ok = 1;
    if (lane == 0) ok = sort_order::sort_order_desc(m_score, m_perm, m, s_stack, sort_order::kStackCap, nullptr) ? 1u : 0u;
    lds_sync();
    if (!uni(ok)) flags |= 2u; // (the stack did not hold: not with kStackCap entries for up to 4 096 chains)
    const uint64_t t0 = rec_start(a, r);
    for (uint32_t i = lane; i < m; i += 64) a.tmp_perm[t0 + i] = m_perm[i];
    if (lane == 0) a.cnt[r] = ChainCnt{nc, na, flags, 0u};
}
// what a read of n seeds may record with the option on: no more than the option, than its seeds can make, than the LDS arrays hold
__device__ __forceinline__ uint32_t many_room(const ChainArgs &a, const uint32_t n, const uint32_t lds_chains) { return min(min(a.cap, n / a.rec_div), lds_chains); }

// kMany: the round's cap on chains a read is the option's, not kChainCap -- the instantiation that is launched when the option is off is the
// kernel as it was, LDS and registers
template <bool kMany> __global__ __launch_bounds__(64) void k_chain(const ChainArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t n2 = a.n2, lane = threadIdx.x, r = blockIdx.x;
    unsigned long long *K1 = reinterpret_cast<unsigned long long *>(smem); // key << 32 | target
    uint32_t *Q = reinterpret_cast<uint32_t *>(K1 + n2);
    float *SC = reinterpret_cast<float *>(Q + n2);
    uint32_t *PR = reinterpret_cast<uint32_t *>(SC + n2);
    unsigned char *FL = reinterpret_cast<unsigned char *>(PR + n2); // 1 used, 2 end candidate, 4 taken
    __shared__ ChainRecDev s_rec[kMany ? 1 : kChainCap];
    __shared__ uint32_t s_perm[kMany ? 1 : kChainCap];
    __shared__ sort_order::Range s_stack[kMany ? sort_order::kStackCap : 1];
    float *m_score = reinterpret_cast<float *>(FL + n2); // (kMany: a.lds_chains scores, then as many entries of the order; n2 is a multiple of 64)
    uint32_t *m_perm = reinterpret_cast<uint32_t *>(m_score + a.lds_chains);
    const uint64_t s0 = a.seed_off[r];
    const uint32_t n = (uint32_t)(a.seed_off[r + 1] - s0);
    const uint32_t room = kMany ? many_room(a, n, a.lds_chains) : kChainCap;
    ChainRecDev *rec_out = kMany ? a.tmp_recs + rec_start(a, r) : s_rec;
    if (n == 0 || n > n2) { // (no seeds: no chains.  Too many: declined -- the host sizes n2 by the round's largest read, so only past the cap)
        if (lane == 0) a.cnt[r] = ChainCnt{0u, 0u, n > n2 ? 1u : 0u, 0u};
        return;
    }
    for (uint32_t i = lane; i < n2; i += 64) {
        if (i < n) { const rawdtw_seed_t s = a.seeds[s0 + i]; K1[i] = ((unsigned long long)s.key << 32) | s.target_position; Q[i] = s.query_position; }
        else { K1[i] = ~0ull; Q[i] = ~0u; }
        FL[i] = 0;
    }
    lds_sync();
    // ---- rmap.cpp:396-401: ascending by (key, target, query) ----
    for (uint32_t k = 2; k <= n2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < n2 / 2; t += 64) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j; // the pair's lower and upper element
                const unsigned long long ka = K1[i], kb = K1[p];
                const uint32_t qa = Q[i], qb = Q[p];
                const bool gt = ka > kb || (ka == kb && qa > qb);
                if (gt == ((i & k) == 0)) { K1[i] = kb; K1[p] = ka; Q[i] = qb; Q[p] = qa; }
            }
            lds_sync();
        }
    const rawdtw_chain_opt_t &o = a.opt;
    const float e_f = (float)o.e;
    float maxs = 0.0f;
    uint32_t nc = 0, na = 0, flags = 0;
    for (uint32_t g0 = 0; g0 < n;) {
        const uint32_t key = (uint32_t)(K1[g0] >> 32), g1 = list_end(K1, key, g0, n, lane); // the (sequence, strand) list [g0, g1)
        // ---- rmap.cpp:436-494 ----
        for (uint32_t ai = g0; ai < g1; ai++) {
            const int32_t ct = (int32_t)(uint32_t)K1[ai], cq = (int32_t)Q[ai];
            float best = e_f;
            uint32_t pred = ai;
            int32_t skips = 0;
            const int32_t lo = (ai - g0 > (uint32_t)o.chaining_band_length) ? (int32_t)ai - o.chaining_band_length : (int32_t)g0;
            for (int32_t base = (int32_t)ai - 1; base >= lo; base -= 64) {
                const int32_t pi = base - (int32_t)lane;
                const bool valid = pi >= lo;
                const int32_t pt = (int32_t)(uint32_t)K1[valid ? pi : lo], pq = (int32_t)Q[valid ? pi : lo];
                const float sp = SC[valid ? pi : lo];
                if (chain_step(o, ct, cq, base, valid, pt, pq, sp, best, pred, skips)) break;
            }
            if (best > maxs) maxs = best;                                                   // rmap.cpp:486-488
            const bool is_end = o.disable_score_filtering || (best >= o.min_chaining_score && best > maxs / 2); // rmap.cpp:489-493
            if (lane == 0) { SC[ai] = best; PR[ai] = pred; FL[ai] = is_end ? 2 : 0; }
            lds_sync();
        }
        chain_ends<false, kMany>(a, K1, Q, SC, PR, FL, key, g0, g1, s0, maxs, lane, rec_out, nc, na, flags, m_score, room);
        g0 = g1;
    }
    if (kMany) chain_order_many(a, r, nc, na, flags, room, m_score, m_perm, s_stack, lane);
    else if (lane == 0) chain_order(a, r, nc, na, flags, s_rec, s_perm);
}

// ---- the long path: reads above k_chain's cap, state in device memory ----
// Scratch a long seed: K1 8 + Q 4 (the sorted seeds), SC 4 + PR 4 + FL 1 (the DP's state) = 21 bytes; a read's stretch starts on a multiple of
// 64 elements (at most 63 * 21 bytes of padding a read) and each of the five arrays on a multiple of 256 bytes.
constexpr uint32_t kSortBlock = 4096;   // elements sorted in LDS at a time: 48 KiB
constexpr uint32_t kRing = 1024;        // the DP's LDS ring: 12 bytes an entry
constexpr uint32_t kNear = kRing - 64;  // candidates at most this far behind the current anchor are read from the ring (see k_chain_long)

struct LongRead { uint32_t r, pad; uint64_t off; }; // the read, and where its stretch of the scratch arrays starts (in elements)
struct LongArgs {
    const LongRead *reads;
    unsigned long long *K1; // key << 32 | target, sorted
    uint32_t *Q;
    float *SC;
    uint32_t *PR;
    unsigned char *FL;
    unsigned long long *far_steps; // the round's totals[4]
    uint32_t lds_chains;           // "chain_max_chains": k_chain_long's dynamic LDS holds the scores and the order of this many chains (0: none)
};

__device__ __forceinline__ void sort_cmp(unsigned long long &ka, uint32_t &qa, unsigned long long &kb, uint32_t &qb)
{
    if (ka > kb || (ka == kb && qa > qb)) { const unsigned long long k = ka; ka = kb; kb = k; const uint32_t q = qa; qa = qb; qb = q; }
}
// the workgroup's writes to device memory, for its own later reads: the waves share the CU's L1, the agent-scope fences are belt and braces
__device__ __forceinline__ void wg_global_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// A workgroup a long read: rmap.cpp:396-401, ascending by (key, target, query), into the read's stretch of K1 / Q.  A bitonic network whose
// comparators all point upwards (each merge starts with the mirrored step i <-> i ^ (k - 1), then half-cleaners i <-> i + j), so that any n
// sorts as if padded with +infinity behind it: a comparator whose upper element is at or past n would find infinity there and is left out.
// Merges up to 4 096 elements, and the tail of every wider merge, run on blocks in LDS; the wider steps run in device memory.
__global__ __launch_bounds__(256) void k_chain_sort_long(const ChainArgs a, const LongArgs la)
{
    __shared__ unsigned long long s_k[kSortBlock];
    __shared__ uint32_t s_q[kSortBlock];
    const LongRead lr = la.reads[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint64_t s0 = a.seed_off[lr.r];
    const uint32_t n = (uint32_t)(a.seed_off[lr.r + 1] - s0);
    unsigned long long *K1 = la.K1 + lr.off;
    uint32_t *Q = la.Q + lr.off;
    for (uint32_t b0 = 0; b0 < n; b0 += kSortBlock) {
        for (uint32_t i = tid; i < kSortBlock; i += 256) {
            if (b0 + i < n) { const rawdtw_seed_t s = a.seeds[s0 + b0 + i]; s_k[i] = ((unsigned long long)s.key << 32) | s.target_position; s_q[i] = s.query_position; }
            else { s_k[i] = ~0ull; s_q[i] = ~0u; }
        }
        __syncthreads();
        for (uint32_t k = 2; k <= kSortBlock; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t t = tid; t < kSortBlock / 2; t += 256) {
                    const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = (j == (k >> 1)) ? (i ^ (k - 1)) : (i | j);
                    sort_cmp(s_k[i], s_q[i], s_k[p], s_q[p]);
                }
                __syncthreads();
            }
        for (uint32_t i = tid; i < kSortBlock && b0 + i < n; i += 256) { K1[b0 + i] = s_k[i]; Q[b0 + i] = s_q[i]; }
        __syncthreads();
    }
    if (n <= kSortBlock) return;
    uint32_t n2 = kSortBlock;
    while (n2 < n) n2 <<= 1;
    wg_global_sync();
    for (uint32_t k = 2 * kSortBlock; k <= n2; k <<= 1) {
        for (uint32_t j = k >> 1; j >= kSortBlock; j >>= 1) {
            for (uint32_t t = tid; t < n2 / 2; t += 256) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = (j == (k >> 1)) ? (i ^ (k - 1)) : (i | j);
                if (p < n) { // (i < p)
                    unsigned long long ka = K1[i], kb = K1[p];
                    uint32_t qa = Q[i], qb = Q[p];
                    if (ka > kb || (ka == kb && qa > qb)) { K1[i] = kb; K1[p] = ka; Q[i] = qb; Q[p] = qa; }
                }
            }
            wg_global_sync();
        }
        for (uint32_t b0 = 0; b0 < n; b0 += kSortBlock) { // the half-cleaners below the block size
            for (uint32_t i = tid; i < kSortBlock; i += 256) {
                if (b0 + i < n) { s_k[i] = K1[b0 + i]; s_q[i] = Q[b0 + i]; }
                else { s_k[i] = ~0ull; s_q[i] = ~0u; }
            }
            __syncthreads();
            for (uint32_t j = kSortBlock >> 1; j > 0; j >>= 1) {
                for (uint32_t t = tid; t < kSortBlock / 2; t += 256) {
                    const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    sort_cmp(s_k[i], s_q[i], s_k[i | j], s_q[i | j]);
                }
                __syncthreads();
            }
            for (uint32_t i = tid; i < kSortBlock && b0 + i < n; i += 256) { K1[b0 + i] = s_k[i]; Q[b0 + i] = s_q[i]; }
            __syncthreads();
        }
        wg_global_sync();
    }
}

// A wave a long read: k_chain's DP, ends, traceback and order over the sorted seeds in scratch.
//   * The anchors come 64 at a time into registers (lane l: anchor blk + l) and, with their targets and queries, into the LDS ring at slot
//     index & (kRing - 1); an anchor's score joins its slot when it is final.  Loading a block overwrites the slots of anchors blk - kRing ..
//     blk - kRing + 63, so the ring is good for candidates no more than kNear = kRing - 64 behind the current anchor.
//   * SC, PR and FL of a block are kept in registers and go to scratch when the block (or the list) ends: `flushed` anchors are in scratch.
//   * A candidate further back than kNear -- reached only through a run of pass-over candidates longer than that -- is read from scratch:
//     the far path.  It is at least kNear - 63 > 0 anchors behind the last flush, so what it reads was stored by this wave at least one flush
//     earlier; every flush ends in an agent-scope release (the stores are complete at L2 before the wave goes on), and the scores, the only
//     array of the three that this launch wrote, are loaded with agent-scope atomic loads, which do not take a line from L1.  That holds for
//     any kRing >= 128, not by the distance of 960.
//   * Ends and traceback read and mark scratch: a release and an acquire at agent scope stand between lane 0's marks and the wave's next look.
template <bool kMany> __global__ __launch_bounds__(64) void k_chain_long(const ChainArgs a, const LongArgs la)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[]; // (kMany only: la.lds_chains scores, then as many entries of the order)
    __shared__ uint32_t r_t[kRing], r_q[kRing];
    __shared__ float r_s[kRing];
    __shared__ ChainRecDev s_rec[kMany ? 1 : kChainCap];
    __shared__ uint32_t s_perm[kMany ? 1 : kChainCap];
    __shared__ sort_order::Range s_stack[kMany ? sort_order::kStackCap : 1];
    const LongRead lr = la.reads[blockIdx.x];
    const uint32_t lane = threadIdx.x, r = lr.r;
    const uint64_t s0 = a.seed_off[r];
    const uint32_t n = (uint32_t)(a.seed_off[r + 1] - s0);
    float *m_score = kMany ? reinterpret_cast<float *>(smem) : nullptr;
    uint32_t *m_perm = kMany ? reinterpret_cast<uint32_t *>(m_score + la.lds_chains) : nullptr;
    const uint32_t room = kMany ? many_room(a, n, la.lds_chains) : kChainCap;
    ChainRecDev *rec_out = kMany ? a.tmp_recs + rec_start(a, r) : s_rec;
    const unsigned long long *K1 = la.K1 + lr.off;
    const uint32_t *Q = la.Q + lr.off;
    float *SC = la.SC + lr.off;
    uint32_t *PR = la.PR + lr.off;
    unsigned char *FL = la.FL + lr.off;
    if (n == 0) { if (lane == 0) a.cnt[r] = ChainCnt{0u, 0u, 0u, 0u}; return; }
    auto slot = [](const uint32_t i) { return i & (kRing - 1); };
    const rawdtw_chain_opt_t &o = a.opt;
    const float e_f = (float)o.e;
    float maxs = 0.0f;
    uint32_t nc = 0, na = 0, flags = 0, far = 0, flushed = 0;
    uint32_t b_t = 0, b_q = 0, b_pr = 0, b_fl = 0; // this lane's anchor of the current block, and its state
    float b_sc = 0.0f;
    auto flush = [&](const uint32_t upto) { // anchors [flushed, upto) -- inside one block -- to scratch
        const uint32_t x = (flushed & ~63u) + lane;
        if (x >= flushed && x < upto) { SC[x] = b_sc; PR[x] = b_pr; FL[x] = (unsigned char)b_fl; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        flushed = upto;
    };
    for (uint32_t g0 = 0; g0 < n;) {
        const uint32_t key = (uint32_t)(K1[g0] >> 32), g1 = list_end(K1, key, g0, n, lane); // the (sequence, strand) list [g0, g1)
        // ---- rmap.cpp:436-494 ----
        for (uint32_t ai = g0; ai < g1; ai++) {
            if (ai == 0 || (ai & 63u) == 0) { // the next block: registers and ring
                const uint32_t x = ai + lane;
                if (x < n) { b_t = (uint32_t)K1[x]; b_q = Q[x]; r_t[slot(x)] = b_t; r_q[slot(x)] = b_q; }
                lds_sync();
            }
            const int32_t ct = (int32_t)lane_of(b_t, ai & 63u), cq = (int32_t)lane_of(b_q, ai & 63u);
            float best = e_f;
            uint32_t pred = ai;
            int32_t skips = 0;
            const int32_t lo = (ai - g0 > (uint32_t)o.chaining_band_length) ? (int32_t)ai - o.chaining_band_length : (int32_t)g0;
            for (int32_t base = (int32_t)ai - 1; base >= lo; base -= 64) {
                const int32_t pi = base - (int32_t)lane;
                const bool valid = pi >= lo;
                const uint32_t x = (uint32_t)(valid ? pi : lo);
                const bool is_far = x + kNear < ai;
                int32_t pt, pq;
                float sp;
                if (!is_far) { pt = (int32_t)r_t[slot(x)]; pq = (int32_t)r_q[slot(x)]; sp = r_s[slot(x)]; }
                else { pt = (int32_t)(uint32_t)K1[x]; pq = (int32_t)Q[x]; sp = __hip_atomic_load(SC + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
                if (__ballot(valid && is_far)) far++;
                if (chain_step(o, ct, cq, base, valid, pt, pq, sp, best, pred, skips)) break;
            }
            if (best > maxs) maxs = best;                                                   // rmap.cpp:486-488
            const bool is_end = o.disable_score_filtering || (best >= o.min_chaining_score && best > maxs / 2); // rmap.cpp:489-493
            if (lane == (ai & 63u)) { b_sc = best; b_pr = pred; b_fl = is_end ? 2u : 0u; }
            if (lane == 0) r_s[slot(ai)] = best;
            lds_sync();
            if ((ai & 63u) == 63u) flush(ai + 1);
        }
        if (flushed < g1) flush(g1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        chain_ends<true, kMany>(a, K1, Q, SC, PR, FL, key, g0, g1, s0, maxs, lane, rec_out, nc, na, flags, m_score, room);
        g0 = g1;
    }
    if (kMany) chain_order_many(a, r, nc, na, flags, room, m_score, m_perm, s_stack, lane);
    else if (lane == 0) chain_order(a, r, nc, na, flags, s_rec, s_perm);
    if (lane == 0 && far) atomicAdd(la.far_steps, (unsigned long long)far);
}

// DECLINING A READ ("chain_decline_reads", off by default).  A read the device cannot chain -- more seeds than the caps (marked by the host at
// begin: reason 1), or what k_chain / k_chain_long flag in its count (1 too many seeds, 2 too many chains, 4 an order only std::sort knows) -- no
// longer declines its round.  The declining instantiations of the scan and the compaction give it an empty stretch of chain_off, its reason in
// why[r] and an entry of the compact list of declined reads, ascending; the round's flags stay 0.  The host chains those reads and puts their
// chains behind the device's (rawdtw_chain_round_append).  The <false> instantiations are the kernels as they were.
struct DeclRec { uint32_t r, why; uint64_t seed0; }; // a declined read, its reason, and the declined reads' seeds before it
struct DeclArgs {
    const uint8_t *mark; // per read: declined at begin
    uint32_t *why;       // per read: 0, or the reason's bits
    DeclRec *list;       // the declined reads, ascending
    const uint64_t *seed_off;
};

// the reads' chains and anchors before each read; the round's totals and its flags; totals[5 .. 7]: the reads with more than kChainCap chains,
// with more than kChainStable, and the most chains a read has (rawdtw_chain_order_stats).  cap: chains a read the round records.
// kDecline: totals has 16 words -- [8] the declined reads, [9 .. 11] those with reason bit 1, 2, 4, [12] their seeds; [2] stays 0, and
// [5 .. 7] count the reads that were not declined.
template <bool kDecline> __global__ __launch_bounds__(1024) void k_chain_scan(const ChainCnt *__restrict__ cnt, const uint32_t n_reads, const uint32_t cap, uint64_t *__restrict__ chain_off,
                                                     uint64_t *__restrict__ read_anchor0, uint64_t *__restrict__ totals /* chains, anchors, flags */, const DeclArgs dd)
{
    __shared__ uint64_t s_c[1024], s_a[1024];
    __shared__ uint32_t s_f[1024];
    __shared__ uint32_t s_st[3];
    __shared__ uint32_t s_d[kDecline ? 1024 : 1], s_why[kDecline ? 3 : 1];
    __shared__ uint64_t s_ds[kDecline ? 1024 : 1];
    const uint32_t t = threadIdx.x, per = (n_reads + 1023u) / 1024u, lo = min(n_reads, t * per), hi = min(n_reads, lo + per);
    uint64_t c = 0, x = 0, ds = 0;
    uint32_t f = 0, above_cap = 0, above_stable = 0, most = 0, nd = 0;
    if (t < 3) s_st[t] = 0;
    if (kDecline && t < 3) s_why[t] = 0;
    __syncthreads();
    for (uint32_t r = lo; r < hi; r++) {
        const uint32_t nc = cnt[r].nc;
        if (kDecline) {
            const uint32_t why = dd.mark[r] ? 1u : (cnt[r].flags & 7u);
            dd.why[r] = why;
            if (why) {
                nd++; ds += dd.seed_off[r + 1] - dd.seed_off[r];
                for (uint32_t b = 0; b < 3; b++) if (why >> b & 1u) atomicAdd(&s_why[b], 1u);
                continue;
            }
        }
        c += min(nc, cap); x += cnt[r].na; f |= cnt[r].flags;
        above_cap += nc > kChainCap; above_stable += nc > kChainStable; most = max(most, nc);
    }
    s_c[t] = c; s_a[t] = x; s_f[t] = f;
    if (kDecline) { s_d[t] = nd; s_ds[t] = ds; }
    if (above_cap) atomicAdd(&s_st[0], above_cap);
    if (above_stable) atomicAdd(&s_st[1], above_stable);
    if (most) atomicMax(&s_st[2], most);
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t pc = t >= d ? s_c[t - d] : 0, pa = t >= d ? s_a[t - d] : 0;
        const uint32_t pf = t >= d ? s_f[t - d] : 0;
        const uint32_t pd = kDecline && t >= d ? s_d[t - d] : 0;
        const uint64_t ps = kDecline && t >= d ? s_ds[t - d] : 0;
        __syncthreads();
        s_c[t] += pc; s_a[t] += pa; s_f[t] |= pf;
        if (kDecline) { s_d[t] += pd; s_ds[t] += ps; }
        __syncthreads();
    }
    uint64_t bc = s_c[t] - c, ba = s_a[t] - x;
    uint32_t bd = kDecline ? s_d[t] - nd : 0;  // (the declined reads before this thread's: its reads ascend, so does the list)
    uint64_t bs = kDecline ? s_ds[t] - ds : 0;
    for (uint32_t r = lo; r < hi; r++) {
        chain_off[r] = bc; read_anchor0[r] = ba;
        if (kDecline && dd.why[r]) { dd.list[bd++] = DeclRec{r, dd.why[r], bs}; bs += dd.seed_off[r + 1] - dd.seed_off[r]; continue; }
        bc += min(cnt[r].nc, cap); ba += cnt[r].na;
    }
    if (t == 1023) {
        chain_off[n_reads] = s_c[t]; totals[0] = s_c[t]; totals[1] = s_a[t]; totals[2] = s_f[t]; totals[3] = 0;
        totals[5] = s_st[0]; totals[6] = s_st[1]; totals[7] = s_st[2];
        if (kDecline) { totals[8] = s_d[t]; totals[9] = s_why[0]; totals[10] = s_why[1]; totals[11] = s_why[2]; totals[12] = s_ds[t]; }
    }
}

// a wave a read: its chains, in evaluation order, into the batch's arrays.  kDecline: nothing for a declined read (why[r] != 0).
template <bool kDecline> __global__ __launch_bounds__(64) void k_chain_compact(const ChainArgs a, const uint64_t *__restrict__ chain_off, const uint64_t *__restrict__ read_anchor0,
                                                      const uint32_t *__restrict__ read_base, const uint64_t *__restrict__ key_base, const uint32_t n_keys,
                                                      uint64_t *__restrict__ anchor_off, rawdtw_anchor_t *__restrict__ anchors, uint64_t *__restrict__ ref_base,
                                                      uint32_t *__restrict__ read_base_c, rawdtw_chain_rec_t *__restrict__ recs, uint64_t *__restrict__ totals,
                                                      // the caller's page-locked host arrays, written from here (null: they are copied afterwards)
                                                      uint64_t *__restrict__ h_anchor_off, rawdtw_chain_rec_t *__restrict__ h_recs, rawdtw_anchor_t *__restrict__ h_anchors,
                                                      const uint64_t h_chains_cap, const uint32_t *__restrict__ why)
{
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const uint64_t c0 = chain_off[r], s0 = a.seed_off[r], t0 = rec_start(a, r);
    uint32_t nc = min(a.cnt[r].nc, a.cap);
    if (kDecline && why[r]) nc = 0;
    if (a.rec_div) nc = (uint32_t)min((uint64_t)nc, (a.seed_off[r + 1] - s0) / a.rec_div); // (many chains a read: the stretch the kernels recorded into; a read has no more chains than that)
    const bool host = h_anchor_off && totals[2] == 0 && totals[0] <= h_chains_cap; // (a declined round leaves the host arrays alone)
    uint64_t dst = read_anchor0[r];
    for (uint32_t i = 0; i < nc; i++) {
        const ChainRecDev rec = a.tmp_recs[t0 + (a.tmp_perm ? min(a.tmp_perm[t0 + i], nc - 1u) : i)]; // (many chains a read: through the order, inside the read's records)
        for (uint32_t k = lane; k < rec.n; k += 64) {
            const rawdtw_anchor_t v = a.tmp_anchors[s0 + rec.a_off + k];
            anchors[dst + k] = v;
            if (host && h_anchors) h_anchors[dst + k] = v;
        }
        if (lane == 0) {
            const rawdtw_chain_rec_t out{rec.score, rec.key, rec.start, rec.end, rec.n};
            anchor_off[c0 + i] = dst;
            ref_base[c0 + i] = rec.key < n_keys ? key_base[rec.key] : 0ull;
            if (rec.key >= n_keys) atomicOr(reinterpret_cast<unsigned long long *>(totals + 3), 1ull); // (a seed on a key the caller gave no base for)
            read_base_c[c0 + i] = read_base[r];
            recs[c0 + i] = out;
            if (host) { h_anchor_off[c0 + i] = dst; h_recs[c0 + i] = out; }
        }
        dst += rec.n;
    }
    if (r == 0 && lane == 0) { anchor_off[totals[0]] = totals[1]; if (host) h_anchor_off[totals[0]] = totals[1]; }
}

// "chain_decline_reads": a wave a declined read -- its stretch of the round's seed list as it was laid down (in a resident round by the seeding's
// writer launch, from the kept store, the host's previous anchors and the hits), 12 bytes a seed, to out[list[j].seed0 ..).  The host launches
// one block for each entry of the list and has checked that `out` holds the list's seeds (totals[12]).
__global__ __launch_bounds__(64) void k_declined_seeds(const DeclRec *__restrict__ list, const uint64_t *__restrict__ seed_off, const rawdtw_seed_t *__restrict__ seeds,
                                                       rawdtw_seed_t *__restrict__ out)
{
    const DeclRec d = list[blockIdx.x];
    const uint64_t s0 = seed_off[d.r], words = (seed_off[d.r + 1] - s0) * 3;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(seeds + s0);
    uint32_t *dst = reinterpret_cast<uint32_t *>(out + d.seed0);
    for (uint64_t i = threadIdx.x; i < words; i += 64) dst[i] = src[i];
}

using capi::carve;
// A round's workspace, described once: lay(0) gives the bytes it needs, lay(the block's base) the round's pointers.  Every array starts on a
// multiple of 256 bytes; the arrays of a resident round and of the long path take no space in a round that has none.
struct ChainLayout {
    uint64_t n_reads, n_seeds, n_keys;
    bool resident;
    uint64_t n_prev, n_long, long_elems; // (long_elems: the long reads' seeds, each read's stretch rounded up to 64)
    // "chain_max_chains" (0: off -- kChainCap chains a read) and max(1, min_num_anchors).  With the option on the chain-sized arrays hold
    // min(n_reads * max_chains, n_seeds / rec_div + 1) entries: chains of a read share no anchor and a recorded chain has at least min_num_anchors,
    // so a read of n seeds records at most n / rec_div chains and the round n_seeds / rec_div.  A read's records then start at seed_off[r] / rec_div
    // (by_seeds) -- floor(x / d) + floor(n / d) <= floor((x + n) / d): the stretches do not overlap -- or, where n_reads * max_chains is the
    // smaller bound, at r * max_chains.  68 bytes a chain: trec 24, tperm 4, aoff 8, refb 8, rbc 4, recs 20.
    // "chain_decline_reads": the host's chains of the declined reads are appended behind the device's, in the batch's arrays.  Chains of a read
    // share no anchor and a recorded chain has at least max(1, min_num_anchors) anchors, whoever made it: a read of n seeds has at most
    // n / rec_div chains and the ROUND AT MOST n_seeds / rec_div, device-made and appended together -- chains_by_seeds().  The batch's chain-sized
    // arrays (aoff, refb, rbc, recs) then hold max(chain_entries(), chains_by_seeds()) entries, and the anchors' n_seeds + 2 hold every chain's
    // anchors as they always did; rawdtw_chain_round_append checks both before it writes.  The per-read arrays of the option (mark, why, dlist) and
    // the second half of the totals take no space with the option off.
    uint64_t max_chains = 0, rec_div = 1;
    bool decline = false;
    uint8_t *mark; uint32_t *why; DeclRec *dlist;
    uint64_t *soff; rawdtw_seed_t *seeds; uint32_t *rb; uint64_t *kb;                          // inputs
    rawdtw_anchor_t *tmpa; ChainRecDev *trec; ChainCnt *cnt; uint64_t *coff, *ra0;             // per-read scratch
    uint64_t *tot;                                                                             // chains, anchors, flags, bad keys; [4]: the long path's far steps; [5 .. 7]: k_chain_scan's counts
    uint64_t *aoff; rawdtw_anchor_t *anch; uint64_t *refb; uint32_t *rbc; rawdtw_chain_rec_t *recs; // the batch's arrays
    rawdtw_seed_t *prev; uint64_t *poff; uint32_t *cs; uint8_t *so; // a resident round: the previous anchors, dense, their offsets, the chunk starts, the sits-out flags
    uint32_t *psrc;                                            // ... and per read where its previous anchors come from: RAWDTW_PREV_HOST (the dense upload) or a half of the kept chains' store
    LongArgs la;                                               // the long reads' list and their scratch: 21 bytes a seed -- K1 8, Q 4, SC 4, PR 4, FL 1
    uint32_t *tperm;                                           // "chain_max_chains": the reads' evaluation orders (ChainArgs::tmp_perm)

    uint64_t cap() const { return max_chains ? max_chains : kChainCap; }
    uint64_t chains_by_seeds() const { return n_seeds / rec_div + 1; }
    bool by_seeds() const { return max_chains && chains_by_seeds() <= n_reads * max_chains; }
    uint64_t chain_entries() const { return by_seeds() ? chains_by_seeds() : n_reads * cap(); } // what the chain-sized arrays hold
    uint64_t batch_entries() const { return decline ? std::max(chain_entries(), chains_by_seeds()) : chain_entries(); } // ... and the batch's, which take the append
    uint64_t tot_words() const { return decline ? 16 : 8; }

    size_t lay(void *base)
    {
        uintptr_t p = reinterpret_cast<uintptr_t>(base);
        const uint64_t nc = chain_entries(), nb = batch_entries(), nres = resident ? n_reads : 0, ndec = decline ? n_reads : 0;
        soff = carve<uint64_t>(p, n_reads + 1); seeds = carve<rawdtw_seed_t>(p, n_seeds + 2); rb = carve<uint32_t>(p, n_reads); kb = carve<uint64_t>(p, n_keys + 1);
        tmpa = carve<rawdtw_anchor_t>(p, n_seeds + 2); trec = carve<ChainRecDev>(p, nc); cnt = carve<ChainCnt>(p, n_reads);
        coff = carve<uint64_t>(p, n_reads + 1); ra0 = carve<uint64_t>(p, n_reads); tot = carve<uint64_t>(p, tot_words());
        aoff = carve<uint64_t>(p, nb + 1); anch = carve<rawdtw_anchor_t>(p, n_seeds + 2); refb = carve<uint64_t>(p, nb + 1); rbc = carve<uint32_t>(p, nb + 2);
        recs = carve<rawdtw_chain_rec_t>(p, nb + 1);
        prev = carve<rawdtw_seed_t>(p, resident ? n_prev + 2 : 0); poff = carve<uint64_t>(p, resident ? n_reads + 1 : 0); cs = carve<uint32_t>(p, nres);
        so = carve<uint8_t>(p, nres); psrc = carve<uint32_t>(p, nres);
        la.reads = carve<LongRead>(p, n_long); la.K1 = carve<unsigned long long>(p, long_elems); la.Q = carve<uint32_t>(p, long_elems);
        la.SC = carve<float>(p, long_elems); la.PR = carve<uint32_t>(p, long_elems); la.FL = carve<unsigned char>(p, long_elems);
        la.far_steps = reinterpret_cast<unsigned long long *>(tot) + 4;
        tperm = carve<uint32_t>(p, max_chains ? nc : 0);
        mark = carve<uint8_t>(p, ndec); why = carve<uint32_t>(p, ndec); dlist = carve<DeclRec>(p, ndec);
        return (size_t)(p - reinterpret_cast<uintptr_t>(base));
    }
};

struct ChainWs {
    void *dev = nullptr;
    size_t dev_bytes = 0;
    void *pin = nullptr; // totals
    hipEvent_t done = nullptr; // behind a round's last copy: what rawdtw_chain_round_end waits for (not for what the caller enqueued behind the round)
    // a round begun and not ended
    bool pending = false, direct = false;
    uint64_t n_reads = 0, chains_cap = 0, n_long = 0;
    uint64_t *h_anchor_off = nullptr;
    rawdtw_chain_rec_t *h_recs = nullptr;
    rawdtw_anchor_t *h_anchors = nullptr;
    const uint64_t *d_aoff = nullptr;
    const rawdtw_chain_rec_t *d_recs = nullptr;
    const rawdtw_anchor_t *d_anch = nullptr;
    const uint64_t *d_refb = nullptr;
    const uint32_t *d_rbc = nullptr;
    // the long path: the round's long reads (kept here until the round's end: their upload reads them), and rawdtw_chain_round_stats' counters
    std::vector<LongRead> long_reads;
    uint64_t st_rounds = 0, st_long_reads = 0, st_long_seeds = 0, st_far_steps = 0;
    // rawdtw_chain_order_stats' counters, over the rounds that were not declined
    bool many = false; // (the round begun ran with "chain_max_chains" on)
    uint64_t st_above_32 = 0, st_restated = 0, st_max_chains = 0;
    // "chain_decline_reads": the round begun ran with it; what the append and the declined reads' seeds need of the round after its end
    bool decline = false, ended = false, appendable = false; // (ended: a declining round's _end succeeded and no round was begun since)
    size_t pin_bytes = 0;
    uint64_t n_seeds = 0, batch_room = 0, nc = 0, na = 0, decl_seeds = 0;
    uint64_t *h_chain_off = nullptr;
    std::vector<uint8_t> marks;
    std::vector<uint32_t> h_read_base, decl_reads, decl_why, app_rbc;
    std::vector<uint64_t> h_key_base, decl_seed0, app_refb;
    std::vector<DeclRec> decl;
    const uint64_t *d_soff = nullptr; const rawdtw_seed_t *d_seeds = nullptr; const DeclRec *d_list = nullptr;
    void *pin_seeds = nullptr; size_t pin_seeds_bytes = 0; // the declined reads' seeds on their way to an array that is not page-locked
};

bool page_locked(const void *q)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}

} // namespace
} // namespace rawdtw

using namespace rawdtw;
using namespace rawdtw::capi;

struct rawdtw_chain_ws { ChainWs w; };

namespace {

// where a resident round's seeds come from (rawdtw_chain_round_begin_resident): the previous chains' anchors from the host, the hits from the
// context's ended resident seeding
struct ResidentSeeds {
    const uint64_t *prev_off;
    const rawdtw_seed_t *prev_seeds;
    const uint32_t *chunk_start;
    const uint8_t *sits_out;
    const uint32_t *prev_src; // (null: every read's from the host -- rawdtw_chain_round_begin_resident)
};

// rawdtw_chain_round_begin; `res`: the seed list is not the caller's `seeds` but laid down on the device
int chain_begin(rawdtw_ctx *ctx, const rawdtw_chain_opt_t *opt, uint64_t n_reads, const uint64_t *seed_off, const rawdtw_seed_t *seeds, const ResidentSeeds *res,
                const uint32_t *read_base, uint32_t n_keys, const uint64_t *key_base, uint64_t *chain_off, uint64_t *anchor_off,
                rawdtw_chain_rec_t *recs, uint64_t chains_cap, rawdtw_anchor_t *anchors)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!opt || !seed_off || (!res && !seeds && n_reads && seed_off[n_reads]) || !read_base || (!key_base && n_keys) || !chain_off || !anchor_off || !recs)
        return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (res && (!res->prev_off || !res->chunk_start || !res->sits_out)) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (ctx->chain_ws && ctx->chain_ws->w.pending) return fail(ctx, RAWDTW_ERR_INVALID, "a chaining round is begun on this context and not ended");
    if (ctx->chain_ws) { // (any begin, refused or not, ends what the round before left for rawdtw_chain_round_declined / _append)
        ChainWs &w0 = ctx->chain_ws->w;
        w0.ended = false; w0.appendable = false; w0.decl_reads.clear(); w0.decl_why.clear(); w0.decl_seed0.clear(); w0.decl_seeds = 0;
    }
    if (n_reads == 0 || n_reads > 0xffffffffull) return fail(ctx, RAWDTW_ERR_INVALID, "no reads, or more than 2^32");
    uint64_t n_prev = 0;
    if (res) { // every read's stretch is its previous anchors plus its chunk's hits, or empty: the device writes exactly that and nothing else
        uint64_t nc = 0;
        const uint64_t *hoff = seed_resident_hit_off(ctx, &nc);
        if (!hoff) return fail(ctx, RAWDTW_ERR_INVALID, "no ended resident seeding on this context (rawdtw_seed_resident_begin / _end)");
        if (nc != n_reads) return fail(ctx, RAWDTW_ERR_INVALID, "the resident seeding's chunks are not this round's reads");
        if (seed_off[0] != 0 || res->prev_off[0] != 0) return fail(ctx, RAWDTW_ERR_INVALID, "offsets do not start at 0");
        KeepStoreView kv;
        const bool store = res->prev_src && keep_store_view(ctx, &kv);
        for (uint64_t r = 0; r < n_reads; r++) {
            if (seed_off[r + 1] < seed_off[r] || res->prev_off[r + 1] < res->prev_off[r]) return fail(ctx, RAWDTW_ERR_INVALID, "offsets do not ascend");
            uint64_t pv = res->prev_off[r + 1] - res->prev_off[r];
            if (res->prev_src && res->prev_src[r] != RAWDTW_PREV_HOST) { // from the store: the half's count as the last fetched keep left it
                const uint32_t addr = res->prev_src[r];
                if (!store || addr >= kv.L.halves()) return fail(ctx, RAWDTW_ERR_INVALID, "a read's source is outside the store of kept chains (or there is none)");
                if (kv.mirror[addr] == RAWDTW_NOT_KEPT) return fail(ctx, RAWDTW_ERR_INVALID, "a read's source is a half that holds no kept chains");
                if (res->sits_out[r]) return fail(ctx, RAWDTW_ERR_INVALID, "a read that sits out has a source in the store of kept chains");
                if (pv) return fail(ctx, RAWDTW_ERR_INVALID, "a read seeded from the store of kept chains has previous seeds from the host too");
                pv = kv.mirror[addr];
            }
            const uint64_t want = res->sits_out[r] ? 0 : pv + (hoff[r + 1] - hoff[r]);
            if ((res->sits_out[r] && pv) || seed_off[r + 1] - seed_off[r] != want)
                return fail(ctx, RAWDTW_ERR_INVALID, "a read's seed_off stretch is not its previous anchors plus its chunk's hits (empty for a read that sits out)");
        }
        n_prev = res->prev_off[n_reads];
        if (n_prev && !res->prev_seeds) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t n_seeds = seed_off[n_reads];
    const uint32_t seed_cap = ctx->chain_max_seeds ? std::min(kChainMaxSeeds, ctx->chain_max_seeds) : kChainMaxSeeds;
    const uint64_t long_cap = ctx->chain_long_seeds; // ("chain_long_seeds"; 0: no long path)
    const uint32_t max_chains = ctx->chain_max_chains; // ("chain_max_chains"; 0: kChainCap a read, kChainStable with ties)
    const uint32_t rec_div = (uint32_t)std::max(1, opt->min_num_anchors);
    uint32_t most = 0; // (of the reads k_chain takes)
    uint64_t n_long = 0, long_elems = 0, most_long = 0;
    const bool decline = ctx->chain_decline_reads; // ("chain_decline_reads": a read above the caps is declined alone, and left out of `most` and the long list)
    bool too_long = false;
    for (uint64_t r = 0; r < n_reads; r++) {
        if (seed_off[r + 1] < seed_off[r]) return fail(ctx, RAWDTW_ERR_INVALID, "offsets do not ascend");
        const uint64_t nr = seed_off[r + 1] - seed_off[r];
        if (nr <= seed_cap) most = std::max(most, (uint32_t)nr);
        else if (nr <= long_cap) { n_long++; long_elems += (nr + 63) & ~63ull; most_long = std::max(most_long, nr); }
        else if (!decline) too_long = true;
    }
    if (too_long) return fail(ctx, RAWDTW_ERR_UNSUPPORTED, long_cap ? "a read has more seeds than \"chain_long_seeds\" allows: chain this round on the host"
                                                                   : "a read has more seeds than the device chains (2048): chain this round on the host");
    uint32_t n2 = 64;
    while (n2 < most) n2 <<= 1;
    // one block of device memory, grow-only: laid out from 0 for its size, from the block's base for the round's pointers
    ChainLayout L{n_reads, n_seeds, n_keys, res != nullptr, n_prev, n_long, long_elems, max_chains, rec_div, decline};
    const size_t need = L.lay(nullptr);
    if (!ctx->chain_ws) ctx->chain_ws = new (std::nothrow) rawdtw_chain_ws;
    if (!ctx->chain_ws) return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed");
    ChainWs &w = ctx->chain_ws->w;
    if (n_long) {
        try { w.long_reads.resize(n_long); } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
        uint64_t k = 0, at = 0;
        for (uint64_t r = 0; r < n_reads; r++) {
            const uint64_t nr = seed_off[r + 1] - seed_off[r];
            if (nr > seed_cap && nr <= long_cap) { w.long_reads[k++] = LongRead{(uint32_t)r, 0u, at}; at += (nr + 63) & ~63ull; }
        }
    }
    if (decline) { // the marks, and the host's copies of what the append needs after the caller's arrays may be gone
        try {
            w.marks.assign(n_reads, 0);
            w.h_read_base.assign(read_base, read_base + n_reads);
            w.h_key_base.assign(key_base, key_base + n_keys);
        } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
        for (uint64_t r = 0; r < n_reads; r++) {
            const uint64_t nr = seed_off[r + 1] - seed_off[r];
            w.marks[r] = nr > seed_cap && nr > long_cap;
        }
    }
    if (w.dev_bytes < need) {
        if (w.dev) (void)hipFree(w.dev);
        w.dev = nullptr; w.dev_bytes = 0;
        const size_t want = need + need / 4;
        if (hipMalloc(&w.dev, want) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, RAWDTW_ERR_OOM, "chaining workspace allocation failed"); }
        w.dev_bytes = want;
    }
    const size_t tot_bytes = (size_t)L.tot_words() * 8; // (64, as it was, until a round declines reads: 128)
    if (w.pin && w.pin_bytes < tot_bytes) { (void)hipHostFree(w.pin); w.pin = nullptr; }
    if (!w.pin && hipHostMalloc(&w.pin, tot_bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); w.pin = nullptr; return fail(ctx, RAWDTW_ERR_OOM, "pinned allocation failed"); }
    w.pin_bytes = std::max(w.pin_bytes, tot_bytes);
    (void)L.lay(w.dev);
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(L.soff, seed_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, s));
    if (res) { // only the previous anchors go up; rawdtw_seed.hip's writer puts them and the hits in place
        if (n_prev) HIP_TRY(ctx, hipMemcpyAsync(L.prev, res->prev_seeds, (size_t)n_prev * sizeof(rawdtw_seed_t), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(L.poff, res->prev_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(L.cs, res->chunk_start, n_reads * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(L.so, res->sits_out, n_reads, hipMemcpyHostToDevice, s));
        if (res->prev_src) HIP_TRY(ctx, hipMemcpyAsync(L.psrc, res->prev_src, n_reads * 4, hipMemcpyHostToDevice, s));
        // THE ORDER the store is read in: the keep launch that wrote a half (rawdtw_keep.hip, the round before) and this writer launch are both on
        // the context's stream, the keep first -- the half's count and seeds are complete when the writer reads them, and the count is the mirror's
        seed_resident_write_chain(ctx, L.seeds, L.soff, L.poff, L.prev, L.cs, L.so, res->prev_src ? L.psrc : nullptr);
        HIP_TRY(ctx, hipGetLastError());
    } else if (n_seeds) HIP_TRY(ctx, hipMemcpyAsync(L.seeds, seeds, (size_t)n_seeds * sizeof(rawdtw_seed_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(L.rb, read_base, n_reads * 4, hipMemcpyHostToDevice, s));
    if (n_keys) HIP_TRY(ctx, hipMemcpyAsync(L.kb, key_base, (size_t)n_keys * 8, hipMemcpyHostToDevice, s));
    // many chains a read: the scores and the order of a read's chains lie in LDS, 8 bytes a chain, for as many as the option and the launch's
    // largest read allow (k_chain: at most 2 048 / rec_div, 16 KiB behind 42 KiB of seeds; k_chain_long: at most 4 096, 32 KiB behind its ring)
    auto lds_chains = [&](const uint64_t seeds_most) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(max_chains, seeds_most / rec_div)); };
    ChainArgs a{L.soff, L.seeds, (uint32_t)n_reads, n2, *opt, L.tmpa, L.trec, L.cnt, (uint32_t)L.cap(), max_chains ? rec_div : 0u, L.by_seeds() ? 1u : 0u,
                max_chains ? lds_chains(most) : 0u, max_chains ? L.tperm : nullptr};
    const size_t lds = (size_t)n2 * 21 + 16;
    if (max_chains) hipLaunchKernelGGL(k_chain<true>, dim3((uint32_t)n_reads), dim3(64), lds + (size_t)a.lds_chains * 8, s, a);
    else hipLaunchKernelGGL(k_chain<false>, dim3((uint32_t)n_reads), dim3(64), lds, s, a);
    if (n_long) { // behind k_chain, which has flagged these reads as too long for it: the long launch writes their cnt over that
        HIP_TRY(ctx, hipMemcpyAsync(const_cast<LongRead *>(L.la.reads), w.long_reads.data(), n_long * sizeof(LongRead), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemsetAsync(L.la.far_steps, 0, 8, s));
        hipLaunchKernelGGL(k_chain_sort_long, dim3((uint32_t)n_long), dim3(256), 0, s, a, L.la);
        L.la.lds_chains = max_chains ? lds_chains(most_long) : 0u;
        if (max_chains) hipLaunchKernelGGL(k_chain_long<true>, dim3((uint32_t)n_long), dim3(64), (size_t)L.la.lds_chains * 8, s, a, L.la);
        else hipLaunchKernelGGL(k_chain_long<false>, dim3((uint32_t)n_long), dim3(64), 0, s, a, L.la);
    }
    const DeclArgs da{L.mark, L.why, L.dlist, L.soff};
    if (decline) {
        HIP_TRY(ctx, hipMemcpyAsync(L.mark, w.marks.data(), n_reads, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_chain_scan<true>, dim3(1), dim3(1024), 0, s, L.cnt, (uint32_t)n_reads, a.cap, L.coff, L.ra0, L.tot, da);
    } else hipLaunchKernelGGL(k_chain_scan<false>, dim3(1), dim3(1024), 0, s, L.cnt, (uint32_t)n_reads, a.cap, L.coff, L.ra0, L.tot, DeclArgs{});
    // the caller's arrays: written by the compaction launch itself when they are page-locked (rawdtw_host_alloc) -- no copy command, no second
    // wait for sizes only the device knows; else copied at the round's end
    const bool direct = page_locked(anchor_off) && page_locked(recs) && (!anchors || page_locked(anchors)) && page_locked(chain_off);
    if (decline)
        hipLaunchKernelGGL(k_chain_compact<true>, dim3((uint32_t)n_reads), dim3(64), 0, s, a, L.coff, L.ra0, L.rb, L.kb, n_keys, L.aoff, L.anch, L.refb, L.rbc, L.recs, L.tot,
                           direct ? anchor_off : nullptr, direct ? recs : nullptr, direct ? anchors : nullptr, chains_cap, L.why);
    else
        hipLaunchKernelGGL(k_chain_compact<false>, dim3((uint32_t)n_reads), dim3(64), 0, s, a, L.coff, L.ra0, L.rb, L.kb, n_keys, L.aoff, L.anch, L.refb, L.rbc, L.recs, L.tot,
                           direct ? anchor_off : nullptr, direct ? recs : nullptr, direct ? anchors : nullptr, chains_cap, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    uint64_t *h_tot = static_cast<uint64_t *>(w.pin);
    HIP_TRY(ctx, hipMemcpyAsync(h_tot, L.tot, tot_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(chain_off, L.coff, (n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    if (!w.done) HIP_TRY(ctx, hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventRecord(w.done, s));
    w.pending = true; w.direct = direct; w.n_reads = n_reads; w.chains_cap = chains_cap;
    w.n_long = n_long; w.many = max_chains != 0;
    w.st_rounds++; w.st_long_reads += n_long;
    for (uint64_t k = 0; k < n_long; k++) w.st_long_seeds += seed_off[w.long_reads[k].r + 1] - seed_off[w.long_reads[k].r];
    w.h_anchor_off = anchor_off; w.h_recs = recs; w.h_anchors = anchors;
    w.d_aoff = L.aoff; w.d_recs = L.recs; w.d_anch = L.anch; w.d_refb = L.refb; w.d_rbc = L.rbc;
    w.decline = decline; w.n_seeds = n_seeds; w.batch_room = L.batch_entries(); w.h_chain_off = chain_off;
    w.d_soff = L.soff; w.d_seeds = L.seeds; w.d_list = L.dlist;
    return RAWDTW_OK;
}

} // namespace

extern "C" {

int rawdtw_chain_round_begin(rawdtw_ctx *ctx, const rawdtw_chain_opt_t *opt, uint64_t n_reads, const uint64_t *seed_off, const rawdtw_seed_t *seeds,
                             const uint32_t *read_base, uint32_t n_keys, const uint64_t *key_base, uint64_t *chain_off, uint64_t *anchor_off,
                             rawdtw_chain_rec_t *recs, uint64_t chains_cap, rawdtw_anchor_t *anchors)
{
    return chain_begin(ctx, opt, n_reads, seed_off, seeds, nullptr, read_base, n_keys, key_base, chain_off, anchor_off, recs, chains_cap, anchors);
}

int rawdtw_chain_round_begin_resident(rawdtw_ctx *ctx, const rawdtw_chain_opt_t *opt, uint64_t n_reads, const uint64_t *seed_off, const uint64_t *prev_off,
                                      const rawdtw_seed_t *prev_seeds, const uint32_t *chunk_start, const uint8_t *sits_out, const uint32_t *read_base,
                                      uint32_t n_keys, const uint64_t *key_base, uint64_t *chain_off, uint64_t *anchor_off, rawdtw_chain_rec_t *recs,
                                      uint64_t chains_cap, rawdtw_anchor_t *anchors)
{
    const ResidentSeeds res{prev_off, prev_seeds, chunk_start, sits_out, nullptr};
    return chain_begin(ctx, opt, n_reads, seed_off, nullptr, &res, read_base, n_keys, key_base, chain_off, anchor_off, recs, chains_cap, anchors);
}

int rawdtw_chain_round_begin_resident_kept(rawdtw_ctx *ctx, const rawdtw_chain_opt_t *opt, uint64_t n_reads, const uint64_t *seed_off, const uint64_t *prev_off,
                                           const rawdtw_seed_t *prev_seeds, const uint32_t *prev_src, const uint32_t *chunk_start, const uint8_t *sits_out,
                                           const uint32_t *read_base, uint32_t n_keys, const uint64_t *key_base, uint64_t *chain_off, uint64_t *anchor_off,
                                           rawdtw_chain_rec_t *recs, uint64_t chains_cap, rawdtw_anchor_t *anchors)
{
    if (ctx && !prev_src) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    const ResidentSeeds res{prev_off, prev_seeds, chunk_start, sits_out, prev_src};
    return chain_begin(ctx, opt, n_reads, seed_off, nullptr, &res, read_base, n_keys, key_base, chain_off, anchor_off, recs, chains_cap, anchors);
}

int rawdtw_chain_round_end(rawdtw_ctx *ctx, const rawdtw_anchor_t **d_anchors, const uint64_t **d_ref_base, const uint32_t **d_read_base)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!d_anchors || !d_ref_base || !d_read_base) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (!ctx->chain_ws || !ctx->chain_ws->w.pending) return fail(ctx, RAWDTW_ERR_INVALID, "no chaining round begun on this context");
    ChainWs &w = ctx->chain_ws->w;
    w.pending = false;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipEventSynchronize(w.done)); // (the round's own work: what was enqueued behind it -- the caller's next uploads -- goes on)
    const uint64_t *h_tot = static_cast<const uint64_t *>(w.pin);
    const uint64_t nc = h_tot[0], na = h_tot[1], flags = h_tot[2];
    if (w.n_long) w.st_far_steps += h_tot[4];
    if (h_tot[3]) return fail(ctx, RAWDTW_ERR_INVALID, "a seed's key is not below n_keys");
    if (flags) return fail(ctx, RAWDTW_ERR_UNSUPPORTED, w.many ? "a read with more chains than \"chain_max_chains\" allows: chain this round on the host"
                                                        : flags & 4 ? "a read with more than 16 chains, two of them with equal scores: chain this round on the host, or set \"chain_max_chains\""
                                                                    : "a read with more than 32 chains (or more seeds than the device chains): chain this round on the host, or set \"chain_max_chains\"");
    w.st_above_32 += h_tot[5]; w.st_max_chains = std::max<uint64_t>(w.st_max_chains, h_tot[7]);
    if (w.many) w.st_restated += h_tot[6];
    if (nc > w.chains_cap) return fail(ctx, RAWDTW_ERR_RANGE, "chain output arrays too small");
    if (w.decline) { // the declined reads, ascending, with their reasons and where their seeds start among the declined reads' seeds
        const uint64_t nd = h_tot[8];
        if (nd > w.n_reads) return fail(ctx, RAWDTW_ERR_DEVICE, "the chaining's count of declined reads is not one of this round");
        try { w.decl.resize(nd); w.decl_reads.resize(nd); w.decl_why.resize(nd); w.decl_seed0.resize(nd + 1); }
        catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
        if (nd) {
            HIP_TRY(ctx, hipMemcpyAsync(w.decl.data(), w.d_list, nd * sizeof(DeclRec), hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
        }
        for (uint64_t j = 0; j < nd; j++) { w.decl_reads[j] = w.decl[j].r; w.decl_why[j] = w.decl[j].why; w.decl_seed0[j] = w.decl[j].seed0; }
        w.decl_seed0[nd] = w.decl_seeds = h_tot[12];
        w.nc = nc; w.na = na;
    }
    if (!w.direct) {
        HIP_TRY(ctx, hipMemcpyAsync(w.h_anchor_off, w.d_aoff, (nc + 1) * 8, hipMemcpyDeviceToHost, s));
        if (nc) HIP_TRY(ctx, hipMemcpyAsync(w.h_recs, w.d_recs, nc * sizeof(rawdtw_chain_rec_t), hipMemcpyDeviceToHost, s));
        if (w.h_anchors && na) HIP_TRY(ctx, hipMemcpyAsync(w.h_anchors, w.d_anch, na * sizeof(rawdtw_anchor_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    *d_anchors = w.d_anch; *d_ref_base = w.d_refb; *d_read_base = w.d_rbc;
    w.ended = w.appendable = w.decline;
    return RAWDTW_OK;
}

int rawdtw_chain_round_declined(rawdtw_ctx *ctx, uint64_t *n_declined, const uint32_t **reads, const uint32_t **why)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!n_declined) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    *n_declined = 0;
    if (reads) *reads = nullptr;
    if (why) *why = nullptr;
    if (!ctx->chain_ws) return RAWDTW_OK;
    const ChainWs &w = ctx->chain_ws->w;
    if (w.pending) return fail(ctx, RAWDTW_ERR_INVALID, "a chaining round is begun on this context and not ended");
    if (!w.ended) return RAWDTW_OK; // (the option was off, or the round's end failed: nobody was declined alone)
    *n_declined = w.decl_reads.size();
    if (reads) *reads = w.decl_reads.data();
    if (why) *why = w.decl_why.data();
    return RAWDTW_OK;
}

int rawdtw_chain_round_declined_seeds(rawdtw_ctx *ctx, uint64_t *seed_off_out, rawdtw_seed_t *seeds_out, uint64_t cap)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!seed_off_out || (!seeds_out && cap)) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (!ctx->chain_ws || ctx->chain_ws->w.pending || !ctx->chain_ws->w.ended)
        return fail(ctx, RAWDTW_ERR_INVALID, "no ended chaining round with \"chain_decline_reads\" on this context");
    ChainWs &w = ctx->chain_ws->w;
    const uint64_t nd = w.decl_reads.size(), total = w.decl_seeds;
    memcpy(seed_off_out, w.decl_seed0.data(), (nd + 1) * 8);
    if (total > cap) return fail(ctx, RAWDTW_ERR_RANGE, "the declined reads' seeds do not fit the array (the offsets are filled)");
    if (nd == 0 || total == 0) return RAWDTW_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    rawdtw_seed_t *dst = seeds_out;
    if (!page_locked(seeds_out)) { // through page-locked memory of the workspace's own, grow-only
        const size_t need = (size_t)total * sizeof(rawdtw_seed_t);
        if (w.pin_seeds_bytes < need) {
            if (w.pin_seeds) (void)hipHostFree(w.pin_seeds);
            w.pin_seeds = nullptr; w.pin_seeds_bytes = 0;
            if (hipHostMalloc(&w.pin_seeds, need + need / 4, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); w.pin_seeds = nullptr; return fail(ctx, RAWDTW_ERR_OOM, "pinned allocation failed"); }
            w.pin_seeds_bytes = need + need / 4;
        }
        dst = static_cast<rawdtw_seed_t *>(w.pin_seeds);
    }
    hipLaunchKernelGGL(k_declined_seeds, dim3((uint32_t)nd), dim3(64), 0, s, w.d_list, w.d_soff, w.d_seeds, dst);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (dst != seeds_out) memcpy(seeds_out, dst, (size_t)total * sizeof(rawdtw_seed_t));
    return RAWDTW_OK;
}

int rawdtw_chain_round_append(rawdtw_ctx *ctx, uint64_t n_declined, const uint64_t *chain_off, const rawdtw_chain_rec_t *recs, const uint64_t *anchor_off,
                              const rawdtw_anchor_t *anchors, uint64_t *chain_off_ext, uint64_t *anchor_off_ext, const rawdtw_anchor_t **d_anchors,
                              const uint64_t **d_ref_base, const uint32_t **d_read_base)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!chain_off || !anchor_off || !chain_off_ext || !anchor_off_ext || !d_anchors || !d_ref_base || !d_read_base) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    if (!ctx->chain_ws || ctx->chain_ws->w.pending || !ctx->chain_ws->w.appendable)
        return fail(ctx, RAWDTW_ERR_INVALID, "no ended chaining round with \"chain_decline_reads\" on this context that waits for its declined reads' chains");
    ChainWs &w = ctx->chain_ws->w;
    if (n_declined != w.decl_reads.size()) return fail(ctx, RAWDTW_ERR_INVALID, "the appended reads are not the round's declined reads");
    const uint64_t nc0 = w.nc, na0 = w.na;
    // every check before the first write
    for (uint64_t j = 0; j < n_declined; j++) if (chain_off[j + 1] < chain_off[j]) return fail(ctx, RAWDTW_ERR_INVALID, "offsets do not ascend");
    const uint64_t nca = chain_off[n_declined];
    if ((nca && (!recs || !anchors))) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    for (uint64_t c = 0; c < nca; c++) {
        if (anchor_off[c + 1] < anchor_off[c] || anchor_off[c + 1] - anchor_off[c] != recs[c].n_anchors) return fail(ctx, RAWDTW_ERR_INVALID, "a chain's anchor_off stretch is not its record's n_anchors");
        if (recs[c].key >= w.h_key_base.size()) return fail(ctx, RAWDTW_ERR_INVALID, "a seed's key is not below n_keys");
    }
    // room: the workspace's batch arrays (ChainLayout: what the round's seeds can make) -- the caller sized chain_off_ext and anchor_off_ext itself
    const int st = chain_append::extend_offsets(w.n_reads, w.h_chain_off, w.h_anchor_off, nc0, na0, n_declined, chain_off, anchor_off, w.batch_room, w.n_seeds,
                                                chain_off_ext, anchor_off_ext);
    if (st == chain_append::kBadOffsets) return fail(ctx, RAWDTW_ERR_INVALID, "offsets do not start at 0, or the round's chain_off / anchor_off are no longer the round's");
    if (st == chain_append::kNoRoom) return fail(ctx, RAWDTW_ERR_RANGE, "more chains or anchors than the round's seeds can make");
    const uint64_t naa = anchor_off[nca];
    try { w.app_refb.resize(nca); w.app_rbc.resize(nca); } catch (const std::bad_alloc &) { return fail(ctx, RAWDTW_ERR_OOM, "host allocation failed"); }
    for (uint64_t j = 0; j < n_declined; j++)
        for (uint64_t c = chain_off[j]; c < chain_off[j + 1]; c++) { w.app_refb[c] = w.h_key_base[recs[c].key]; w.app_rbc[c] = w.h_read_base[w.decl_reads[j]]; }
    w.appendable = false;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint64_t *>(w.d_aoff) + nc0, anchor_off_ext + nc0, (nca + 1) * 8, hipMemcpyHostToDevice, s));
    if (nca) {
        HIP_TRY(ctx, hipMemcpyAsync(const_cast<rawdtw_chain_rec_t *>(w.d_recs) + nc0, recs, nca * sizeof(rawdtw_chain_rec_t), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint64_t *>(w.d_refb) + nc0, w.app_refb.data(), nca * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint32_t *>(w.d_rbc) + nc0, w.app_rbc.data(), nca * 4, hipMemcpyHostToDevice, s));
    }
    if (naa) HIP_TRY(ctx, hipMemcpyAsync(const_cast<rawdtw_anchor_t *>(w.d_anch) + na0, anchors, naa * sizeof(rawdtw_anchor_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s)); // (the caller's arrays and the workspace's staging are free again)
    w.nc = nc0 + nca; w.na = na0 + naa;
    *d_anchors = w.d_anch; *d_ref_base = w.d_refb; *d_read_base = w.d_rbc;
    return RAWDTW_OK;
}

int rawdtw_chain_round_recs(rawdtw_ctx *ctx, const rawdtw_chain_rec_t **d_recs)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    if (!d_recs) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    *d_recs = nullptr;
    if (!ctx->chain_ws || ctx->chain_ws->w.pending || !ctx->chain_ws->w.d_recs) return fail(ctx, RAWDTW_ERR_INVALID, "no ended chaining round on this context");
    *d_recs = ctx->chain_ws->w.d_recs;
    return RAWDTW_OK;
}

int rawdtw_chain_round_stats(const rawdtw_ctx *ctx, uint64_t *rounds, uint64_t *long_reads, uint64_t *long_seeds, uint64_t *far_steps)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    const ChainWs none;
    const ChainWs &w = ctx->chain_ws ? ctx->chain_ws->w : none;
    if (rounds) *rounds = w.st_rounds;
    if (long_reads) *long_reads = w.st_long_reads;
    if (long_seeds) *long_seeds = w.st_long_seeds;
    if (far_steps) *far_steps = w.st_far_steps;
    return RAWDTW_OK;
}

int rawdtw_chain_order_stats(const rawdtw_ctx *ctx, uint64_t *reads_above_32, uint64_t *reads_ordered_restated, uint64_t *max_chains_a_read)
{
    if (!ctx) return RAWDTW_ERR_INVALID;
    const ChainWs none;
    const ChainWs &w = ctx->chain_ws ? ctx->chain_ws->w : none;
    if (reads_above_32) *reads_above_32 = w.st_above_32;
    if (reads_ordered_restated) *reads_ordered_restated = w.st_restated;
    if (max_chains_a_read) *max_chains_a_read = w.st_max_chains;
    return RAWDTW_OK;
}

int rawdtw_chain_round(rawdtw_ctx *ctx, const rawdtw_chain_opt_t *opt, uint64_t n_reads, const uint64_t *seed_off, const rawdtw_seed_t *seeds,
                       const uint32_t *read_base, uint32_t n_keys, const uint64_t *key_base, uint64_t *chain_off, uint64_t *anchor_off,
                       rawdtw_chain_rec_t *recs, uint64_t chains_cap, rawdtw_anchor_t *anchors, const rawdtw_anchor_t **d_anchors,
                       const uint64_t **d_ref_base, const uint32_t **d_read_base)
{
    if (ctx && (!d_anchors || !d_ref_base || !d_read_base)) return fail(ctx, RAWDTW_ERR_INVALID, "null argument");
    const int st = rawdtw_chain_round_begin(ctx, opt, n_reads, seed_off, seeds, read_base, n_keys, key_base, chain_off, anchor_off, recs, chains_cap, anchors);
    return st == RAWDTW_OK ? rawdtw_chain_round_end(ctx, d_anchors, d_ref_base, d_read_base) : st;
}

} // extern "C"

namespace rawdtw { namespace capi {
bool chain_kept_view(const rawdtw_ctx *ctx, ChainKeptView *v)
{
    if (!ctx || !ctx->chain_ws || ctx->chain_ws->w.pending || !ctx->chain_ws->w.d_recs) return false;
    v->d_recs = ctx->chain_ws->w.d_recs; v->d_aoff = ctx->chain_ws->w.d_aoff; v->d_anch = ctx->chain_ws->w.d_anch;
    return true;
}
void chain_ws_free(rawdtw_ctx *ctx)
{
    if (!ctx || !ctx->chain_ws) return;
    if (ctx->chain_ws->w.dev) (void)hipFree(ctx->chain_ws->w.dev);
    if (ctx->chain_ws->w.pin) (void)hipHostFree(ctx->chain_ws->w.pin);
    if (ctx->chain_ws->w.pin_seeds) (void)hipHostFree(ctx->chain_ws->w.pin_seeds);
    if (ctx->chain_ws->w.done) (void)hipEventDestroy(ctx->chain_ws->w.done);
    delete ctx->chain_ws;
    ctx->chain_ws = nullptr;
}
} }
