// rawdtw_mapper.cpp -- the chunk-round mapping loop on the library's host side (include/rawdtw.h, rawdtw_mapper_*).
//
// What it restates: the control flow of map_worker_for / ri_map_frag / gen_chains (src/rmap.cpp:667-822, 545-578, 315-541)
// turned inside out so that every chunk round makes ONE device submission per read group (option A), and the
// PAF line of a read (src/rmap.cpp:696-801, 950-965).
//
// A round, per read group (the reads are dealt over one or two groups, each with a context of its own):
//   host phase   a pool of threads over the group's reads, as the reference runs kt_for over n_threads reads
//                (rmap.cpp:916): append the chunk's events (rmap.cpp:554-567), re-seed with the previous chains' anchors plus the
//                chunk's seed hits (344-391), sort (396-401), the chaining DP per (sequence, strand) (430-507:
//                rawdtw_chain_anchors), evaluation order (512), and -- chunk rounds with carry -- per chain the chain of the
//                round before it continues and the number of leading parts that did not change, compared anchor by anchor
//   lay-out      the round's arrays in pinned memory: chain and anchor offsets, bases, the NEW anchors and the carry records
//                (or the whole lists for a round without a predecessor), the new events' segments
//   submit       rawdtw_events_append + rawdtw_batch_submit_carry / rawdtw_batch_submit: enqueued, not waited for
// then, group by group: fetch (the only wait), and the round's end per read on the pool: gen_primary_chains, comp_mapq, the
// stop rule (532-541, 692), into the round's own state -- the commit after the last group is the one place it reaches the reads.
// With two groups one group's host phase runs while the other's batch is on the device, and one group's round end while the
// other's batch finishes -- the overlap the reference gets from its two pipeline workers (rmap.cpp:1015,1033).
//
// Event detection and seeding stay in RawAlign (revent.c, rsketch.c, rawindex.cpp): the caller hands in each chunk's events
// and seed hits.  rawalign_amd/mapper.py is the Python mirror of the control flow; tests/test_mapper.py and
// tests/test_abi_shim.py compare the two and the oracle-scored flow line by line.  Pure host code above the C ABI: no kernel
// is launched from here directly.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/rawdtw.h"

namespace {

struct MChain {
    float chaining_score = 0.f, alignment_score = 0.f;
    uint32_t ref = 0;
    int32_t strand = 0;
    uint32_t start_position = 0, end_position = 0, mapq = 0;
    std::vector<rawdtw_anchor_t> anchors; // end-first (rmap.cpp:193-196)
    std::string aln;                      // aln:s: of the best chain (--dtw-output-cigar)
    bool has_aln = false;
};

struct MRead {
    std::string name;
    uint32_t qlen = 0, n_chunks = 0, chunks_done = 0;
    bool finished = false, broke_early = false, released = false;
    std::vector<float> events;   // p->events[read].values -- the host's copy: kept for what reads it (an external scorer, --dtw-output-cigar's
                                 // traceback at the end); a mapper that only scores on the device keeps the count (the events are in the arena)
    uint32_t n_events = 0;
    uint32_t offset = 0;         // reg->offset: events of the chunks that were chained (rmap.cpp:574; a chunk below min_events does not count)
    std::vector<MChain> chains;  // reg0->chains: the primary chains, best first
    uint32_t slot = 0;           // its place in the mapper's event arenas: group = slot % groups, place there = slot / groups
    uint64_t last_round = 0;     // the round it was last scored in, and its position among its group's reads then
    uint64_t last_pos = 0;
    uint64_t seen_round = 0;     // (duplicate check)
    bool closed = false;         // sequence-until: in a closed mini-batch
    // "resident_chains": the half of its slot in the context's store of kept chains that holds its chains' anchors as seeds (rawdtw_keep.hip),
    // and how many.  Written in a round's commit block only; cleared wherever the chains change without a keep launch behind them.
    struct Kept { bool valid = false; uint8_t half = 0; uint32_t count = 0; } kept;
    bool gated = false;          // ... at or after the stop point of its batch (rmap.cpp:960: a mapped read's line loses its fields)
    bool dropped = false;        // ... added but in no closed batch when the stop fired, or added after it: finished, no line
    bool host_only = false;      // some of its events never reached the arena: a round that ran nothing on the device (no DTW stage and the chains
                                 // made on the host, an external scorer, no context) -- the host's copy is then complete up to that round
};

// growable array in page-locked memory (plain memory for a mapper without a device); contents are NOT kept over a growth
template <typename T> struct PinBuf {
    T *p = nullptr;
    size_t cap = 0;
    bool pinned = false;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    PinBuf &operator=(PinBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(pinned, o.pinned); return *this; }
    ~PinBuf() { release(); }
    void release()
    {
        if (p) { if (pinned) rawdtw_host_free(p); else free(p); }
        p = nullptr; cap = 0;
    }
    // (`keep`: the first `keep` elements survive a move)
    bool ensure(size_t n, bool want_pinned, size_t keep = 0)
    {
        if (n <= cap) return true;
        const size_t c = n + n / 4 + 64;
        void *q = nullptr;
        bool pin = false;
        if (want_pinned && rawdtw_host_alloc(c * sizeof(T), &q) == RAWDTW_OK && q) pin = true;
        else q = malloc(c * sizeof(T));
        if (!q) return false;
        if (p && keep) memcpy(q, p, std::min(keep, cap) * sizeof(T));
        release();
        p = static_cast<T *>(q); cap = c; pinned = pin;
        return true;
    }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
};

// one round's arrays of one read group, as handed to the device (and kept for the next round's matching)
struct RoundArrays {
    std::vector<uint32_t> ks;  // the group's reads: indices into the round's read list, in order
    PinBuf<uint64_t> chain_off, anchor_off, ref_base, new_off, seg_src;
    PinBuf<uint32_t> read_base, seg_dst;
    PinBuf<rawdtw_anchor_t> anchors, new_anchors;
    PinBuf<rawdtw_carry_t> carry;
    PinBuf<float> new_events, score;
    PinBuf<uint8_t> keep;
    PinBuf<uint64_t> seed_off;           // device chaining (opt.device_chain): the reads' seed lists in, the chains' records out
    PinBuf<rawdtw_seed_t> seeds;
    PinBuf<rawdtw_chain_rec_t> recs;
    PinBuf<uint64_t> prev_off, ev_start;  // a resident round (rawdtw_mapper_round_seeded_resident): the previous anchors' offsets (the anchors themselves, dense, in
    PinBuf<uint32_t> chunk_start, ev_len; // `seeds`), the chunks' places in the event arena, and what the device's writer needs per read
    PinBuf<uint8_t> sits_out;
    PinBuf<uint32_t> prev_src, keep_dst, kept_count; // "resident_chains": per read where its previous seeds come from, where its chains are kept, and what was kept
    PinBuf<rawdtw_round_out_t> re_out;    // the round's end from the device ("device_round_end"): per read, and per chain the primaries' indices
    PinBuf<uint32_t> re_primary;
    PinBuf<uint64_t> chain_off_ext, anchor_off_ext; // "chain_decline_reads", a round that declined reads: the batch's read list -- the group's reads, then a pseudo-read
                                          // for each declined read -- and the chains' anchor offsets with the host's chains behind the device's; grown on demand
    std::vector<uint32_t> chain_seq; // (the external scorer's view)
    std::vector<int32_t> chain_strand;
    uint64_t n_reads = 0, n_chains = 0, n_anchors = 0; // (the sizes the next round's matching reads again)
    uint64_t n_reads_batch = 0;          // the reads of the round's batch: n_reads, and with "chain_decline_reads" the declined reads' pseudo-reads
    rawdtw_batch *batch = nullptr;
    uint64_t round_id = 0;
    bool carried = false;
};

struct Group {
    rawdtw_ctx *ctx = nullptr;
    bool own_ctx = false;
    RoundArrays buf[2];
    int cur = 0;          // buf[cur]: the round at hand; buf[cur ^ 1]: the round before (when has_prev)
    bool has_prev = false;
    // the largest round so far: BOTH buffers are sized to it when it grows (page-locked memory is slow to get -- ~0.2 ms a megabyte --, and a
    // round that is the first of its size in ITS buffer would pay that again one round after its neighbour did)
    uint64_t hw_reads = 0, hw_chains = 0, hw_anchors = 0, hw_new = 0, hw_events = 0, hw_seg = 0, hw_seeds = 0;
};

// what a round leaves per read until its commit (the host phase, the round's end)
struct RoundRead {
    std::vector<MChain> chains;          // the round's candidate chains in evaluation order
    std::vector<rawdtw_carry_t> carry;   // per chain
    std::vector<uint64_t> ref_base;      // per chain
    std::vector<MChain> primary;         // the round's end: its primary chains, best first (rd.chains at the commit)
    std::string log;
    uint64_t ne = 0;
    uint32_t ev_before = 0, off_before = 0;
    bool skipped = false;                // a chunk below min_events: no chaining, chains and offset stay (rmap.cpp:569-575)
    bool high = false;                   // the round's end: mapped with high confidence (rmap.cpp:692)
    uint64_t chain0 = 0, anchor0 = 0, new0 = 0, ev0 = 0; // its first chain / anchor / new anchor / new event in the group's arrays
    uint64_t seed0 = 0, n_seeds = 0;     // device chaining: its seeds in the group's list
    uint32_t chunk_start = 0;
    bool from_store = false;             // "resident_chains": its previous seeds were taken from the store of kept chains
    uint64_t n_prev = 0;                 // ... and how many it had, from either side
    bool declined = false;               // "chain_decline_reads": the device chaining declined it alone; its chains are the host's, behind the device's
    uint64_t bpos = 0;                   // its read in the group's batch: its position, or a declined read's pseudo-read behind the group's reads
    int err = RAWDTW_OK;
};

// a pool of threads running one loop at a time; the calling thread works too
class Pool {
public:
    explicit Pool(int threads)
    {
        for (int t = 1; t < threads; t++) th_.emplace_back([this] { worker(); });
    }
    ~Pool()
    {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; gen_.fetch_add(1, std::memory_order_release); }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    // fn(i) for i in [0, n), dealt in pieces of `grain` from a shared counter (as kt_for deals reads: kthread.c:54-72).
    // A round is half a dozen such loops a few hundred microseconds apart: a worker that has run out of work keeps looking for the next loop
    // for a short while before it goes to sleep, and the caller for the last worker -- waking sixteen threads through a condition variable
    // was 50-100 us a loop, most of a small round.
    void run(size_t n, size_t grain, const std::function<void(size_t)> &fn)
    {
        if (n == 0) return;
        if (th_.empty() || n <= grain) { for (size_t i = 0; i < n; i++) fn(i); return; }
        fn_ = &fn; n_ = n; grain_ = grain; next_.store(0, std::memory_order_relaxed);
        busy_.store((int)th_.size(), std::memory_order_relaxed);
        gen_.fetch_add(1, std::memory_order_release);
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (sleeping_ > 0) cv_.notify_all();
        }
        work();
        const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(2000);
        while (busy_.load(std::memory_order_acquire) != 0) {
            if (std::chrono::steady_clock::now() > until) {
                std::unique_lock<std::mutex> lk(mu_);
                waiting_ = true;
                done_.wait(lk, [this] { return busy_.load(std::memory_order_acquire) == 0; });
                waiting_ = false;
                break;
            }
            relax();
        }
        fn_ = nullptr;
    }
    int threads() const { return (int)th_.size() + 1; }

private:
    static void relax()
    {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#else
        std::this_thread::yield();
#endif
    }
    void work()
    {
        for (;;) {
            const size_t s = next_.fetch_add(grain_);
            if (s >= n_) break;
            const size_t e = std::min(n_, s + grain_);
            for (size_t i = s; i < e; i++) (*fn_)(i);
        }
    }
    void worker()
    {
        uint64_t seen = 0;
        for (;;) {
            uint64_t g = gen_.load(std::memory_order_acquire);
            if (g == seen) { // nothing yet: look for a while, then sleep
                const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(200);
                while ((g = gen_.load(std::memory_order_acquire)) == seen && std::chrono::steady_clock::now() < until) relax();
                if (g == seen) {
                    std::unique_lock<std::mutex> lk(mu_);
                    sleeping_++;
                    cv_.wait(lk, [&] { return gen_.load(std::memory_order_acquire) != seen; });
                    sleeping_--;
                    g = gen_.load(std::memory_order_acquire);
                }
            }
            seen = g;
            if (stop_) return;
            work();
            if (busy_.fetch_sub(1, std::memory_order_acq_rel) == 1) {
                std::lock_guard<std::mutex> lk(mu_);
                if (waiting_) done_.notify_one();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(size_t)> *fn_ = nullptr;
    size_t n_ = 0, grain_ = 1;
    std::atomic<size_t> next_{0};
    std::atomic<int> busy_{0};
    std::atomic<uint64_t> gen_{0};
    int sleeping_ = 0;      // (under mu_)
    bool waiting_ = false;  // (under mu_) the caller sleeps on done_
    std::atomic<bool> stop_{false};
};

rawdtw_chain_t record_of(const MChain &c, uint32_t tag)
{
    return rawdtw_chain_t{c.chaining_score, c.alignment_score, c.ref, c.start_position, c.end_position, (uint32_t)c.anchors.size(), c.strand, 0u, tag};
}

std::string fmt_f(double x) // std::to_string(float/double) == printf("%f")
{
    char b[64];
    snprintf(b, sizeof b, "%f", x);
    return b;
}

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

} // namespace

struct rawdtw_mapper {
    rawdtw_ctx *ctx = nullptr;
    rawdtw_mapper_opt_t opt{};
    std::vector<std::string> seq_names;
    std::vector<uint32_t> seq_len;
    std::vector<uint64_t> ref_off; // [seq * 2 + strand]: the strand array's offset in the reference arena (a scorer-only mapper: its index)
    std::vector<MRead> reads;
    std::vector<uint32_t> free_slots;
    uint32_t slots_used = 0;
    Group groups_store[2];
    struct GroupSpan { Group *b; size_t n; Group *begin() const { return b; } Group *end() const { return b + n; } size_t size() const { return n; } Group &operator[](size_t i) const { return b[i]; } } groups{groups_store, 1};
    Pool *pool = nullptr;
    std::string log;
    uint64_t rounds = 0, parts_scored = 0, parts_reused = 0;
    double timing[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    rawdtw_scorer_fn scorer = nullptr;
    void *scorer_user = nullptr;
    bool keep_host_events = true; // (false: scored on the device only and no CIGAR asked for -- nothing reads the host's copy of a read's events)
    std::string err;
    rawdtw_su *su = nullptr;      // sequence-until (flag 0x1 or rawdtw_mapper_set_sequence_until): the state su_batch feeds
    bool su_closed_any = false;   // a batch has been closed (the parameters are fixed from then on)
    bool su_stopped = false;
    uint32_t su_mapped = 0;       // mapped reads of closed batches before the gate
    // rawdtw_mapper_round_seeded: the round's hits, page-locked when the mapper has a context (the device writes them itself: seed_room)
    PinBuf<uint64_t> seed_off;
    PinBuf<rawdtw_seed_hit_t> seed_hits;
    // rawdtw_mapper_round_seeded_resident (rawdtw_mapper_resident_stats)
    uint64_t res_rounds = 0, res_fallbacks = 0, res_hit_bytes = 0, res_seed_bytes = 0;
    // rawdtw_mapper_round_signal_resident / _raw_resident (rawdtw_mapper_signal_stats): the round's tables, the counts that come home
    PinBuf<uint64_t> sig_dst;
    PinBuf<uint32_t> sig_room, sig_evlen;
    std::vector<uint64_t> sig_evoff;
    uint64_t sig_rounds = 0, sig_retried = 0, sig_sample_bytes = 0;
    uint64_t re_rounds = 0, re_reads = 0, re_declined = 0; // rawdtw_mapper_round_end_stats
    // rawdtw_mapper_kept_stats ("resident_chains"): reads with previous seeds taken from the device / sent up from the host, those seeds, and
    // reads whose chains a keep launch did not keep; the store's N as this mapper reserved it
    uint64_t kp_reads_dev = 0, kp_reads_host = 0, kp_seeds_dev = 0, kp_seeds_host = 0, kp_not_kept = 0;
    uint32_t kp_reserved = 0;
    bool kp_any = false; // some read may hold kept chains
    // rawdtw_mapper_decline_stats ("chain_decline_reads"): rounds in which the device chaining declined reads alone, those reads by reason, the reads
    // it chained in such rounds' place of a fall-back or not, and the declined reads' seeds a resident round brought home
    uint64_t dc_rounds = 0, dc_reads_seeds = 0, dc_reads_chains = 0, dc_reads_device = 0, dc_seed_bytes = 0;
    PinBuf<uint64_t> decl_soff;     // the declined reads' seeds from the device (rawdtw_chain_round_declined_seeds), page-locked
    PinBuf<rawdtw_seed_t> decl_seeds;
    uint64_t sig_cap = 0; // the largest events_cap a round from signal ran with: what the seeding's workspace holds already
    bool arena_replaced = false;    // rawdtw_mapper_finish has uploaded the host's copies over the event arena: no slot holds its read's events any more
    bool finish_from_arena = false; // "signal_cigar": a --dtw-output-cigar mapper has committed a round from signal -- the host's copy of a read's
                                    // events is incomplete from then on, and rawdtw_mapper_finish reads every read's events in its slot of the arena
};

namespace {

rawdtw_select_opt_t select_opt(const rawdtw_mapper *m)
{
    return rawdtw_select_opt_t{(m->opt.flag & 0x2) ? 1 : 0, m->opt.min_bestmap_ratio, m->opt.min_meanmap_ratio, m->opt.min_chain_anchor};
}

// gen_primary_chains + comp_mapq over `post` (rmap.cpp:532-536): the primary chains, best first
std::vector<MChain> primary_chains(const rawdtw_mapper *m, std::vector<MChain> &post)
{
    std::vector<MChain> out;
    if (post.empty()) return out;
    static thread_local std::vector<rawdtw_chain_t> rec; // (scratch of the pool's threads: a round calls this once a read)
    static thread_local std::vector<uint32_t> kept;
    rec.resize(post.size()); kept.resize(post.size());
    for (size_t k = 0; k < post.size(); k++) rec[k] = record_of(post[k], (uint32_t)k);
    const rawdtw_select_opt_t so = select_opt(m);
    const uint32_t nk = rawdtw_gen_primary_chains(rec.data(), (uint32_t)rec.size(), &so, kept.data());
    out.reserve(nk);
    for (uint32_t k = 0; k < nk; k++) out.push_back(std::move(post[rec[kept[k]].tag]));
    if (nk) out[0].mapq = rec[kept[0]].mapq;
    return out;
}

bool high_confidence(const rawdtw_mapper *m, const std::vector<MChain> &primary)
{
    if (primary.empty()) return false;
    static thread_local std::vector<rawdtw_chain_t> rec;
    rec.resize(primary.size());
    for (size_t k = 0; k < primary.size(); k++) rec[k] = record_of(primary[k], (uint32_t)k);
    const rawdtw_select_opt_t so = select_opt(m);
    return rawdtw_is_mapped_with_high_confidence(rec.data(), (uint32_t)rec.size(), &so) != 0;
}

int fail(rawdtw_mapper *m, int st, const std::string &msg)
{
    if (m) m->err = msg;
    return st;
}

// room for `count` records in one of the seeding's buffers (contents are not kept).  With a context the device writes into them: page-locked,
// or no room -- PinBuf's fall-back to plain memory does not reach them.
template <typename T> bool seed_room(const rawdtw_mapper *m, PinBuf<T> &b, uint64_t count)
{
    return b.ensure(count, m->ctx != nullptr) && (b.pinned || !m->ctx);
}

void drop_batches(rawdtw_mapper *m) // (and with them what a round could carry from)
{
    for (Group &g : m->groups) {
        for (RoundArrays &ra : g.buf) {
            if (ra.batch) rawdtw_batch_destroy(ra.batch);
            ra.batch = nullptr;
        }
        g.has_prev = false;
    }
}

// a read's seeds for the round, unsorted: the previous chains' anchors (rmap.cpp:344-357), then the chunk's seed hits with their query
// positions from the chunk's start (371-391)
uint64_t seed_count(const MRead &rd, uint64_t n_hits)
{
    for (const MChain &ch : rd.chains) n_hits += ch.anchors.size();
    return n_hits;
}

void write_seeds(const MRead &rd, const rawdtw_seed_hit_t *hits, uint64_t n_hits, uint32_t chunk_start, rawdtw_seed_t *out)
{
    for (const MChain &ch : rd.chains)
        for (const rawdtw_anchor_t &a : ch.anchors) *out++ = rawdtw_seed_t{ch.ref * 2u + (uint32_t)ch.strand, a.target_position, a.query_position};
    for (uint64_t h = 0; h < n_hits; h++)
        *out++ = rawdtw_seed_t{hits[h].ref_seq * 2u + (uint32_t)(hits[h].strand ? 1 : 0), hits[h].target_position, hits[h].query_position + chunk_start};
}

// The host phase of one read after its events: the round's anchors, chaining, evaluation order, carry records -- the round's chains
// in rr.chains.  `pv` = the arrays of the round before of the read's group (null: none, or the read was not in it).
void host_chain_seeds(rawdtw_mapper *m, RoundRead &rr, std::vector<rawdtw_seed_t> &seeds, bool runs_dtw);
void host_phase_carry(const MRead &rd, RoundRead &rr, const RoundArrays *pv);

void host_phase_chain(rawdtw_mapper *m, const MRead &rd, RoundRead &rr, const rawdtw_seed_hit_t *hits, uint64_t n_hits, const RoundArrays *pv, bool runs_dtw)
{
    std::vector<rawdtw_seed_t> seeds(seed_count(rd, n_hits));
    write_seeds(rd, hits, n_hits, rr.chunk_start, seeds.data());
    host_chain_seeds(m, rr, seeds, runs_dtw);
    if (rr.err != RAWDTW_OK || !runs_dtw || !pv) return;
    host_phase_carry(rd, rr, pv);
}

// a read's seeds, in any order, to its round's chains in evaluation order (rr.chains, rr.ref_base): what host_phase_chain does with the seeds
// it builds, and what a round does with the seeds of a read the device chaining declined alone ("chain_decline_reads") -- one code, the same chains
void host_chain_seeds(rawdtw_mapper *m, RoundRead &rr, std::vector<rawdtw_seed_t> &seeds, bool runs_dtw)
{
    // by (sequence, strand), then (target, query): rmap.cpp:396-401 sorts every list; rmap.cpp:432-433 walks them sequence-major,
    // strand 0 then 1
    std::sort(seeds.begin(), seeds.end(), [](const rawdtw_seed_t &a, const rawdtw_seed_t &b) {
        return std::tie(a.key, a.target_position, a.query_position) < std::tie(b.key, b.target_position, b.query_position);
    });
    std::vector<MChain> chains;
    float maxs = 0.0f;
    const uint32_t cap = (uint32_t)std::max(1, m->opt.chain.num_best_chains);
    std::vector<rawdtw_chain_out_t> outc(cap);
    std::vector<uint64_t> off(cap + 1);
    std::vector<rawdtw_anchor_t> a, outa;
    for (size_t s0 = 0; s0 < seeds.size();) {
        size_t s1 = s0;
        while (s1 < seeds.size() && seeds[s1].key == seeds[s0].key) s1++;
        a.resize(s1 - s0);
        for (size_t q = s0; q < s1; q++) a[q - s0] = rawdtw_anchor_t{seeds[q].target_position, seeds[q].query_position};
        outa.resize(std::max<size_t>(a.size(), 1));
        const int nc = rawdtw_chain_anchors(&m->opt.chain, a.data(), (uint32_t)a.size(), &maxs, outc.data(), off.data(), outa.data(), cap, outa.size());
        if (nc < 0) { rr.err = RAWDTW_ERR_RANGE; return; }
        for (int c = 0; c < nc; c++) {
            MChain ch;
            ch.chaining_score = outc[c].chaining_score; ch.ref = seeds[s0].key >> 1; ch.strand = (int32_t)(seeds[s0].key & 1u);
            ch.start_position = outc[c].start_position; ch.end_position = outc[c].end_position;
            ch.anchors.assign(outa.begin() + off[c], outa.begin() + off[c + 1]);
            chains.push_back(std::move(ch));
        }
        s0 = s1;
    }
    if (!chains.empty() && runs_dtw) { // rmap.cpp:512: std::sort by chaining score, descending (its permutation)
        std::vector<float> cs(chains.size());
        for (size_t c = 0; c < chains.size(); c++) cs[c] = chains[c].chaining_score;
        std::vector<uint32_t> perm(chains.size());
        if (rawdtw_sort_by_chaining_score(cs.data(), (uint32_t)cs.size(), perm.data()) != RAWDTW_OK) { rr.err = RAWDTW_ERR_INVALID; return; }
        std::vector<MChain> sorted;
        sorted.reserve(chains.size());
        for (uint32_t p : perm) sorted.push_back(std::move(chains[p]));
        chains.swap(sorted);
    }
    rr.chains = std::move(chains);
    if (!runs_dtw) return;
    rr.ref_base.resize(rr.chains.size());
    rr.carry.assign(rr.chains.size(), rawdtw_carry_t{RAWDTW_NO_CHAIN, 0u, 0u, rawdtw_anchor_t{0u, 0u}});
    for (size_t c = 0; c < rr.chains.size(); c++) rr.ref_base[c] = m->ref_off[rr.chains[c].ref * 2u + (uint32_t)rr.chains[c].strand];
}

void host_phase_carry(const MRead &rd, RoundRead &rr, const RoundArrays *pv)
{
    // chunk rounds: the chain of the round before this chain continues -- same strand array, same start anchor, the longest
    // common tail, compared anchor by anchor -- and the leading parts taken over (as rawdtw_round_match_chains)
    const uint64_t pr = rd.last_pos;
    for (size_t c = 0; c < rr.chains.size(); c++) {
        const std::vector<rawdtw_anchor_t> &an = rr.chains[c].anchors;
        const uint64_t na = an.size();
        if (na) rr.carry[c].start = an[na - 1];
        if (na < 2) continue;
        uint64_t best = 0, best_b0 = 0, best_b1 = 0;
        for (uint64_t pc = pv->chain_off[pr]; pc < pv->chain_off[pr + 1]; pc++) {
            const uint64_t b0 = pv->anchor_off[pc], b1 = pv->anchor_off[pc + 1];
            if (b1 < b0 + 2 || pv->ref_base[pc] != rr.ref_base[c]) continue;
            const rawdtw_anchor_t *pa = pv->anchors.p;
            uint64_t same = 0;
            while (same < na && same < b1 - b0 && an[na - 1 - same].target_position == pa[b1 - 1 - same].target_position &&
                   an[na - 1 - same].query_position == pa[b1 - 1 - same].query_position)
                same++;
            if (same == na && same < b1 - b0) same--; // (its last part was not the last then: rmap.cpp:270, no exact way back)
            if (same >= 2 && same > best) { best = same; best_b0 = b0; best_b1 = b1; }
        }
        if (best >= 2) {
            rr.carry[c].parts = (uint32_t)(best - 1);
            rr.carry[c].prev_src = best_b1 - best;                                    // the stretch's first entry in the previous full list
            rr.carry[c].flags = (best == best_b1 - best_b0 && na > best) ? 1u : 0u;    // its first part was the last one then and is not now
        }
    }
}

// sequence-until: a mini-batch the caller closes -- every read known, held, finished, in no closed batch, once
int su_check_batch(rawdtw_mapper *m, uint32_t n, const uint32_t *read_ids)
{
    if (n && !read_ids) return fail(m, RAWDTW_ERR_INVALID, "null read ids");
    if (!m->su) return fail(m, RAWDTW_ERR_INVALID, "sequence-until is off (flag 0x1 or rawdtw_mapper_set_sequence_until)");
    int st = RAWDTW_OK;
    const char *msg = "";
    const uint64_t stamp = ~(uint64_t)0; // (duplicate check through seen_round, which a round clears again)
    uint32_t k = 0;
    for (; k < n && st == RAWDTW_OK; k++) {
        if (read_ids[k] >= m->reads.size()) { st = RAWDTW_ERR_INVALID; msg = "unknown read id"; break; }
        MRead &rd = m->reads[read_ids[k]];
        if (rd.seen_round == stamp) { st = RAWDTW_ERR_INVALID; msg = "a read twice in one batch"; break; }
        if (rd.released) { st = RAWDTW_ERR_INVALID; msg = "a released read in a batch"; }
        else if (!rd.finished) { st = RAWDTW_ERR_INVALID; msg = "an unfinished read in a batch"; }
        else if (rd.closed) { st = RAWDTW_ERR_INVALID; msg = "a read of a batch closed before"; }
        rd.seen_round = stamp;
    }
    for (uint32_t q = 0; q < k && q < n; q++) m->reads[read_ids[q]].seen_round = 0;
    return st == RAWDTW_OK ? RAWDTW_OK : fail(m, st, msg);
}

// a read's record as rmap.cpp:750-756 / 790-799 leave it in reg0: (mapped, ref_id, fragment_length); (0, 0, 0) for a read without a line
void su_record(const rawdtw_mapper *m, const MRead &rd, uint8_t *mapped, uint32_t *ref_id, uint32_t *fragment_length)
{
    const bool mp = !rd.dropped && high_confidence(m, rd.chains);
    *mapped = mp ? 1 : 0;
    *ref_id = mp ? rd.chains[0].ref : 0u;
    *fragment_length = mp ? rd.chains[0].end_position - rd.chains[0].start_position + 1u : 0u;
}

// a chaining round begun on the device and not to be used: ended, its results dropped
void discard_chain_round(rawdtw_ctx *ctx)
{
    const rawdtw_anchor_t *a = nullptr; const uint64_t *rb = nullptr; const uint32_t *qb = nullptr;
    (void)rawdtw_chain_round_end(ctx, &a, &rb, &qb);
}

// a context's option as the mapper reads it, through the public ABI: 0 for no context or a refusal
int64_t ctx_option(const rawdtw_ctx *ctx, const char *name)
{
    int64_t v = 0;
    return ctx && rawdtw_get_option(ctx, name, &v) == RAWDTW_OK ? v : 0;
}

// a read's slot in its group's event arena: the group's context and the slot's first float
rawdtw_ctx *slot_of(const rawdtw_mapper *m, const MRead &rd, uint32_t *base)
{
    const uint32_t G = (uint32_t)m->groups.size();
    *base = (G == 2 ? rd.slot / 2 : rd.slot) * m->opt.slot_events;
    return m->groups[rd.slot % G].ctx;
}

// a round's sizes in one group (0 where its path does not know them)
struct Sizes { uint64_t reads = 0, chains = 0, anchors = 0, new_anchors = 0, events = 0, seg = 0, seeds = 0; };

// One rawdtw_mapper_round after its checks.  The phases write only into the round's own state (rr, the groups' buffers of the round
// at hand, per); commit() is the one place the result reaches the reads and the mapper, and rollback() drops it.  The exception is
// the host's copy of a read's events, which the external scorer reads during the round: appended early, cut back by the rollback.
struct Round {
    rawdtw_mapper *m;
    uint32_t n_reads;
    const uint32_t *read_ids; const uint64_t *event_off; const float *events; const uint64_t *hit_off; const rawdtw_seed_hit_t *hits;
    double t0; // (the last lap)
    // a resident round: the hits are on the device (hit_off / hits are set only by its fall-back, which fetches them)
    bool resident = false, fell_back = false;
    bool signal = false; // a round from signal: the events are in the arena already (the device detected them there), event_off holds their counts
    uint64_t res_prev = 0, res_hits = 0; // previous anchors sent up as seeds; hits fetched by the fall-back
    uint32_t G = (uint32_t)m->groups.size(); // (1 or 2)
    uint64_t id = m->rounds + 1;
    bool runs_dtw = (m->opt.flag & (0x2 | 0x8)) != 0, on_device = runs_dtw && !m->scorer;
    // the caller's event array goes to the device as it is when it is page-locked (rawdtw_host_alloc) and one read group takes the whole round:
    // its reads' chunks ARE the segments, in order -- no copy into the mapper's own staging (a third of the host phase)
    bool events_in_place = on_device && m->opt.device_chain && G == 1 && event_off[n_reads] > 0 && rawdtw_host_is_page_locked(events) == 1;
    std::vector<RoundRead> rr = std::vector<RoundRead>(n_reads);
    struct GroupOpt { bool decline_reads = false; uint32_t max_chains = 0; }; // the group's context's "chain_decline_reads" and "chain_max_chains"
    static GroupOpt group_opt(const rawdtw_mapper *m, size_t gi)
    {
        const rawdtw_ctx *ctx = gi < m->groups.size() ? m->groups[gi].ctx : nullptr;
        return GroupOpt{ctx_option(ctx, "chain_decline_reads") != 0, (uint32_t)ctx_option(ctx, "chain_max_chains")};
    }
    struct PerGroup { GroupOpt opt; // (read once, when the round is built: a phase that starts the group's record over keeps it)
                      bool chaining = false; uint64_t ns = 0, nev = 0, nseg = 0, scored = 0, reused = 0, extra = 0; // (ns: seeds sent up; extra: other bytes)
                      bool round_end = false; uint64_t re_reads = 0, re_declined = 0; // (the round's end enqueued on the device; the reads it ended / declined)
                      bool keep = false;                                              // (... and the keep launch behind it)
                      uint64_t dc_reads = 0, dc_seeds = 0, dc_chains = 0, dc_device = 0, dc_bytes = 0; // ("chain_decline_reads": the reads declined alone, by reason; the others; seed bytes home)
    } per[2] = {{group_opt(m, 0)}, {group_opt(m, 1)}};
    const GroupOpt &opt_of(const Group &g) const { return per[&g - m->groups.begin()].opt; }
    bool device_round_end = ctx_option(m->ctx, "device_round_end") != 0;         // (the mapper's own context's, read once a round)
    uint32_t resident_chains = (uint32_t)ctx_option(m->ctx, "resident_chains"); // (so is this)
    // the round takes previous seeds from the store of kept chains and keeps its own there: a resident round with the option on whose end
    // is enqueued on the device
    bool use_store() const { return resident && resident_chains != 0 && device_round_end && runs_dtw; }
    int status = RAWDTW_OK;
    std::string msg;

    MRead &read(uint32_t k) const { return m->reads[read_ids[k]]; }
    uint32_t arena_base(const MRead &rd) const { return (G == 2 ? rd.slot / 2 : rd.slot) * m->opt.slot_events; } // its slot in its group's event arena
    bool ok() const { return status == RAWDTW_OK; }
    void failed(int st, const std::string &s) { if (ok()) { status = st; msg = s; } }
    void lap(int slot) { const double t = now_ms(); m->timing[slot] += t - t0; t0 = t; } // (include/rawdtw.h: rawdtw_mapper_timing)

    void deal() // the round's reads over the groups, into each group's other buffer
    {
        for (Group &g : m->groups) { g.cur ^= 1; g.buf[g.cur].ks.clear(); }
        for (uint32_t k = 0; k < n_reads; k++) { Group &g = m->groups[read(k).slot % G]; g.buf[g.cur].ks.push_back(k); }
    }

    // The host phase of one read: the chunk's events (rmap.cpp:554-575); false: the chunk is below min_events -- no gen_chains this round.
    // Then host_phase_chain, or with device chaining its seed list.
    bool append_events(uint32_t k)
    {
        MRead &rd = read(k);
        RoundRead &r = rr[k];
        r.ne = event_off[k + 1] - event_off[k];
        r.ev_before = rd.n_events; r.off_before = rd.offset;
        if (m->keep_host_events && !signal) rd.events.insert(rd.events.end(), events + event_off[k], events + event_off[k + 1]); // rmap.cpp:554-567
        rd.n_events += (uint32_t)r.ne;
        if (r.ne < m->opt.min_events) { r.skipped = true; return false; } // rmap.cpp:569-572: no gen_chains, reg->offset stays
        r.chunk_start = rd.offset;  // reg->offset (rmap.cpp:574)
        rd.offset += (uint32_t)r.ne; // rmap.cpp:575
        return true;
    }

    // Both of a group's buffers grown to its high-water marks, as its path needs them: chaining on the device (seed lists in, chains out)
    // or on the host (anchor lists, the events' staging, carry records), page-locked unless an external scorer takes the round.  The
    // round before's first n_reads + 1 / n_chains + 1 / n_anchors + 1 entries survive a growth (the host chaining's matching reads them).
    bool size_arrays(Group &g, const Sizes &n, bool dev)
    {
        const bool pin = on_device, carry = on_device && !dev && m->opt.carry;
        g.hw_reads = std::max(g.hw_reads, n.reads); g.hw_chains = std::max(g.hw_chains, n.chains); g.hw_anchors = std::max(g.hw_anchors, n.anchors);
        g.hw_new = std::max(g.hw_new, n.new_anchors); g.hw_events = std::max(g.hw_events, n.events); g.hw_seg = std::max(g.hw_seg, n.seg);
        g.hw_seeds = std::max(g.hw_seeds, n.seeds);
        if (dev) { // the device's cap on chains a read: 32, or "chain_max_chains" -- then no more than the seeds can make, min_num_anchors a chain
            const uint32_t many = opt_of(g).max_chains;
            const uint64_t by_seeds = g.hw_seeds / (uint64_t)std::max(1, m->opt.chain.min_num_anchors) + 1;
            g.hw_chains = std::max<uint64_t>(g.hw_chains, many > 0 ? std::min<uint64_t>(g.hw_reads * (uint64_t)many, by_seeds) : g.hw_reads * 32);
        }
        const uint64_t nr = g.hw_reads + 1, nc = g.hw_chains + 1;
        for (int b = 0; b < 2; b++) {
            RoundArrays &x = g.buf[g.cur ^ b];
            const bool kept = b == 1 && !dev;
            const size_t k_r = kept ? x.n_reads + 1 : 0, k_c = kept ? x.n_chains + 1 : 0, k_a = kept ? x.n_anchors + 1 : 0;
            bool ok = x.chain_off.ensure(nr, pin, k_r) && x.anchor_off.ensure(nc, pin, k_c) && x.read_base.ensure(nc, pin, k_c) &&
                      x.anchors.ensure((dev ? g.hw_seeds : g.hw_anchors) + 1, pin && !(m->opt.carry && g.has_prev), k_a) && x.score.ensure(nc, pin) &&
                      x.keep.ensure(nc, pin);
            if (dev) ok = ok && x.seed_off.ensure(nr, pin) && x.seeds.ensure(g.hw_seeds + 1, pin) && x.recs.ensure(nc, pin);
            else ok = ok && x.ref_base.ensure(nc, pin, k_c);
            if (carry) ok = ok && x.new_off.ensure(nc, pin) && x.new_anchors.ensure(g.hw_new + 1, pin) && x.carry.ensure(nc, pin);
            if (pin)
                ok = ok && x.new_events.ensure((events_in_place ? 0 : g.hw_events) + 1, pin) && x.seg_src.ensure(g.hw_seg + 2, pin) &&
                     x.seg_dst.ensure((dev ? g.hw_reads : g.hw_seg) + 1, pin);
            if (!ok) { failed(RAWDTW_ERR_OOM, "host allocation failed"); return false; }
        }
        return true;
    }

    // ---- a group's first half: the host phase, lay-out and submission; with device chaining the chaining begun instead ----
    void begin_group(uint32_t gi)
    {
        Group &g = m->groups[gi]; RoundArrays &ra = g.buf[g.cur];
        const RoundArrays &pb = g.buf[g.cur ^ 1];
        ra.carried = false; ra.round_id = id; ra.n_reads = ra.ks.size();
        if (on_device && m->opt.device_chain) {
            if (!device_begin(gi) && ok()) host_round(gi, nullptr, true);
            return;
        }
        const RoundArrays *pv = nullptr;
        if (on_device && m->opt.carry && g.has_prev && pb.batch && rawdtw_batch_can_carry(g.ctx, pb.batch, &m->opt.align)) {
            size_t known = 0; // (a round none of whose reads was in the round before has nothing to take over: submitted whole)
            for (size_t i = 0; i < ra.ks.size() && !known; i++) known += read(ra.ks[i]).last_round == pb.round_id;
            if (known) { pv = &pb; ra.carried = true; }
        }
        host_round(gi, pv, false);
    }

    // ---- device chaining, first half: the host phase is the events and the seed lists; sort, chaining DP, traceback and order are
    // enqueued (rawdtw_chain_round_begin) and run while the next group's host phase does.  false: the device declined (its cap on seeds a
    // read) -- the events are in place on both sides, the round is chained on the host.
    bool device_begin(uint32_t gi)
    {
        Group &g = m->groups[gi]; RoundArrays &ra = g.buf[g.cur];
        const size_t nr = ra.ks.size();
        if (nr == 0) return true; // (none of the round's reads is this group's)
        m->pool->run(nr, 64, [&](size_t i) {
            const uint32_t k = ra.ks[i];
            if (append_events(k)) rr[k].n_seeds = seed_count(read(k), hit_off[k + 1] - hit_off[k]);
        });
        Sizes n{nr};
        for (uint32_t k : ra.ks) { rr[k].seed0 = n.seeds; n.seeds += rr[k].n_seeds; }
        if (!stage_events(g, n, true, events_in_place)) return true;
        ra.seed_off[nr] = n.seeds;
        m->pool->run(nr, 64, [&](size_t i) {
            const uint32_t k = ra.ks[i];
            const RoundRead &r = rr[k];
            ra.seed_off[i] = r.seed0;
            ra.read_base[i] = arena_base(read(k));
            if (!r.skipped) write_seeds(read(k), hits + hit_off[k], hit_off[k + 1] - hit_off[k], r.chunk_start, ra.seeds.p + r.seed0);
            if (!events_in_place) stage_chunk(ra, k);
        });
        lap(0);
        // the chaining first, the events behind it: the sort + DP does not read them, and rawdtw_chain_round_end waits for the round's own work only
        // -- the events' upload (the round's largest) runs on while the host goes on
        int st = rawdtw_chain_round_begin(g.ctx, &m->opt.chain, nr, ra.seed_off.p, ra.seeds.p, ra.read_base.p, (uint32_t)m->ref_off.size(), m->ref_off.data(),
                                          ra.chain_off.p, ra.anchor_off.p, ra.recs.p, g.hw_chains, ra.anchors.p);
        const bool declined = st == RAWDTW_ERR_UNSUPPORTED;
        if (st == RAWDTW_OK || declined) {
            const int se = upload_events(g, n, events_in_place);
            if (se != RAWDTW_OK && st == RAWDTW_OK) discard_chain_round(g.ctx);
            if (se != RAWDTW_OK) st = se;
        }
        lap(2);
        if (declined && st == RAWDTW_ERR_UNSUPPORTED) return false;
        if (st != RAWDTW_OK) { failed(st, rawdtw_last_error(g.ctx)); return true; }
        per[gi] = PerGroup{per[gi].opt, true, n.seeds, n.events, n.seg};
        return true;
    }

    // ---- a resident round's first half (one group): the events go up first, the seeding reads them in the arena and sends the hit counts
    // home -- the one wait --, the arrays are sized by them, and the chaining is begun on seeds the device lays down itself: only the previous
    // chains' anchors go up.  A round the chaining declines fetches the hits and is chained on the host, as device_begin's is.
    void resident_begin(uint32_t gi)
    {
        Group &g = m->groups[gi]; RoundArrays &ra = g.buf[g.cur];
        ra.carried = false; ra.round_id = id; ra.n_reads = ra.ks.size();
        const size_t nr = ra.ks.size();
        m->pool->run(nr, 64, [&](size_t i) { append_events(ra.ks[i]); });
        Sizes n{nr};
        if (!stage_events(g, n, true, events_in_place)) return;
        const uint64_t nev = n.events, nseg = n.seg;
        if (!resident_arrays(g)) return;
        m->pool->run(nr, 64, [&](size_t i) {
            const uint32_t k = ra.ks[i];
            const RoundRead &r = rr[k];
            ra.ev_start[i] = (uint64_t)arena_base(read(k)) + r.ev_before;
            ra.ev_len[i] = (uint32_t)r.ne;
            if (!events_in_place) stage_chunk(ra, k);
        });
        lap(0);
        int st = upload_events(g, n, events_in_place);
        if (st == RAWDTW_OK) st = rawdtw_seed_resident_begin(g.ctx, (uint32_t)nr, ra.ev_start.p, ra.ev_len.p, m->seed_off.p);
        if (st == RAWDTW_OK) st = rawdtw_seed_resident_end(g.ctx, nullptr);
        lap(2);
        if (st != RAWDTW_OK) return failed(st, rawdtw_last_error(g.ctx));
        resident_chain(gi, nev, nseg);
    }

    // a resident round's own per-read arrays, in both buffers (sized by the group's high-water mark of reads)
    bool resident_arrays(Group &g)
    {
        for (int b = 0; b < 2; b++) {
            RoundArrays &x = g.buf[g.cur ^ b];
            if (!(x.prev_off.ensure(g.hw_reads + 1, true) && x.ev_start.ensure(g.hw_reads + 1, true) && x.ev_len.ensure(g.hw_reads + 1, true) &&
                  x.chunk_start.ensure(g.hw_reads + 1, true) && x.sits_out.ensure(g.hw_reads + 1, true))) {
                failed(RAWDTW_ERR_OOM, "host allocation failed");
                return false;
            }
        }
        return true;
    }

    // ---- a round from signal, first half: detection and seeding ran on the device before the round was set up (rawdtw_mapper_round_signal_*),
    // the events are in the arena and their counts in event_off; what is left of the host phase is the bookkeeping of append_events ----
    void signal_begin(uint32_t gi)
    {
        Group &g = m->groups[gi]; RoundArrays &ra = g.buf[g.cur];
        ra.carried = false; ra.round_id = id; ra.n_reads = ra.ks.size();
        const size_t nr = ra.ks.size();
        m->pool->run(nr, 64, [&](size_t i) { append_events(ra.ks[i]); });
        if (!size_arrays(g, Sizes{nr}, true) || !resident_arrays(g)) return;
        lap(0);
        resident_chain(gi, 0, 0); // (no event went up from the host: nothing for slot 6)
    }

    // ---- a resident round from the ended seeding on: the arrays sized by the hit counts, the chaining begun on seeds the device lays down
    // itself, or the fall-back.  nev / nseg: the events and segments the host sent up this round (the byte counters') ----
    void resident_chain(uint32_t gi, uint64_t nev, uint64_t nseg)
    {
        Group &g = m->groups[gi]; RoundArrays &ra = g.buf[g.cur];
        const size_t nr = ra.ks.size();
        int st = RAWDTW_OK;
        const uint64_t *hoff = m->seed_off.p; // (chunk i is read ks[i]: one group, the round's reads in order)
        uint64_t ns = 0, np = 0;
        const bool store = use_store();
        if (store && !reserve_store(g)) return;
        for (size_t i = 0; i < nr; i++) {
            RoundRead &r = rr[ra.ks[i]];
            const MRead &rd = read(ra.ks[i]);
            const uint64_t pv = r.skipped ? 0 : seed_count(rd, 0);
            r.from_store = store && !r.skipped && rd.kept.valid;
            r.n_prev = pv;
            if (r.from_store && rd.kept.count != pv) // (the half holds another list than write_seeds would build: never go on with it)
                return failed(RAWDTW_ERR_DEVICE, "a read's kept chains on the device (" + std::to_string(rd.kept.count) + " seeds) are not its chains on the host (" +
                                                     std::to_string(pv) + " anchors)");
            r.seed0 = np; np += r.from_store ? 0 : pv; // (a read seeded from the store sends nothing up)
            r.n_seeds = r.skipped ? 0 : pv + (hoff[i + 1] - hoff[i]);
            ns += r.n_seeds;
        }
        if (!size_arrays(g, Sizes{nr, 0, 0, 0, nev, nseg, ns}, true)) return; // (the seed list's size: room for the round's anchors coming back)
        uint64_t at = 0;
        for (size_t i = 0; i < nr; i++) { const RoundRead &r = rr[ra.ks[i]]; ra.seed_off[i] = at; ra.prev_off[i] = r.seed0; at += r.n_seeds; }
        ra.seed_off[nr] = ns; ra.prev_off[nr] = np;
        m->pool->run(nr, 64, [&](size_t i) {
            const uint32_t k = ra.ks[i];
            const RoundRead &r = rr[k];
            ra.read_base[i] = arena_base(read(k));
            ra.chunk_start[i] = r.chunk_start;
            ra.sits_out[i] = r.skipped ? 1 : 0;
            if (!r.skipped && !r.from_store) write_seeds(read(k), nullptr, 0, 0, ra.seeds.p + r.seed0); // (the previous chains' anchors only)
            if (store) { // its previous seeds from the half it holds; its chains into the other one (half 0 for a read that holds none)
                const MRead &rd = read(k);
                ra.prev_src[i] = r.from_store ? rd.slot * 2u + rd.kept.half : RAWDTW_PREV_HOST;
                ra.keep_dst[i] = r.skipped ? RAWDTW_NO_KEEP : rd.slot * 2u + (rd.kept.valid ? (rd.kept.half ^ 1u) : 0u);
            }
        });
        lap(0);
        if (store)
            st = rawdtw_chain_round_begin_resident_kept(g.ctx, &m->opt.chain, nr, ra.seed_off.p, ra.prev_off.p, ra.seeds.p, ra.prev_src.p, ra.chunk_start.p, ra.sits_out.p,
                                                        ra.read_base.p, (uint32_t)m->ref_off.size(), m->ref_off.data(), ra.chain_off.p, ra.anchor_off.p, ra.recs.p,
                                                        g.hw_chains, ra.anchors.p);
        else
            st = rawdtw_chain_round_begin_resident(g.ctx, &m->opt.chain, nr, ra.seed_off.p, ra.prev_off.p, ra.seeds.p, ra.chunk_start.p, ra.sits_out.p, ra.read_base.p,
                                                   (uint32_t)m->ref_off.size(), m->ref_off.data(), ra.chain_off.p, ra.anchor_off.p, ra.recs.p, g.hw_chains, ra.anchors.p);
        lap(2);
        if (st == RAWDTW_ERR_UNSUPPORTED) { // a read above the device's cap on seeds: nothing was enqueued
            m->timing[6] += (double)(nev * sizeof(float));
            if (fetch_resident_hits(gi)) host_round(gi, nullptr, true);
            return;
        }
        if (st != RAWDTW_OK) return failed(st, rawdtw_last_error(g.ctx));
        res_prev = np;
        // (beside the chaining's own arrays: prev_off, chunk_start, sits_out; the seeding's offsets and source starts)
        per[gi] = PerGroup{per[gi].opt, true, np, nev, nseg, 0, 0, (nr + 1) * 8 + nr * 5 + (nr + 1) * 8 + nr * 8};
    }

    // "resident_chains": the context's store reserved for every slot of the mapper at the first round that uses it, and this round's
    // per-read arrays.  A store that had to grow (the option was raised) has lost its contents: no read holds kept chains any more.
    bool reserve_store(Group &g)
    {
        if (m->kp_reserved < resident_chains) {
            const int st = rawdtw_chain_keep_reserve(g.ctx, m->opt.max_reads, resident_chains);
            if (st != RAWDTW_OK) { failed(st, rawdtw_last_error(g.ctx)); return false; }
            if (m->kp_reserved) for (MRead &rd : m->reads) rd.kept.valid = false;
            m->kp_reserved = resident_chains;
        }
        for (int b = 0; b < 2; b++) {
            RoundArrays &x = g.buf[g.cur ^ b];
            if (!(x.prev_src.ensure(g.hw_reads + 1, true) && x.keep_dst.ensure(g.hw_reads + 1, false) && x.kept_count.ensure(g.hw_reads + 1, false))) {
                failed(RAWDTW_ERR_OOM, "host allocation failed");
                return false;
            }
        }
        return true;
    }

    // the fall-back of a resident round: its hits to the host, once, where host_round reads them
    bool fetch_resident_hits(uint32_t gi)
    {
        const uint64_t tot = m->seed_off[n_reads];
        if (!seed_room(m, m->seed_hits, tot + 1)) { failed(RAWDTW_ERR_OOM, "no page-locked memory for the round's hits"); return false; }
        const int st = rawdtw_seed_resident_fetch(m->groups[gi].ctx, m->seed_hits.p, m->seed_hits.cap);
        if (st != RAWDTW_OK) { failed(st, rawdtw_last_error(m->groups[gi].ctx)); return false; }
        hit_off = m->seed_off.p; hits = m->seed_hits.p;
        fell_back = true; res_hits = tot;
        lap(2);
        return true;
    }

    // second half: the wait, the DTW submission straight from the device's arrays, and -- while that batch runs -- the round's chains per read, as
    // the host phase would have left them; a round the device declined (a read with too many chains, or an order only std::sort knows) is
    // chained on the host.  After a failure elsewhere the chaining begun is discarded.
    void end_device_chain(uint32_t gi)
    {
        Group &g = m->groups[gi]; RoundArrays &ra = g.buf[g.cur];
        PerGroup &p = per[gi];
        if (!p.chaining) return;
        p.chaining = false;
        if (!ok()) return discard_chain_round(g.ctx);
        const size_t nr = ra.ks.size();
        const rawdtw_anchor_t *d_anchors = nullptr; const uint64_t *d_ref_base = nullptr; const uint32_t *d_read_base = nullptr;
        int st = rawdtw_chain_round_end(g.ctx, &d_anchors, &d_ref_base, &d_read_base);
        if (st == RAWDTW_ERR_UNSUPPORTED) {
            lap(2);
            if (resident) { m->timing[6] += (double)(p.nev * sizeof(float)); if (!fetch_resident_hits(gi)) return; }
            return host_round(gi, nullptr, true);
        }
        if (st != RAWDTW_OK) return failed(st, rawdtw_last_error(g.ctx));
        // "chain_decline_reads": the reads the device declined alone are chained here, their chains appended behind the device's
        uint64_t nd = 0;
        const uint64_t *batch_off = ra.chain_off.p, *batch_aoff = ra.anchor_off.p;
        if (opt_of(g).decline_reads) {
            if (!append_declined(gi, &nd, &d_anchors, &d_ref_base, &d_read_base)) return;
            if (nd) { batch_off = ra.chain_off_ext.p; batch_aoff = ra.anchor_off_ext.p; }
        }
        const uint64_t nc = batch_off[nr + nd], na = batch_aoff[nc];
        ra.n_chains = nc; ra.n_anchors = na; ra.n_reads_batch = nr + nd;
        // (a resident round of a mapper that runs no DTW -- neither EVALUATE_CHAINS nor LOG_SCORES -- ends with the chains: rmap.cpp:509)
        if (runs_dtw) st = rawdtw_batch_submit_device(g.ctx, &m->opt.align, nr + nd, batch_off, batch_aoff, d_anchors, d_ref_base, d_read_base, &ra.batch);
        if (st != RAWDTW_OK) return failed(st, rawdtw_last_error(g.ctx));
        if (runs_dtw && device_round_end && ra.batch) st = begin_round_end(g, ra, p);
        if (st != RAWDTW_OK) return failed(st, rawdtw_last_error(g.ctx));
        m->timing[6] += (double)(p.nev * sizeof(float));
        m->timing[7] += (double)(p.ns * sizeof(rawdtw_seed_t) + (nr + 1) * 16 + nr * 4 + (nc + 1) * 8 + p.nseg * 12 + p.extra);
        lap(2);
        m->pool->run(nr, 32, [&](size_t i) {
            RoundRead &r = rr[ra.ks[i]];
            if (r.declined) return; // (its chains are the host's already, and chain0 / bpos its pseudo-read's)
            r.bpos = i;
            r.chain0 = ra.chain_off[i];
            r.chains.resize(ra.chain_off[i + 1] - ra.chain_off[i]);
            for (uint64_t c = 0; c < r.chains.size(); c++) {
                const rawdtw_chain_rec_t &rec = ra.recs[r.chain0 + c];
                MChain &ch = r.chains[c];
                ch.chaining_score = rec.chaining_score; ch.ref = rec.key >> 1; ch.strand = (int32_t)(rec.key & 1u);
                ch.start_position = rec.start_position; ch.end_position = rec.end_position;
                const rawdtw_anchor_t *an = ra.anchors.p + ra.anchor_off[r.chain0 + c];
                ch.anchors.assign(an, an + rec.n_anchors);
            }
        });
        lap(1);
    }

    // "chain_decline_reads", after a successful rawdtw_chain_round_end: the declined reads' seeds (from the device in a resident round, whose
    // seed list was laid down there; from the group's own list otherwise), their chains by the host's code on the pool, and the append.  Each
    // declined read gets a pseudo-read at the end of the batch's read list (bpos): the batch's score and keep, k_round_end's record and primaries
    // are read there, and its own empty stretch is never looked at.  It is not kept in the store (RAWDTW_NO_KEEP on both).  false: failed.
    bool append_declined(uint32_t gi, uint64_t *n_declined, const rawdtw_anchor_t **d_anchors, const uint64_t **d_ref_base, const uint32_t **d_read_base)
    {
        Group &g = m->groups[gi]; RoundArrays &ra = g.buf[g.cur];
        PerGroup &p = per[gi];
        const size_t nr = ra.ks.size();
        uint64_t nd = 0;
        const uint32_t *dreads = nullptr, *dwhy = nullptr;
        int st = rawdtw_chain_round_declined(g.ctx, &nd, &dreads, &dwhy);
        if (st != RAWDTW_OK) { failed(st, rawdtw_last_error(g.ctx)); return false; }
        *n_declined = nd;
        for (size_t i = 0; i < nr; i++) p.dc_device += rr[ra.ks[i]].skipped ? 0 : 1;
        if (nd == 0) return true;
        const uint64_t *soff = ra.seed_off.p; // (a declined read's seeds: [soff[x], soff[x + 1]) of `seeds`, x its position in the group or in the list)
        const rawdtw_seed_t *seeds = ra.seeds.p;
        if (resident) {
            if (!seed_room(m, m->decl_soff, nd + 1)) { failed(RAWDTW_ERR_OOM, "no page-locked memory for the declined reads' seeds"); return false; }
            st = rawdtw_chain_round_declined_seeds(g.ctx, m->decl_soff.p, m->decl_seeds.p, m->decl_seeds.p ? m->decl_seeds.cap : 0);
            if (st == RAWDTW_ERR_RANGE) { // (the offsets are filled: room for what they say, then again)
                if (!seed_room(m, m->decl_seeds, m->decl_soff[nd] + 1)) { failed(RAWDTW_ERR_OOM, "no page-locked memory for the declined reads' seeds"); return false; }
                st = rawdtw_chain_round_declined_seeds(g.ctx, m->decl_soff.p, m->decl_seeds.p, m->decl_seeds.cap);
            }
            if (st != RAWDTW_OK) { failed(st, rawdtw_last_error(g.ctx)); return false; }
            soff = m->decl_soff.p; seeds = m->decl_seeds.p;
            p.dc_bytes += m->decl_soff[nd] * sizeof(rawdtw_seed_t);
        }
        m->pool->run(nd, 1, [&](size_t j) {
            const size_t x = resident ? j : dreads[j];
            RoundRead &r = rr[ra.ks[dreads[j]]];
            std::vector<rawdtw_seed_t> mine(seeds + soff[x], seeds + soff[x + 1]);
            host_chain_seeds(m, r, mine, runs_dtw);
            r.declined = true; r.bpos = nr + j;
        });
        std::vector<uint64_t> coff(nd + 1, 0), aoff(1, 0);
        for (uint64_t j = 0; j < nd; j++) {
            const RoundRead &r = rr[ra.ks[dreads[j]]];
            if (r.err != RAWDTW_OK) { failed(r.err, "chaining failed (chain output buffers too small)"); return false; }
            coff[j + 1] = coff[j] + r.chains.size();
            p.dc_reads++; p.dc_seeds += dwhy[j] & 1u; p.dc_chains += (dwhy[j] & 6u) ? 1 : 0;
        }
        p.dc_device -= nd;
        std::vector<rawdtw_chain_rec_t> recs(coff[nd] + 1);
        std::vector<rawdtw_anchor_t> anchors;
        for (uint64_t j = 0; j < nd; j++) {
            const RoundRead &r = rr[ra.ks[dreads[j]]];
            for (size_t c = 0; c < r.chains.size(); c++) {
                const MChain &ch = r.chains[c];
                recs[coff[j] + c] = rawdtw_chain_rec_t{ch.chaining_score, ch.ref * 2u + (uint32_t)ch.strand, ch.start_position, ch.end_position, (uint32_t)ch.anchors.size()};
                anchors.insert(anchors.end(), ch.anchors.begin(), ch.anchors.end());
                aoff.push_back(anchors.size());
            }
        }
        anchors.push_back(rawdtw_anchor_t{0, 0}); // (never a null array)
        // room, on demand -- a round nobody is declined in allocates nothing: the batch's two offset arrays, its per-chain results, and with the
        // store its per-read destinations (whose first nr entries are written already)
        const uint64_t nc = ra.chain_off[nr] + coff[nd], nb = nr + nd;
        bool room = ra.chain_off_ext.ensure(nb + 1, on_device) && ra.anchor_off_ext.ensure(nc + 1, on_device) && ra.score.ensure(nc + 1, on_device) &&
                    ra.keep.ensure(nc + 1, on_device);
        if (use_store()) room = room && ra.keep_dst.ensure(nb + 1, false, nr) && ra.kept_count.ensure(nb + 1, false);
        if (!room) { failed(RAWDTW_ERR_OOM, "host allocation failed"); return false; }
        st = rawdtw_chain_round_append(g.ctx, nd, coff.data(), recs.data(), aoff.data(), anchors.data(), ra.chain_off_ext.p, ra.anchor_off_ext.p, d_anchors, d_ref_base,
                                       d_read_base);
        if (st != RAWDTW_OK) { failed(st, rawdtw_last_error(g.ctx)); return false; }
        for (uint64_t j = 0; j < nd; j++) {
            rr[ra.ks[dreads[j]]].chain0 = ra.chain_off_ext[nr + j];
            if (use_store()) { ra.keep_dst[dreads[j]] = RAWDTW_NO_KEEP; ra.keep_dst[nr + j] = RAWDTW_NO_KEEP; }
        }
        p.extra += (nd + 1) * 8 + coff[nd] * (sizeof(rawdtw_chain_rec_t) + 20) + (anchors.size() - 1) * sizeof(rawdtw_anchor_t);
        return true;
    }

    // "device_round_end": the round's end enqueued right behind the batch, on the chaining workspace's records where they lie
    int begin_round_end(Group &g, RoundArrays &ra, PerGroup &p)
    {
        // (a round that declined reads alone has a pseudo-read for each of them, and their chains behind the device's: ra.n_reads_batch / n_chains)
        if (!ra.re_out.ensure(std::max<uint64_t>(g.hw_reads, ra.n_reads_batch) + 1, false) || !ra.re_primary.ensure(std::max<uint64_t>(g.hw_chains, ra.n_chains) + 1, false)) { failed(RAWDTW_ERR_OOM, "host allocation failed"); return RAWDTW_ERR_OOM; }
        const rawdtw_chain_rec_t *d_recs = nullptr;
        int st = rawdtw_chain_round_recs(g.ctx, &d_recs);
        const rawdtw_select_opt_t so = select_opt(m);
        if (st == RAWDTW_OK) st = rawdtw_batch_round_end_begin(g.ctx, ra.batch, &so, d_recs, 1);
        p.round_end = st == RAWDTW_OK;
        // "resident_chains": the primary chains' anchors into the reads' other halves, right behind the round end that names them
        if (st == RAWDTW_OK && use_store()) { st = rawdtw_batch_round_end_keep(g.ctx, ra.batch, ra.keep_dst.p); p.keep = st == RAWDTW_OK; }
        return st;
    }

    // ---- a group's round with the chains made on the host: host phase, lay-out, submit (`events_done`: a round the device declined to chain --
    // its events are appended already, on both sides) ----
    void host_round(uint32_t gi, const RoundArrays *pv, bool events_done)
    {
        const RoundArrays &ra = m->groups[gi].buf[m->groups[gi].cur];
        m->pool->run(ra.ks.size(), 16, [&](size_t i) {
            const uint32_t k = ra.ks[i];
            const MRead &rd = read(k);
            if (events_done ? !rr[k].skipped : append_events(k))
                host_phase_chain(m, rd, rr[k], hits + hit_off[k], hit_off[k + 1] - hit_off[k], pv && rd.last_round == pv->round_id ? pv : nullptr, runs_dtw);
        });
        lap(0);
        for (uint32_t k : ra.ks) if (rr[k].err != RAWDTW_OK) failed(rr[k].err, "chaining failed (chain output buffers too small)");
        if (ok() && runs_dtw) lay_out_and_submit(gi, events_done);
    }

    // ---- lay-out: offsets by a running sum, then every read copies its own stretch; then the submission ----
    void lay_out_and_submit(uint32_t gi, bool events_done)
    {
        Group &g = m->groups[gi]; RoundArrays &ra = g.buf[g.cur];
        const size_t nr = ra.ks.size();
        Sizes n{nr};
        for (uint32_t k : ra.ks) {
            RoundRead &r = rr[k];
            r.chain0 = n.chains; r.anchor0 = n.anchors; r.new0 = n.new_anchors;
            n.chains += r.chains.size();
            for (size_t c = 0; c < r.chains.size(); c++) {
                n.anchors += r.chains[c].anchors.size();
                n.new_anchors += r.chains[c].anchors.size() - r.carry[c].parts; // (the new entries and, when a stretch is taken over, the junction)
            }
        }
        const uint64_t nc = n.chains, na = n.anchors;
        ra.n_chains = nc; ra.n_anchors = na;
        const bool stage = on_device && !events_done; // (an external scorer reads the host's copy of the events)
        if (!(stage ? stage_events(g, n, false, false) : size_arrays(g, n, false))) return;
        if (m->scorer) { ra.chain_seq.resize(nc); ra.chain_strand.resize(nc); }
        ra.chain_off[nr] = nc; ra.anchor_off[nc] = na;
        if (ra.carried) ra.new_off[nc] = n.new_anchors;
        ra.ref_base[nc] = 0; ra.read_base[nc] = 0; // (non-null, initialised arrays for a round without chains)
        ra.anchors[na] = rawdtw_anchor_t{0, 0};
        m->pool->run(nr, 32, [&](size_t i) {
            const uint32_t k = ra.ks[i];
            const RoundRead &r = rr[k];
            const uint32_t rb = arena_base(read(k));
            ra.chain_off[i] = r.chain0;
            uint64_t at = r.anchor0, nat = r.new0;
            for (size_t c = 0; c < r.chains.size(); c++) {
                const std::vector<rawdtw_anchor_t> &an = r.chains[c].anchors;
                const uint64_t cc = r.chain0 + c;
                ra.anchor_off[cc] = at;
                ra.ref_base[cc] = r.ref_base[c];
                ra.read_base[cc] = rb;
                if (m->scorer) { ra.chain_seq[cc] = r.chains[c].ref; ra.chain_strand[cc] = r.chains[c].strand; }
                memcpy(ra.anchors.p + at, an.data(), an.size() * sizeof(rawdtw_anchor_t));
                if (ra.carried) {
                    const uint64_t n_new = an.size() - r.carry[c].parts; // (with the junction)
                    ra.carry[cc] = r.carry[c];
                    ra.new_off[cc] = nat;
                    memcpy(ra.new_anchors.p + nat, an.data(), n_new * sizeof(rawdtw_anchor_t));
                    nat += n_new;
                }
                at += an.size();
            }
            if (stage) stage_chunk(ra, k);
        });
        lap(1);
        // ---- submit: the DTW block of gen_chains for every read of the group (rmap.cpp:509-530), one device submission ----
        if (on_device) {
            int st = upload_events(g, n, false);
            if (st == RAWDTW_OK && ra.carried) {
                st = rawdtw_batch_submit_carry(g.ctx, &m->opt.align, nr, ra.chain_off.p, ra.anchor_off.p, ra.anchors.p, ra.new_off.p, ra.new_anchors.p,
                                               ra.ref_base.p, ra.read_base.p, g.buf[g.cur ^ 1].batch, ra.carry.p, &ra.batch);
                if (st == RAWDTW_ERR_UNSUPPORTED) { ra.carried = false; st = RAWDTW_OK; } // (e.g. a round without a chain: nothing to plan on the device)
            }
            if (st == RAWDTW_OK && !ra.carried)
                st = rawdtw_batch_submit(g.ctx, &m->opt.align, nr, ra.chain_off.p, ra.anchor_off.p, ra.anchors.p, ra.ref_base.p, ra.read_base.p, &ra.batch);
            if (st != RAWDTW_OK) failed(st, rawdtw_last_error(g.ctx));
            m->timing[5] += (double)((ra.carried ? n.new_anchors : na) * sizeof(rawdtw_anchor_t));
            m->timing[6] += (double)(n.events * sizeof(float));
            m->timing[7] += (double)((nr + 1) * 8 + (nc + 1) * 8 + nc * 12 + (ra.carried ? nc * 32 + 8 : 0) + n.seg * 12);
        } else {
            std::vector<const float *> evp(nr);
            std::vector<uint32_t> evn(nr);
            for (size_t i = 0; i < nr; i++) { const MRead &rd = read(ra.ks[i]); evp[i] = rd.events.data(); evn[i] = (uint32_t)rd.events.size(); }
            if (m->scorer(m->scorer_user, nr, ra.chain_off.p, ra.anchor_off.p, ra.anchors.p, ra.chain_seq.data(), ra.chain_strand.data(), evp.data(), evn.data(),
                          ra.score.p, ra.keep.p) != 0)
                failed(RAWDTW_ERR_DEVICE, "the external scorer failed");
        }
        lap(2);
    }

    // ---- the staged events, shared by every path that sends a round's events up ----
    // A group's chunks laid out: every read's place in the staging (ev0), their sums into n.events / n.seg, the group's arrays sized by `n`, and
    // the segments written.  The chunks' copies are left to the caller's pass over the reads on the pool (stage_chunk).  false: no memory.
    bool stage_events(Group &g, Sizes &n, bool dev, bool in_place)
    {
        RoundArrays &ra = g.buf[g.cur];
        for (uint32_t k : ra.ks) { RoundRead &r = rr[k]; r.ev0 = n.events; n.events += r.ne; n.seg += r.ne ? 1 : 0; }
        if (!size_arrays(g, n, dev)) return false;
        write_segments(ra, in_place);
        return true;
    }
    void stage_chunk(RoundArrays &ra, uint32_t k) const
    {
        if (rr[k].ne) memcpy(ra.new_events.p + rr[k].ev0, events + event_off[k], rr[k].ne * sizeof(float));
    }
    // ... and sent to the group's arena: the caller's array in place (every read a segment), or the staging
    int upload_events(Group &g, const Sizes &n, bool in_place) const
    {
        const RoundArrays &ra = g.buf[g.cur];
        if (!n.seg) return RAWDTW_OK;
        if (in_place) return rawdtw_events_append(g.ctx, events, event_off[n_reads], (uint32_t)ra.ks.size(), event_off, ra.seg_dst.p);
        return rawdtw_events_append(g.ctx, ra.new_events.p, n.events, (uint32_t)n.seg, ra.seg_src.p, ra.seg_dst.p);
    }

    // the new events' segments: where each stretch of the staged events goes in the group's event arena -- the reads with a chunk this
    // round, in order.  In place: every read a segment, empty ones too (event_off itself is the table of sources).
    void write_segments(RoundArrays &ra, bool in_place)
    {
        uint64_t s = 0, at = 0;
        for (uint32_t k : ra.ks) {
            if (!rr[k].ne && !in_place) continue;
            if (!in_place) ra.seg_src[s] = at;
            ra.seg_dst[s++] = arena_base(read(k)) + rr[k].ev_before;
            at += rr[k].ne;
        }
        if (!in_place) ra.seg_src[s] = at;
    }

    // ---- per group: fetch (the only wait), then the round's end per read: gen_primary_chains, comp_mapq, the stop rule ----
    void fetch_and_end(uint32_t gi)
    {
        Group &g = m->groups[gi]; RoundArrays &ra = g.buf[g.cur];
        if (on_device && ra.batch) {
            const int st = rawdtw_batch_fetch(g.ctx, ra.batch, ra.score.p, ra.keep.p, nullptr); // (also after a failure elsewhere: the arrays it reads go out of use here)
            if (st != RAWDTW_OK) failed(st, rawdtw_last_error(g.ctx));
            uint64_t sc = 0, ru = 0;
            if (ok() && rawdtw_batch_round_stats(g.ctx, ra.batch, &sc, &ru) == RAWDTW_OK) { per[gi].scored = sc; per[gi].reused = ru; }
            if (per[gi].round_end) { // (also after a failure: the context's round end is begun and must be ended)
                const int se = rawdtw_batch_round_end_fetch(g.ctx, ra.batch, ra.re_out.p, ra.re_primary.p);
                if (se != RAWDTW_OK) failed(se, rawdtw_last_error(g.ctx));
                if (se == RAWDTW_OK && per[gi].keep) { // (a keep whose round end failed goes with the batch)
                    const int sk = rawdtw_batch_round_keep_fetch(g.ctx, ra.batch, ra.kept_count.p);
                    if (sk != RAWDTW_OK) failed(sk, rawdtw_last_error(g.ctx));
                }
            }
        }
        lap(3);
        if (!ok()) return;
        const bool evaluate = (m->opt.flag & 0x2) != 0, log_scores = (m->opt.flag & 0x8) != 0;
        const bool from_device = per[gi].round_end;
        m->pool->run(ra.ks.size(), 16, [&](size_t i) {
            const uint32_t k = ra.ks[i];
            RoundRead &r = rr[k];
            if (r.skipped) { r.high = high_confidence(m, read(k).chains); return; } // rmap.cpp:569-572: the chains stay as they were
            if (from_device && !(ra.re_out[r.bpos].flags & RAWDTW_ROUND_DECLINED)) { // primary, mapq and the stop rule's answer are the device's: the chains are moved
                const rawdtw_round_out_t &o = ra.re_out[r.bpos]; // (its read in the batch: a read the chaining declined alone has a pseudo-read)
                if (log_scores)
                    for (size_t c = 0; c < r.chains.size(); c++) {
                        const float as = ra.score[r.chain0 + c];
                        if (as == -1e10f) continue;
                        char line[128];
                        snprintf(line, sizeof line, "chaining_score=%f alignment_score=%f\n", (double)r.chains[c].chaining_score, (double)as);
                        r.log += line;
                    }
                r.primary.reserve(o.n_primary);
                for (uint32_t p = 0; p < o.n_primary; p++) {
                    const uint32_t c = ra.re_primary[r.chain0 + p];
                    r.chains[c].alignment_score = ra.score[r.chain0 + c];
                    r.primary.push_back(std::move(r.chains[c]));
                }
                if (o.n_primary) r.primary[0].mapq = o.mapq;
                r.high = (o.flags & RAWDTW_ROUND_HIGH) != 0;
                return;
            }
            std::vector<MChain> post;
            post.reserve(r.chains.size());
            for (size_t c = 0; c < r.chains.size(); c++) {
                MChain &ch = r.chains[c];
                bool keep = true;
                if (runs_dtw) {
                    ch.alignment_score = ra.score[r.chain0 + c];
                    keep = ra.keep[r.chain0 + c] != 0;
                    // --dtw-log-scores (rmap.cpp:308-312): in evaluation order; a cut chain returns before the fprintf
                    if (log_scores && ch.alignment_score != -1e10f) {
                        char line[128];
                        snprintf(line, sizeof line, "chaining_score=%f alignment_score=%f\n", (double)ch.chaining_score, (double)ch.alignment_score);
                        r.log += line;
                    }
                }
                if (!evaluate || !runs_dtw || keep) post.push_back(std::move(ch)); // rmap.cpp:525: replaced only under EVALUATE_CHAINS
            }
            r.primary = primary_chains(m, post);
            r.high = high_confidence(m, r.primary);
        });
        if (from_device) // (counted here, not by the pool's threads: sixteen of them adding to one counter cost the round more than its end)
            for (size_t i = 0; i < ra.ks.size(); i++) {
                if (rr[ra.ks[i]].skipped) continue;
                if (ra.re_out[rr[ra.ks[i]].bpos].flags & RAWDTW_ROUND_DECLINED) per[gi].re_declined++; else per[gi].re_reads++;
            }
        lap(4);
    }

    // ---- a failed round: the reads' events cut back, each group's round before stays the round before; nothing else was written ----
    // (A round from signal: the device has written the chunk's events into the arena above the read's committed n_events.  That stretch is
    // scratch -- nothing reads a slot beyond n_events -- and the next attempt's detection overwrites it from the same place.)
    int rollback()
    {
        for (uint32_t k = 0; k < n_reads; k++) {
            MRead &rd = read(k); const RoundRead &r = rr[k];
            if (rd.n_events >= r.ev_before && r.ne + r.ev_before == rd.n_events) {
                rd.n_events = r.ev_before; rd.offset = r.off_before;
                if (rd.events.size() > rd.n_events) rd.events.resize(rd.n_events);
            }
        }
        for (Group &g : m->groups) {
            RoundArrays &ra = g.buf[g.cur];
            if (ra.batch) { rawdtw_batch_destroy(ra.batch); ra.batch = nullptr; }
            g.cur ^= 1;
        }
        return fail(m, status, msg);
    }

    // ---- commit ----
    void commit()
    {
        m->rounds = id;
        if (per[0].round_end || per[1].round_end) m->re_rounds++;
        if (per[0].dc_reads || per[1].dc_reads) m->dc_rounds++;
        if (resident) {
            if (fell_back) { m->res_fallbacks++; m->res_hit_bytes += res_hits * sizeof(rawdtw_seed_hit_t); }
            else m->res_rounds++;
            m->res_seed_bytes += res_prev * sizeof(rawdtw_seed_t);
        }
        for (uint32_t gi = 0; gi < G; gi++) {
            Group &g = m->groups[gi];
            RoundArrays &ra = g.buf[g.cur], &pb = g.buf[g.cur ^ 1];
            if (pb.batch) { rawdtw_batch_destroy(pb.batch); pb.batch = nullptr; }
            g.has_prev = on_device && m->opt.carry && !m->opt.device_chain && ra.batch != nullptr;
            if (!g.has_prev && ra.batch) { rawdtw_batch_destroy(ra.batch); ra.batch = nullptr; }
            m->parts_scored += per[gi].scored; m->parts_reused += per[gi].reused;
            m->re_reads += per[gi].re_reads; m->re_declined += per[gi].re_declined;
            if (per[gi].dc_reads) {
                m->dc_reads_seeds += per[gi].dc_seeds; m->dc_reads_chains += per[gi].dc_chains; m->dc_reads_device += per[gi].dc_device;
                m->dc_seed_bytes += per[gi].dc_bytes;
            }
            for (size_t i = 0; i < ra.ks.size(); i++) { read(ra.ks[i]).last_round = id; read(ra.ks[i]).last_pos = i; }
            // "resident_chains": the one place a read's kept state changes.  A read that sat out keeps its chains and its state; a read whose
            // chains were kept is seeded from that half from now on; every other read's chains are new and not on the device
            // (a mapper that never had the option on has no read to clear: the loop is skipped)
            for (size_t i = 0; (use_store() || m->kp_any) && i < ra.ks.size(); i++) {
                MRead &rd = read(ra.ks[i]); const RoundRead &r = rr[ra.ks[i]];
                if (r.skipped) continue;
                if (use_store() && !fell_back && r.n_prev) { // (a round that fell back was chained on the host, from the host's chains)
                    if (r.from_store) { m->kp_reads_dev++; m->kp_seeds_dev += r.n_prev; } else { m->kp_reads_host++; m->kp_seeds_host += r.n_prev; }
                }
                if (per[gi].keep && ra.kept_count[i] != RAWDTW_NOT_KEPT) { rd.kept = MRead::Kept{true, (uint8_t)(ra.keep_dst[i] & 1u), ra.kept_count[i]}; m->kp_any = true; }
                else { rd.kept.valid = false; if (per[gi].keep) m->kp_not_kept++; }
            }
        }
        for (uint32_t k = 0; k < n_reads; k++) {
            MRead &rd = read(k); RoundRead &r = rr[k];
            if (!r.log.empty()) m->log += r.log;
            rd.chunks_done++;
            if (!on_device && r.ne) rd.host_only = true; // (none of this round's paths sent its events up)
            if (r.high) { rd.finished = true; rd.broke_early = true; } // rmap.cpp:692 (evaluated with the round's end, per read on the pool)
            else if (rd.chunks_done >= std::min(rd.n_chunks, m->opt.max_num_chunk)) rd.finished = true;
        }
        // the new chains in place, and the round's per-read state with the old chains freed, on the pool (ten vectors a read and more: freed one
        // read after the other they were milliseconds of a large round).  rmap.cpp:569-572: a skipped read's chains stay.
        m->pool->run(n_reads, 16, [&](size_t k) {
            if (!rr[k].skipped) std::swap(read((uint32_t)k).chains, rr[k].primary);
            RoundRead gone; std::swap(gone, rr[k]);
        });
        m->timing[4] += now_ms() - t0;
    }

    // The round itself: the reads dealt, every group's first half (`begin`: with device chaining every group's is begun before the first is
    // ended), the chains home, each group's round end (group gi's while group gi + 1's batch is on the device), then the one commit point.
    template <typename Begin> int run(Begin begin)
    {
        deal();
        for (uint32_t gi = 0; gi < G && ok(); gi++) begin(gi);
        for (uint32_t gi = 0; gi < G; gi++) end_device_chain(gi);
        for (uint32_t gi = 0; gi < G; gi++) fetch_and_end(gi);
        if (!ok()) return rollback();
        commit();
        return RAWDTW_OK;
    }
};

} // namespace

extern "C" {

int rawdtw_mapper_create(rawdtw_ctx *ctx, const rawdtw_mapper_opt_t *opt, uint32_t n_seq, const char *const *seq_names,
                         const uint32_t *seq_len, rawdtw_mapper **out)
{
    if (!out) return RAWDTW_ERR_INVALID;
    *out = nullptr;
    if (!opt || (n_seq && (!seq_names || !seq_len)) || opt->slot_events == 0 || opt->max_reads == 0) return RAWDTW_ERR_INVALID;
    if (opt->align.border_constraint != 0 && opt->align.border_constraint != 1) return RAWDTW_ERR_INVALID; // rmap.cpp:301-304
    rawdtw_mapper *m = new (std::nothrow) rawdtw_mapper;
    if (!m) return RAWDTW_ERR_OOM;
    m->ctx = ctx; m->opt = *opt;
    m->opt.groups = (ctx && opt->groups >= 2) ? 2 : 1;
    m->keep_host_events = !ctx || (opt->flag & 0x4) || !(opt->flag & (0x2 | 0x8));
    m->opt.threads = std::max(1, std::min(opt->threads, 256));
    for (uint32_t s = 0; s < n_seq; s++) { m->seq_names.emplace_back(seq_names[s]); m->seq_len.push_back(seq_len[s]); }
    m->ref_off.resize(2ull * n_seq);
    for (uint32_t s = 0; s < n_seq; s++)
        for (int st = 0; st < 2; st++) {
            uint64_t off = 2ull * s + (uint64_t)st;
            if (ctx && rawdtw_reference_offset(ctx, s, st, &off) != RAWDTW_OK) { delete m; return RAWDTW_ERR_INVALID; } // (no reference array for a sequence)
            m->ref_off[2ull * s + (uint64_t)st] = off;
        }
    m->groups.n = (size_t)m->opt.groups;
    m->groups[0].ctx = ctx;
    int st = RAWDTW_OK;
    if (m->opt.groups == 2) { // the second group's context: same device, the same resident reference
        int dev = 0;
        st = rawdtw_context_device(ctx, &dev);
        if (st == RAWDTW_OK) st = rawdtw_create(dev, &m->groups[1].ctx);
        if (st == RAWDTW_OK) { m->groups[1].own_ctx = true; st = rawdtw_share_reference(m->groups[1].ctx, ctx); }
        for (const char *name : {"chain_long_seeds", "chain_max_chains", "chain_decline_reads"}) // (both groups chain the same reads on the device)
            if (st == RAWDTW_OK) st = rawdtw_set_option(m->groups[1].ctx, name, ctx_option(ctx, name));
    }
    const uint64_t per_group = ((uint64_t)opt->max_reads + (uint64_t)m->opt.groups - 1) / (uint64_t)m->opt.groups;
    for (Group &g : m->groups)
        if (st == RAWDTW_OK && g.ctx) st = rawdtw_events_reserve(g.ctx, (uint64_t)opt->slot_events * per_group);
    if (st != RAWDTW_OK) { rawdtw_mapper_destroy(m); return st; }
    if (st == RAWDTW_OK && (opt->flag & 0x1)) st = rawdtw_su_create(n_seq, nullptr, &m->su); // RI_M_SEQUENCEUNTIL with roptions.c:43-46
    if (st != RAWDTW_OK) { rawdtw_mapper_destroy(m); return st; }
    m->pool = new (std::nothrow) Pool(m->opt.threads);
    if (!m->pool) { rawdtw_mapper_destroy(m); return RAWDTW_ERR_OOM; }
    *out = m;
    return RAWDTW_OK;
}

int rawdtw_mapper_destroy(rawdtw_mapper *m)
{
    if (!m) return RAWDTW_OK;
    drop_batches(m);
    m->seed_off.release(); m->seed_hits.release();
    for (Group &g : m->groups) {
        for (RoundArrays &ra : g.buf) ra = RoundArrays(); // (pinned memory goes before the context that may own the device)
        if (g.own_ctx && g.ctx) rawdtw_destroy(g.ctx);
    }
    rawdtw_su_destroy(m->su);
    delete m->pool;
    delete m;
    return RAWDTW_OK;
}

const char *rawdtw_mapper_last_error(const rawdtw_mapper *m) { return m ? m->err.c_str() : "null mapper"; }

int rawdtw_mapper_set_scorer(rawdtw_mapper *m, rawdtw_scorer_fn fn, void *user)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (fn) { // (an external scorer reads the host's copy of the reads' events: from the first round on -- no copy is kept by a mapper that
              // scores on the device only, nor of the chunks a round from signal detected on the device)
        for (const MRead &rd : m->reads)
            if (rd.n_events != rd.events.size() && !rd.released) return fail(m, RAWDTW_ERR_INVALID, "set the scorer before the first round");
        m->keep_host_events = true;
    }
    m->scorer = fn; m->scorer_user = user;
    drop_batches(m); // (a round scored elsewhere leaves nothing to carry from)
    return RAWDTW_OK;
}

int rawdtw_mapper_add_read(rawdtw_mapper *m, const char *name, uint32_t qlen, uint32_t n_chunks_available, uint32_t *read_id)
{
    if (!m || !name || !read_id) return RAWDTW_ERR_INVALID;
    uint32_t slot;
    if (!m->free_slots.empty()) { slot = m->free_slots.back(); m->free_slots.pop_back(); }
    else if (m->slots_used < m->opt.max_reads) slot = m->slots_used++;
    else return fail(m, RAWDTW_ERR_RANGE, "more reads than the mapper has slots for (rawdtw_mapper_release_read gives a finished read's slot back)");
    MRead r;
    r.name = name; r.qlen = qlen; r.n_chunks = n_chunks_available; r.slot = slot;
    if (m->su_stopped) { r.finished = true; r.dropped = true; } // sequence-until: the pipeline reads no further mini-batch (rmap.cpp:885)
    *read_id = (uint32_t)m->reads.size();
    m->reads.push_back(std::move(r));
    return RAWDTW_OK;
}

int rawdtw_mapper_release_read(rawdtw_mapper *m, uint32_t read_id)
{
    if (!m || read_id >= m->reads.size()) return RAWDTW_ERR_INVALID;
    MRead &rd = m->reads[read_id];
    if (rd.released) return RAWDTW_OK;
    if (!rd.finished) return fail(m, RAWDTW_ERR_INVALID, "only a finished read can be released");
    rd.released = true;
    std::vector<float>().swap(rd.events);
    std::vector<MChain>().swap(rd.chains);
    m->free_slots.push_back(rd.slot);
    return RAWDTW_OK;
}

int rawdtw_mapper_read_state(const rawdtw_mapper *m, uint32_t read_id, int *finished, uint32_t *chunks_done)
{
    if (!m || read_id >= m->reads.size()) return RAWDTW_ERR_INVALID;
    if (finished) *finished = m->reads[read_id].finished ? 1 : 0;
    if (chunks_done) *chunks_done = m->reads[read_id].chunks_done;
    return RAWDTW_OK;
}

int rawdtw_mapper_stats(const rawdtw_mapper *m, uint64_t *rounds, uint64_t *parts_scored, uint64_t *parts_reused)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (rounds) *rounds = m->rounds;
    if (parts_scored) *parts_scored = m->parts_scored;
    if (parts_reused) *parts_reused = m->parts_reused;
    return RAWDTW_OK;
}

int rawdtw_mapper_timing(const rawdtw_mapper *m, double out[8])
{
    if (!m || !out) return RAWDTW_ERR_INVALID;
    for (int i = 0; i < 8; i++) out[i] = m->timing[i];
    return RAWDTW_OK;
}

int rawdtw_mapper_log(const rawdtw_mapper *m, const char **text)
{
    if (!m || !text) return RAWDTW_ERR_INVALID;
    *text = m->log.c_str();
    return RAWDTW_OK;
}

} // extern "C"

namespace {

// a round's reads, every one checked before anything changes (`hit_off` null: a resident round, whose hits the host never sees;
// `event_off` null: a round from signal, whose event counts the device finds -- it checks them against the slots' room itself)
int check_round(rawdtw_mapper *m, uint32_t n_reads, const uint32_t *read_ids, const uint64_t *event_off, const uint64_t *hit_off, const rawdtw_seed_hit_t *hits)
{
    const uint32_t n_seq = (uint32_t)m->seq_len.size();
    const uint64_t stamp = m->rounds + 1;
    for (uint32_t k = 0; k < n_reads; k++) {
        if (read_ids[k] >= m->reads.size()) return fail(m, RAWDTW_ERR_INVALID, "unknown read id");
        MRead &rd = m->reads[read_ids[k]];
        bool dup = rd.seen_round == stamp;
        rd.seen_round = stamp;
        if (dup || rd.finished || rd.released || (event_off && event_off[k + 1] < event_off[k]) || (hit_off && hit_off[k + 1] < hit_off[k])) {
            for (uint32_t q = 0; q <= k; q++) m->reads[read_ids[q]].seen_round = 0;
            return fail(m, RAWDTW_ERR_INVALID, dup ? "a read twice in one round" : rd.finished || rd.released ? "a finished read in a round" : "offsets do not ascend");
        }
    }
    for (uint32_t k = 0; k < n_reads; k++) m->reads[read_ids[k]].seen_round = 0; // (a failed round does not count)
    for (uint32_t k = 0; event_off && k < n_reads; k++) {
        const MRead &rd = m->reads[read_ids[k]];
        if ((uint64_t)rd.n_events + (event_off[k + 1] - event_off[k]) > m->opt.slot_events) return fail(m, RAWDTW_ERR_RANGE, "a read outgrew its slot in the event arena");
        for (uint64_t h = hit_off ? hit_off[k] : 0; hit_off && h < hit_off[k + 1]; h++)
            if (hits[h].ref_seq >= n_seq) return fail(m, RAWDTW_ERR_INVALID, "seed hit on an unknown sequence");
    }
    return RAWDTW_OK;
}

} // namespace

extern "C" {

int rawdtw_mapper_round(rawdtw_mapper *m, uint32_t n_reads, const uint32_t *read_ids, const uint64_t *event_off, const float *events,
                        const uint64_t *hit_off, const rawdtw_seed_hit_t *hits)
{
    if (!m || (n_reads && (!read_ids || !event_off || !hit_off)) || (n_reads && event_off[n_reads] && !events) || (n_reads && hit_off[n_reads] && !hits))
        return RAWDTW_ERR_INVALID;
    if (n_reads == 0) return RAWDTW_OK;
    const double t0 = now_ms(); // (the checks and the round's set-up count as host phase, its commit as round end: the five times add up to the call)
    const bool runs_dtw = (m->opt.flag & (0x2 | 0x8)) != 0; // rmap.cpp:509
    if (runs_dtw && !m->scorer && !m->ctx) return fail(m, RAWDTW_ERR_NO_DEVICE, "a mapper without a context needs a scorer (rawdtw_mapper_set_scorer)");
    const int chk = check_round(m, n_reads, read_ids, event_off, hit_off, hits);
    if (chk != RAWDTW_OK) return chk;
    Round r{m, n_reads, read_ids, event_off, events, hit_off, hits, t0};
    return r.run([&r](uint32_t gi) { r.begin_group(gi); });
}

// what every seeded round asks of its index: one that can be read (its parameters out) and holds the mapper's sequences
static int seed_index_checks(rawdtw_mapper *m, const rawdtw_seed_index *six, rawdtw_seed_pars_t *pars)
{
    uint32_t six_seq = 0;
    if (rawdtw_seed_index_info(six, &six_seq, nullptr, nullptr, nullptr, pars) != RAWDTW_OK) return RAWDTW_ERR_INVALID;
    if (six_seq != m->seq_len.size()) return fail(m, RAWDTW_ERR_INVALID, "the seed index and the mapper hold different numbers of sequences");
    return RAWDTW_OK;
}

// a resident round's preconditions (each entry refuses in its own words).  no_cigar: nothing may read the host's copy of a read's events
// later either, which the --dtw-output-cigar traceback (rawdtw_mapper_finish) would
static bool resident_round_ok(const rawdtw_mapper *m, const rawdtw_seed_pars_t &pars, bool no_cigar)
{
    return m->ctx && !m->scorer && m->opt.device_chain && m->groups.size() == 1 && (pars.w == 0 || ctx_option(m->ctx, "seed_minimizer") != 0) &&
           !(no_cigar && (m->opt.flag & 0x4));
}

// The seeding of gen_chains (rmap.cpp:364-391) in front of the round.  Everything the seeding touches is the mapper's own buffers:
// the reads change only inside rawdtw_mapper_round, which runs on the finished hits or not at all.
int rawdtw_mapper_round_seeded(rawdtw_mapper *m, const rawdtw_seed_index *six, uint32_t n_reads, const uint32_t *read_ids,
                               const uint64_t *event_off, const float *events)
{
    if (!m || !six || (n_reads && (!read_ids || !event_off)) || (n_reads && event_off[n_reads] > event_off[0] && !events)) return RAWDTW_ERR_INVALID;
    rawdtw_seed_pars_t pars;
    if (const int st = seed_index_checks(m, six, &pars)) return st;
    if (n_reads == 0) return RAWDTW_OK;
    const bool on_device = m->ctx && (pars.w == 0 || ctx_option(m->ctx, "seed_minimizer") != 0); // (the minimizer sketch is the host's unless "seed_minimizer" is on)
    if (!seed_room(m, m->seed_off, (uint64_t)n_reads + 1)) return fail(m, RAWDTW_ERR_OOM, "no memory for the round's hit offsets");
    if (!on_device) {
        if (rawdtw_seed_index_is_resident(six)) return fail(m, RAWDTW_ERR_UNSUPPORTED, "host seeding needs the index's host copy: rawdtw_seed_index_fetch first");
        int st = rawdtw_seed_hits_host(six, n_reads, event_off, events, m->seed_off.p, nullptr, 0, m->opt.threads); // (counts)
        if (st != RAWDTW_OK && st != RAWDTW_ERR_RANGE) return fail(m, st, "seeding: bad event offsets");
        if (!seed_room(m, m->seed_hits, m->seed_off[n_reads])) return fail(m, RAWDTW_ERR_OOM, "no memory for the round's hits");
        st = rawdtw_seed_hits_host(six, n_reads, event_off, events, m->seed_off.p, m->seed_hits.p, m->seed_hits.cap, m->opt.threads);
        if (st != RAWDTW_OK) return fail(m, st, "seeding failed");
    } else {
        // (every round: the context knows its table by the index's serial and does nothing when this index is there already --
        // also right after the caller uploaded another index to the context, or rebuilt one at the old address)
        const int up = rawdtw_seed_index_upload(m->ctx, six);
        if (up != RAWDTW_OK) return fail(m, up, rawdtw_last_error(m->ctx));
        // the first guess: what the buffer holds, or four hits an event; a round with more says how many and is seeded once more
        uint64_t want = std::max<uint64_t>(m->seed_hits.cap, 4 * (event_off[n_reads] - event_off[0]) + 1024);
        for (int attempt = 0;; attempt++) {
            if (!seed_room(m, m->seed_hits, want)) return fail(m, RAWDTW_ERR_OOM, "no page-locked memory for the round's hits");
            int st = rawdtw_seed_begin(m->ctx, n_reads, event_off, events, m->seed_off.p, m->seed_hits.p, m->seed_hits.cap);
            if (st == RAWDTW_OK) st = rawdtw_seed_end(m->ctx, nullptr);
            if (st == RAWDTW_ERR_RANGE && attempt == 0 && m->seed_off[n_reads] > m->seed_hits.cap) { want = m->seed_off[n_reads]; continue; }
            if (st != RAWDTW_OK) return fail(m, st, rawdtw_last_error(m->ctx));
            break;
        }
    }
    return rawdtw_mapper_round(m, n_reads, read_ids, event_off, events, m->seed_off.p, m->seed_hits.p);
}

// rawdtw_mapper_round_seeded with the hits left on the device: the events are appended, the seeding reads them in the arena, and the
// chaining's seed list is written where the chaining reads it.  Everything it cannot do is refused before anything changes.
int rawdtw_mapper_round_seeded_resident(rawdtw_mapper *m, const rawdtw_seed_index *six, uint32_t n_reads, const uint32_t *read_ids,
                                        const uint64_t *event_off, const float *events)
{
    if (!m || !six || (n_reads && (!read_ids || !event_off)) || (n_reads && event_off[n_reads] > event_off[0] && !events)) return RAWDTW_ERR_INVALID;
    rawdtw_seed_pars_t pars;
    if (const int st = seed_index_checks(m, six, &pars)) return st;
    if (!resident_round_ok(m, pars, false))
        return fail(m, RAWDTW_ERR_UNSUPPORTED, "a resident round needs a context, device chaining, one read group, no external scorer and a w == 0 index, "
                                               "or a w > 0 one with the context's \"seed_minimizer\" option on (rawdtw_mapper_round_seeded maps the round)");
    if (n_reads == 0) return RAWDTW_OK;
    const double t0 = now_ms();
    const int chk = check_round(m, n_reads, read_ids, event_off, nullptr, nullptr);
    if (chk != RAWDTW_OK) return chk;
    if (!seed_room(m, m->seed_off, (uint64_t)n_reads + 1)) return fail(m, RAWDTW_ERR_OOM, "no memory for the round's hit offsets");
    const int up = rawdtw_seed_index_upload(m->ctx, six);
    // (the one thing the upload refuses here: a seeding somebody began on the mapper's context and has not ended)
    if (up == RAWDTW_ERR_INVALID) return fail(m, RAWDTW_ERR_UNSUPPORTED, rawdtw_last_error(m->ctx));
    if (up != RAWDTW_OK) return fail(m, up, rawdtw_last_error(m->ctx));
    Round r{m, n_reads, read_ids, event_off, events, nullptr, nullptr, t0};
    r.resident = true;
    // (seeding and chaining run on the device whether or not a DTW follows them: the round's arrays are the device path's, page-locked)
    r.on_device = true;
    r.events_in_place = event_off[n_reads] > 0 && rawdtw_host_is_page_locked(events) == 1;
    return r.run([&r](uint32_t gi) { r.resident_begin(gi); });
}

} // extern "C"

namespace {

// The round from signal: detection (the pA conversion in front of it for raw windows), seeding and chaining of one chunk round with no
// event on the host.  Detection and seeding are enqueued one behind the other and waited for once; only the counts come home.  They run
// before the round is set up and touch nothing of the mapper's but its own buffers, so whatever they refuse leaves reads and mapper as
// they were; from the counts on it is rawdtw_mapper_round_seeded_resident's round.
int round_from_signal(rawdtw_mapper *m, const rawdtw_seed_index *six, const rawdtw_event_opt_t *ev_opt, uint32_t n_reads, const uint32_t *read_ids,
                      const uint64_t *off, const float *sig, const int16_t *raw, const rawdtw_channel_t *chan, bool is_raw)
{
    if (!m || !six || (n_reads && (!read_ids || !off)) || (n_reads && off[n_reads] > off[0] && (is_raw ? !raw : !sig)) || (n_reads && is_raw && !chan))
        return m ? fail(m, RAWDTW_ERR_INVALID, "null argument") : RAWDTW_ERR_INVALID;
    rawdtw_seed_pars_t pars;
    if (const int st = seed_index_checks(m, six, &pars)) return st;
    // rawdtw_mapper_round_seeded_resident's preconditions, and nothing may read the host's copy of a read's events later: that is the
    // --dtw-output-cigar traceback and an external scorer.  A mapper with no DTW stage keeps the copy for neither.
    // With the context's "signal_cigar" on (read once a round) the traceback reads the arena instead, and flag 0x4 alone refuses nothing.
    const bool cigar_from_arena = ctx_option(m->ctx, "signal_cigar") != 0;
    if (!resident_round_ok(m, pars, !cigar_from_arena))
        return fail(m, RAWDTW_ERR_UNSUPPORTED, cigar_from_arena
                        ? "a round from signal needs a context, device chaining, one read group, no external scorer and a w == 0 index, or a w > 0 one "
                          "with the context's \"seed_minimizer\" option on (rawdtw_detect_raw_begin + rawdtw_mapper_round_seeded_resident map the round)"
                        : "a round from signal needs a context, device chaining, one read group, no external scorer, no --dtw-output-cigar "
                          "and a w == 0 index, or a w > 0 one with the context's \"seed_minimizer\" option on "
                          "(rawdtw_detect_raw_begin + rawdtw_mapper_round_seeded_resident map the round)");
    if (n_reads == 0) return RAWDTW_OK;
    const double t0 = now_ms();
    const int chk = check_round(m, n_reads, read_ids, nullptr, nullptr, nullptr);
    if (chk != RAWDTW_OK) return chk;
    const uint64_t nr = n_reads;
    if (!seed_room(m, m->seed_off, nr + 1) || !m->sig_dst.ensure(nr, false) || !m->sig_room.ensure(nr, false) || !m->sig_evlen.ensure(nr, false))
        return fail(m, RAWDTW_ERR_OOM, "no memory for the round's tables");
    for (uint32_t k = 0; k < n_reads; k++) { // the chunk goes behind the read's committed events, and may fill its slot
        const MRead &rd = m->reads[read_ids[k]];
        m->sig_dst[k] = (uint64_t)rd.slot * m->opt.slot_events + rd.n_events;
        m->sig_room[k] = m->opt.slot_events - std::min(rd.n_events, m->opt.slot_events);
    }
    const int up = rawdtw_seed_index_upload(m->ctx, six);
    if (up == RAWDTW_ERR_INVALID) return fail(m, RAWDTW_ERR_UNSUPPORTED, rawdtw_last_error(m->ctx)); // (somebody's seeding is begun on the context)
    if (up != RAWDTW_OK) return fail(m, up, rawdtw_last_error(m->ctx));
    // events_cap, the first guess: what the seeding's workspace holds already, or a quarter of the samples; a round with more says how many and
    // runs once more (as rawdtw_mapper_round_seeded does for its hits)
    const uint64_t n_samples = off[n_reads] - off[0];
    const int64_t first_cap = ctx_option(m->ctx, "signal_events_cap");
    uint64_t cap = first_cap > 0 ? (uint64_t)first_cap : std::max<uint64_t>(m->sig_cap, n_samples / 4 + 1024);
    uint64_t total = 0;
    bool retried = false;
    for (int attempt = 0;; attempt++) {
        int st = is_raw ? rawdtw_detect_raw_resident_begin(m->ctx, ev_opt, n_reads, off, raw, chan, m->sig_dst.p, m->sig_room.p, cap)
                        : rawdtw_detect_resident_begin(m->ctx, ev_opt, n_reads, off, sig, m->sig_dst.p, m->sig_room.p, cap);
        if (st != RAWDTW_OK) return fail(m, st, rawdtw_last_error(m->ctx));
        const int sb = rawdtw_seed_detected_begin(m->ctx, m->seed_off.p);
        // the one wait: both ends (the detection's first -- it is ended whatever the seeding's begin said)
        st = rawdtw_detect_resident_end(m->ctx, nullptr, m->sig_evlen.p, &total, nullptr);
        std::string msg = st != RAWDTW_OK ? rawdtw_last_error(m->ctx) : "";
        if (sb != RAWDTW_OK) return fail(m, sb, rawdtw_last_error(m->ctx));
        const int se = rawdtw_seed_resident_end(m->ctx, nullptr);
        if (st == RAWDTW_OK && se == RAWDTW_OK) break;
        if (st == RAWDTW_ERR_RANGE) {
            for (uint32_t k = 0; k < n_reads; k++)
                if (m->sig_evlen[k] > m->sig_room[k]) return fail(m, RAWDTW_ERR_RANGE, "a read outgrew its slot in the event arena");
            if (attempt == 0 && total > cap) { cap = total; retried = true; continue; }
        }
        return st != RAWDTW_OK ? fail(m, st, msg) : fail(m, se, rawdtw_last_error(m->ctx));
    }
    m->sig_cap = std::max(m->sig_cap, cap);
    m->sig_evoff.resize(nr + 1);
    m->sig_evoff[0] = 0;
    for (uint32_t k = 0; k < n_reads; k++) m->sig_evoff[k + 1] = m->sig_evoff[k] + m->sig_evlen[k];
    Round r{m, n_reads, read_ids, m->sig_evoff.data(), nullptr, nullptr, nullptr, t0};
    r.resident = true; r.signal = true;
    r.on_device = true; // (as rawdtw_mapper_round_seeded_resident)
    r.events_in_place = false;
    if (const int st = r.run([&r](uint32_t gi) { r.signal_begin(gi); })) return st;
    m->sig_rounds++;
    if (m->opt.flag & 0x4) m->finish_from_arena = true; // (only with "signal_cigar" on does such a mapper get here)
    if (retried) m->sig_retried++;
    m->sig_sample_bytes += n_samples * (is_raw ? sizeof(int16_t) : sizeof(float)) * (retried ? 2 : 1);
    return RAWDTW_OK;
}

} // namespace

extern "C" {

int rawdtw_mapper_round_signal_resident(rawdtw_mapper *m, const rawdtw_seed_index *six, const rawdtw_event_opt_t *ev_opt, uint32_t n_reads,
                                        const uint32_t *read_ids, const uint64_t *sig_off, const float *sig)
{
    return round_from_signal(m, six, ev_opt, n_reads, read_ids, sig_off, sig, nullptr, nullptr, false);
}

int rawdtw_mapper_round_raw_resident(rawdtw_mapper *m, const rawdtw_seed_index *six, const rawdtw_event_opt_t *ev_opt, uint32_t n_reads,
                                     const uint32_t *read_ids, const uint64_t *raw_off, const int16_t *raw, const rawdtw_channel_t *chan)
{
    return round_from_signal(m, six, ev_opt, n_reads, read_ids, raw_off, nullptr, raw, chan, true);
}

int rawdtw_mapper_signal_stats(const rawdtw_mapper *m, uint64_t *rounds, uint64_t *retried_rounds, uint64_t *sample_bytes_to_device,
                               uint64_t *event_bytes_crossed)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (rounds) *rounds = m->sig_rounds;
    if (retried_rounds) *retried_rounds = m->sig_retried;
    if (sample_bytes_to_device) *sample_bytes_to_device = m->sig_sample_bytes;
    if (event_bytes_crossed) *event_bytes_crossed = (uint64_t)m->timing[6]; // (the mapper sends events up and fetches none: slot 6 is all that crosses)
    return RAWDTW_OK;
}

// A read's committed events: where the mapper's rounds put them -- its slot of its group's arena (one segment of rawdtw_events_fetch) on a
// mapper with a context, the host's copy on one without, for a read some of whose rounds ran nothing on the device, and once a finish
// through the host's copies has replaced the arena (such a mapper kept every read's copy).
int rawdtw_mapper_read_events(rawdtw_mapper *m, uint32_t read_id, float *out, uint32_t cap, uint32_t *n)
{
    if (!m || !n) return RAWDTW_ERR_INVALID;
    *n = 0;
    if (read_id >= m->reads.size()) return fail(m, RAWDTW_ERR_INVALID, "unknown read id");
    const MRead &rd = m->reads[read_id];
    if (rd.released) return fail(m, RAWDTW_ERR_INVALID, "a released read has no events");
    *n = rd.n_events;
    if (cap < rd.n_events) return fail(m, RAWDTW_ERR_RANGE, "cap is below the read's events");
    if (rd.n_events == 0) return RAWDTW_OK;
    if (!out) return fail(m, RAWDTW_ERR_INVALID, "null argument");
    if (m->ctx && !rd.host_only && !m->arena_replaced) {
        uint32_t start = 0;
        rawdtw_ctx *ctx = slot_of(m, rd, &start);
        const uint32_t len = rd.n_events;
        uint64_t off[2];
        const int st = rawdtw_events_fetch(ctx, 1, &start, &len, off, out, cap);
        return st == RAWDTW_OK ? RAWDTW_OK : fail(m, st, rawdtw_last_error(ctx));
    }
    if (rd.events.size() != rd.n_events) return fail(m, RAWDTW_ERR_UNSUPPORTED, "the read's events are neither all in the arena nor all on the host");
    memcpy(out, rd.events.data(), (size_t)rd.n_events * sizeof(float));
    return RAWDTW_OK;
}

int rawdtw_mapper_round_end_stats(const rawdtw_mapper *m, uint64_t *rounds, uint64_t *reads_device, uint64_t *reads_declined)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (rounds) *rounds = m->re_rounds;
    if (reads_device) *reads_device = m->re_reads;
    if (reads_declined) *reads_declined = m->re_declined;
    return RAWDTW_OK;
}

int rawdtw_mapper_kept_stats(const rawdtw_mapper *m, uint64_t *reads_from_device, uint64_t *reads_from_host, uint64_t *seeds_from_device,
                             uint64_t *seeds_from_host, uint64_t *reads_not_kept)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (reads_from_device) *reads_from_device = m->kp_reads_dev;
    if (reads_from_host) *reads_from_host = m->kp_reads_host;
    if (seeds_from_device) *seeds_from_device = m->kp_seeds_dev;
    if (seeds_from_host) *seeds_from_host = m->kp_seeds_host;
    if (reads_not_kept) *reads_not_kept = m->kp_not_kept;
    return RAWDTW_OK;
}

int rawdtw_mapper_decline_stats(const rawdtw_mapper *m, uint64_t *rounds_with_declines, uint64_t *reads_declined_seeds, uint64_t *reads_declined_chains,
                                uint64_t *reads_chained_device, uint64_t *seed_bytes_to_host)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (rounds_with_declines) *rounds_with_declines = m->dc_rounds;
    if (reads_declined_seeds) *reads_declined_seeds = m->dc_reads_seeds;
    if (reads_declined_chains) *reads_declined_chains = m->dc_reads_chains;
    if (reads_chained_device) *reads_chained_device = m->dc_reads_device;
    if (seed_bytes_to_host) *seed_bytes_to_host = m->dc_seed_bytes;
    return RAWDTW_OK;
}

int rawdtw_mapper_resident_stats(const rawdtw_mapper *m, uint64_t *resident_rounds, uint64_t *fallback_rounds, uint64_t *hit_bytes_to_host,
                                 uint64_t *seed_bytes_to_device)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (resident_rounds) *resident_rounds = m->res_rounds;
    if (fallback_rounds) *fallback_rounds = m->res_fallbacks;
    if (hit_bytes_to_host) *hit_bytes_to_host = m->res_hit_bytes;
    if (seed_bytes_to_device) *seed_bytes_to_device = m->res_seed_bytes;
    return RAWDTW_OK;
}

// --dtw-output-cigar (rmap.cpp:715-717): the best chain of every mapped read through DTW_global_tb once more, its path as the
// aln:s: string with the reference's two quirks (rmap.cpp:230-233, 283-289).  All reads' jobs go to the device in ONE call;
// the paths come back as steps and distances (rawdtw_traceback_batch_steps: 5 bytes an element) and every read's string is
// written on the pool while the steps are walked.
int rawdtw_mapper_finish(rawdtw_mapper *m)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (!(m->opt.flag & 0x4)) return RAWDTW_OK;
    if (!m->ctx) return fail(m, RAWDTW_ERR_NO_DEVICE, "--dtw-output-cigar needs a device context");
    // Where a read's events are: in the host's copy, laid one read behind the other and uploaded by the traceback call -- or, once a round from
    // signal has been committed ("signal_cigar": no host copy of its chunks exists), where every round of a context mapper put them: the read's slot
    // of the arena, which the traceback then reads as it lies.  The event base of a read's jobs and the traceback entry are all that differs.
    const bool arena = m->finish_from_arena;
    if (arena)
        for (const MRead &rd : m->reads)
            if (rd.host_only && !rd.released && !rd.dropped && high_confidence(m, rd.chains))
                return fail(m, RAWDTW_ERR_UNSUPPORTED, "a mapped read has events from a round that ran nothing on the device: they are not in the event arena");
    if (!arena) drop_batches(m); // (the traceback call replaces the event arena's contents: the mapper's rounds are over)
    struct Item { uint32_t read; uint64_t job0; uint32_t nj; uint64_t ev0; };
    std::vector<Item> items;
    std::vector<rawdtw_job_t> jobs;
    std::vector<float> events;
    for (uint32_t r = 0; r < m->reads.size(); r++) {
        MRead &rd = m->reads[r];
        if (rd.released || rd.dropped || !high_confidence(m, rd.chains)) continue;
        MChain &ch = rd.chains[0];
        const uint32_t na = (uint32_t)ch.anchors.size();
        const uint32_t nj = rawdtw_chain_job_count(&m->opt.align, na);
        if (!arena && (uint64_t)events.size() + rd.events.size() >= (1ull << 32)) return fail(m, RAWDTW_ERR_RANGE, "the mapped reads' events exceed one event arena");
        uint32_t ev_base = (uint32_t)events.size();
        if (arena) (void)slot_of(m, rd, &ev_base); // (one read group: the arena is the mapper's context's)
        const uint64_t j0 = jobs.size();
        jobs.resize(j0 + std::max<uint32_t>(nj, 1));
        const uint64_t rb = m->ref_off[ch.ref * 2u + (uint32_t)ch.strand];
        const int st = rawdtw_chain_build_jobs(&m->opt.align, ch.anchors.data(), na, rb, ev_base, 1, jobs.data() + j0);
        if (st != RAWDTW_OK) return fail(m, st, st == RAWDTW_ERR_UNSUPPORTED ? "banded global alignment with --dtw-output-cigar is not implemented (rmap.cpp:223-225)" : "job building failed");
        jobs.resize(j0 + nj);
        items.push_back(Item{r, j0, nj, ev_base});
        if (!arena) events.insert(events.end(), rd.events.begin(), rd.events.end());
    }
    if (items.empty()) return RAWDTW_OK;
    const uint64_t nj_all = jobs.size();
    std::vector<uint64_t> poff(nj_all + 1, 0);
    for (uint64_t k = 0; k < nj_all; k++) poff[k + 1] = poff[k] + jobs[k].n + jobs[k].m - 1;
    std::vector<uint32_t> plen(nj_all);
    std::vector<uint8_t> step(poff[nj_all] + 1);
    std::vector<float> pd(poff[nj_all] + 1), cost(nj_all);
    if (nj_all) {
        if (!arena) m->arena_replaced = true;
        const int st = arena ? rawdtw_traceback_arena_steps(m->ctx, jobs.data(), nj_all, cost.data(), poff.data(), plen.data(), step.data(), pd.data())
                             : rawdtw_traceback_batch_steps(m->ctx, jobs.data(), nj_all, events.data(), events.size(), cost.data(), poff.data(), plen.data(), step.data(), pd.data());
        if (st != RAWDTW_OK) return fail(m, st, rawdtw_last_error(m->ctx));
    }
    std::vector<std::string> logs(items.size());
    m->pool->run(items.size(), 4, [&](size_t x) {
        const Item &it = items[x];
        MRead &rd = m->reads[it.read];
        MChain &ch = rd.chains[0];
        const uint32_t na = (uint32_t)ch.anchors.size(), nj = it.nj;
        ch.alignment_score = rawdtw_chain_replay(&m->opt.align, ch.anchors.data(), na, cost.data() + it.job0, -1e10f); // rmap.cpp:306 on the summed costs
        std::string s;
        const uint32_t parts = na - 1;
        char el[96];
        for (uint32_t k = 0; k < nj; k++) {
            // sparse: every element offset by its part's start anchor (rmap.cpp:286-289); global: the offsets are added to
            // alignment.back() once per element (rmap.cpp:230-233), i.e. only the last tuple moves
            const rawdtw_anchor_t &s0 = m->opt.align.border_constraint == 0 ? ch.anchors[na - 1] : ch.anchors[parts - k];
            const uint64_t p0 = poff[it.job0 + k];
            const uint32_t len = plen[it.job0 + k];
            unsigned long long pi = 0, pj = 0; // (i, j) from the steps: a global path starts at (0, 0)
            for (uint32_t q = 0; q < len; q++) {
                pi += step[p0 + q] & 1u; pj += step[p0 + q] >> 1;
                unsigned long long i = pi, j = pj;
                if (m->opt.align.border_constraint != 0) { i += s0.query_position; j += s0.target_position; }
                else if (q + 1 == len) { i += (unsigned long long)len * s0.query_position; j += (unsigned long long)len * s0.target_position; }
                snprintf(el, sizeof el, "(%llu,%llu,%g)", i, j, (double)pd[p0 + q]); // ostream << float == %g (rmap.cpp:580-592)
                s += el;
            }
        }
        ch.aln = std::move(s);
        ch.has_aln = true;
        if (m->opt.flag & 0x8) {
            char line[128];
            snprintf(line, sizeof line, "chaining_score=%f alignment_score=%f\n", (double)ch.chaining_score, (double)ch.alignment_score);
            logs[x] = line;
        }
    });
    for (const std::string &l : logs) m->log += l; // (read order)
    return RAWDTW_OK;
}

// The PAF line of one read (rmap.cpp:696-801 for the fields and tags, 956-965 for the format).  `mt:f:` is wall-clock in the
// reference and therefore written as 0 here.
int rawdtw_mapper_paf(const rawdtw_mapper *m, uint32_t read_id, char *buf, uint32_t cap, uint32_t *len)
{
    if (!m || read_id >= m->reads.size() || !len || m->reads[read_id].released) return RAWDTW_ERR_INVALID;
    const MRead &rd = m->reads[read_id];
    if (rd.dropped) { // sequence-until: no line
        *len = 0;
        if (buf && cap) buf[0] = 0;
        return buf && !cap ? RAWDTW_ERR_RANGE : RAWDTW_OK;
    }
    const uint32_t l_chunk = m->opt.chunk_size, max_chunk = m->opt.max_num_chunk;
    uint32_t current_chunk = rd.broke_early ? rd.chunks_done - 1 : rd.chunks_done; // the loop's current_chunk when it exits
    const uint64_t chunk_start = (uint64_t)current_chunk * l_chunk;
    // rmap.cpp:696: step back one chunk when the loop ran out of signal or chunks rather than breaking
    if (!rd.broke_early && current_chunk > 0 && (chunk_start >= rd.qlen || current_chunk == max_chunk)) current_chunk -= 1;
    const uint32_t offset = rd.offset; // reg0->offset: the events of the chunks that were chained (rmap.cpp:574-575)
    // rmap.cpp:698, float arithmetic throughout
    const float scale = offset ? ((float)(current_chunk + 1) * (float)l_chunk / (float)offset) / ((float)m->opt.sample_rate / (float)m->opt.bp_per_sec)
                               : INFINITY;
    const std::vector<MChain> &chains = rd.chains;
    const uint32_t n_chains = (uint32_t)chains.size(), n_anchors0 = n_chains ? (uint32_t)chains[0].anchors.size() : 0;
    float mean_chain_score = 0.f;
    for (const MChain &c : chains) mean_chain_score += c.chaining_score;
    if (n_chains) mean_chain_score /= (float)n_chains;
    const bool mapped = high_confidence(m, chains);
    float at = 0.f, aq = 0.f;
    if (n_chains) { // rmap.cpp:719-724: uint32 differences accumulated in float
        const std::vector<rawdtw_anchor_t> &a = chains[0].anchors;
        for (uint32_t ai = 0; ai + 1 < n_anchors0; ai++) {
            at += (float)(uint32_t)(a[ai].target_position - a[ai + 1].target_position);
            aq += (float)(uint32_t)(a[ai].query_position - a[ai + 1].query_position);
        }
        if (n_anchors0) { at /= (float)n_anchors0; aq /= (float)n_anchors0; }
    }
    std::string tags = "mt:f:" + fmt_f(0.0) + "\tci:i:" + std::to_string(current_chunk + 1) + "\tsl:i:" + std::to_string(rd.qlen);
    std::string line;
    char head[512];
    if (n_chains) {
        tags += "\tcm:i:" + std::to_string(n_anchors0) + "\tnc:i:" + std::to_string(n_chains) + "\ts1:f:" + fmt_f(chains[0].chaining_score) + "\ts2:f:" +
                fmt_f(n_chains > 1 ? (double)chains[1].chaining_score : 0.0) + "\tsm:f:" + fmt_f(mean_chain_score) + "\tat:f:" + fmt_f(at) + "\taq:f:" + fmt_f(aq);
    } else tags += "\tcm:i:0\tnc:i:0\ts1:f:0\ts2:f:0\tsm:f:0\tat:f:0\taq:f:0";
    if (mapped) {
        const MChain &c0 = chains[0];
        if ((m->opt.flag & 0x4) && c0.has_aln) tags += "\talns:f:" + fmt_f(c0.alignment_score) + "\taln:s:" + c0.aln;
        const std::vector<rawdtw_anchor_t> &a = c0.anchors;
        if (m->opt.flag & 0x20) { // --output-chains (rmap.cpp:745-747, anchors_to_string at 53-63): "(query,target)" per anchor, end-first
            tags += "\tanchors:s:";
            for (const rawdtw_anchor_t &x : a) tags += "(" + std::to_string(x.query_position) + "," + std::to_string(x.target_position) + ")";
        }
        const uint32_t read_end = (uint32_t)(scale * (float)a[0].query_position);
        const uint32_t read_start = (uint32_t)(scale * (float)a[n_anchors0 - 1].query_position);
        const uint32_t ref_len = m->seq_len[c0.ref];
        const uint32_t frag_start = c0.strand ? ref_len + 1u - c0.end_position : c0.start_position; // rmap.cpp:751
        const uint32_t frag_len = c0.end_position - c0.start_position + 1u;
        if (rd.gated) // sequence-until: at or after the stop point of its batch (rmap.cpp:960, 965 with the mapped read's values)
            snprintf(head, sizeof head, "%s\t%u\t*\t*\t*\t*\t*\t*\t*\t*\t*\t%d\t", rd.name.c_str(), read_end, (int)c0.mapq);
        else
            snprintf(head, sizeof head, "%s\t%u\t%u\t%u\t%s\t%s\t%u\t%u\t%u\t%u\t%u\t%d\t", rd.name.c_str(), read_end, read_start, read_end,
                     c0.strand ? "-" : "+", m->seq_names[c0.ref].c_str(), ref_len, frag_start, frag_start + frag_len, read_end - read_start - 1u, frag_len,
                     (int)c0.mapq); // rmap.cpp:961-963
        line = head + tags;
    } else {
        const uint32_t read_length = offset ? (uint32_t)(scale * (float)offset) : 0u;
        snprintf(head, sizeof head, "%s\t%u\t*\t*\t*\t*\t*\t*\t*\t*\t*\t%d\t", rd.name.c_str(), read_length, 0); // rmap.cpp:965
        line = head + tags;
    }
    *len = (uint32_t)line.size();
    if (buf && cap) {
        const uint32_t n = std::min<uint32_t>(cap - 1, (uint32_t)line.size());
        memcpy(buf, line.data(), n);
        buf[n] = 0;
    }
    return (buf && cap > line.size()) || !buf ? RAWDTW_OK : RAWDTW_ERR_RANGE;
}

int rawdtw_mapper_set_sequence_until(rawdtw_mapper *m, const rawdtw_su_opt_t *opt)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (m->su_closed_any) return fail(m, RAWDTW_ERR_INVALID, "set sequence-until before the first batch is closed");
    rawdtw_su *su = nullptr;
    const int st = rawdtw_su_create((uint32_t)m->seq_len.size(), opt, &su);
    if (st != RAWDTW_OK) return fail(m, st, "bad sequence-until parameters (n_seq, tn_samples and ttest_freq must be > 0)");
    rawdtw_su_destroy(m->su);
    m->su = su;
    return RAWDTW_OK;
}

int rawdtw_mapper_batch_records(const rawdtw_mapper *m, uint32_t n, const uint32_t *read_ids, uint8_t *mapped, uint32_t *ref_id,
                                uint32_t *fragment_length)
{
    if (!m || (n && (!read_ids || !mapped || !ref_id || !fragment_length))) return RAWDTW_ERR_INVALID;
    for (uint32_t k = 0; k < n; k++)
        if (read_ids[k] >= m->reads.size() || m->reads[read_ids[k]].released || !m->reads[read_ids[k]].finished) return RAWDTW_ERR_INVALID;
    for (uint32_t k = 0; k < n; k++) su_record(m, m->reads[read_ids[k]], mapped + k, ref_id + k, fragment_length + k);
    return RAWDTW_OK;
}

int rawdtw_mapper_su_apply(rawdtw_mapper *m, uint32_t n, const uint32_t *read_ids, uint32_t first_gated)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (first_gated != RAWDTW_SU_NO_STOP && first_gated > n) return fail(m, RAWDTW_ERR_INVALID, "first_gated past the batch");
    const int st = su_check_batch(m, n, read_ids);
    if (st != RAWDTW_OK) return st;
    m->su_closed_any = true;
    const bool was_stopped = m->su_stopped;
    for (uint32_t k = 0; k < n; k++) {
        MRead &rd = m->reads[read_ids[k]];
        rd.closed = true;
        if (was_stopped) continue; // (dropped when the stop fired: still no line)
        if (first_gated != RAWDTW_SU_NO_STOP && k >= first_gated) rd.gated = true;
        else if (high_confidence(m, rd.chains)) m->su_mapped++;
    }
    if (was_stopped || first_gated == RAWDTW_SU_NO_STOP) return RAWDTW_OK;
    // the stop: the pipeline ends at step 0 of the next mini-batch (rmap.cpp:885) -- what is not in a closed batch is never mapped
    m->su_stopped = true;
    for (MRead &rd : m->reads)
        if (!rd.released && !rd.closed) { rd.finished = true; rd.dropped = true; }
    return RAWDTW_OK;
}

int rawdtw_mapper_su_batch(rawdtw_mapper *m, uint32_t n, const uint32_t *read_ids, uint32_t *stop)
{
    if (!m || !stop) return RAWDTW_ERR_INVALID;
    int st = su_check_batch(m, n, read_ids);
    if (st != RAWDTW_OK) return st;
    std::vector<uint8_t> mapped(n);
    std::vector<uint32_t> ref_id(n), frag(n);
    for (uint32_t k = 0; k < n; k++) su_record(m, m->reads[read_ids[k]], &mapped[k], &ref_id[k], &frag[k]);
    uint32_t s = 0;
    st = rawdtw_su_feed(m->su, n, mapped.data(), ref_id.data(), frag.data(), &s);
    if (st != RAWDTW_OK) return fail(m, st, "rawdtw_su_feed failed");
    // (a batch after the stop: its reads were dropped and stay without a line; the feed counted nothing and repeats the stop)
    st = rawdtw_mapper_su_apply(m, n, read_ids, s && !m->su_stopped ? s : RAWDTW_SU_NO_STOP);
    if (st != RAWDTW_OK) return st;
    *stop = s;
    return RAWDTW_OK;
}

int rawdtw_mapper_su_state(const rawdtw_mapper *m, int *stopped, uint32_t *n_mapped_at_stop)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (stopped) *stopped = m->su_stopped ? 1 : 0;
    if (n_mapped_at_stop) *n_mapped_at_stop = m->su_stopped ? m->su_mapped : 0u;
    return RAWDTW_OK;
}

} // extern "C"
