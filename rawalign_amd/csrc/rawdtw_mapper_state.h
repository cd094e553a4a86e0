// rawdtw_mapper_state.h -- what the two halves of the chunk-round mapper share: the mapper's state (rawdtw_mapper.cpp creates, reads and
// destroys it; rawdtw_mapper_round.cpp runs the rounds over it) and the few helpers both use.  Only include/rawdtw.h and the standard library.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rawdtw.h"
#include "rawdtw_pool.h"

namespace rawdtw_map {

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

// one round's arrays of one read group, as handed to the device (and kept for the next round's matching).  Which path of a round needs
// which of the buffers, how large and in what memory: Round::grow (rawdtw_mapper_round.cpp), the one place they are sized.
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

// Every counter the stats entries report (rawdtw_mapper_stats, _resident_stats, _signal_stats, _round_end_stats, _kept_stats,
// _decline_stats) and the three byte counters of rawdtw_mapper_timing's slots 5-7: once on the mapper, once on a round, which fills its
// own and adds it at its commit.
#define RAWDTW_MAPPER_COUNTERS(X) \
    X(rounds) X(parts_scored) X(parts_reused) \
    /* resident rounds; those that fell back as a whole and the hits they fetched; previous anchors sent up as seeds */ \
    X(res_rounds) X(res_fallbacks) X(res_hit_bytes) X(res_seed_bytes) \
    /* rounds from signal */ \
    X(sig_rounds) X(sig_retried) X(sig_sample_bytes) \
    /* "device_round_end": rounds whose end ran on the device, the reads it ended and the reads it declined */ \
    X(re_rounds) X(re_reads) X(re_declined) \
    /* "resident_chains": reads with previous seeds taken from the device / sent up from the host, those seeds, and reads whose chains a \
       keep launch did not keep */ \
    X(kp_reads_dev) X(kp_reads_host) X(kp_seeds_dev) X(kp_seeds_host) X(kp_not_kept) \
    /* "chain_decline_reads": rounds in which the device chaining declined reads alone, those reads by reason, the reads it chained in \
       such rounds, and the declined reads' seeds a resident round brought home */ \
    X(dc_rounds) X(dc_reads_seeds) X(dc_reads_chains) X(dc_reads_device) X(dc_seed_bytes) \
    /* host to device: timing slots 5, 6, 7 (include/rawdtw.h: rawdtw_mapper_timing) */ \
    X(anchor_bytes) X(event_bytes) X(other_bytes)
struct Counters {
#define X(name) uint64_t name = 0;
    RAWDTW_MAPPER_COUNTERS(X)
#undef X
    Counters &operator+=(const Counters &o)
    {
#define X(name) name += o.name;
        RAWDTW_MAPPER_COUNTERS(X)
#undef X
        return *this;
    }
};

} // namespace rawdtw_map

struct rawdtw_mapper {
    rawdtw_ctx *ctx = nullptr;
    rawdtw_mapper_opt_t opt{};
    std::vector<std::string> seq_names;
    std::vector<uint32_t> seq_len;
    std::vector<uint64_t> ref_off; // [seq * 2 + strand]: the strand array's offset in the reference arena (a scorer-only mapper: its index)
    std::vector<rawdtw_map::MRead> reads;
    std::vector<uint32_t> free_slots;
    uint32_t slots_used = 0;
    rawdtw_map::Group groups_store[2];
    struct GroupSpan { rawdtw_map::Group *b; size_t n; rawdtw_map::Group *begin() const { return b; } rawdtw_map::Group *end() const { return b + n; }
                       size_t size() const { return n; } rawdtw_map::Group &operator[](size_t i) const { return b[i]; } } groups{groups_store, 1};
    rawdtw_map::Pool *pool = nullptr;
    std::string log;
    rawdtw_map::Counters cnt;   // (committed rounds only, but for the byte counters: a failed round's traffic happened)
    double timing[5] = {0, 0, 0, 0, 0}; // the five times of rawdtw_mapper_timing; its slots 5-7 are cnt's byte counters
    rawdtw_scorer_fn scorer = nullptr;
    void *scorer_user = nullptr;
    bool keep_host_events = true; // (false: scored on the device only and no CIGAR asked for -- nothing reads the host's copy of a read's events)
    std::string err;
    rawdtw_su *su = nullptr;      // sequence-until (flag 0x1 or rawdtw_mapper_set_sequence_until): the state su_batch feeds
    bool su_closed_any = false;   // a batch has been closed (the parameters are fixed from then on)
    bool su_stopped = false;
    uint32_t su_mapped = 0;       // mapped reads of closed batches before the gate
    // The mapper's own buffers, beside the groups' round arrays.  With a context the device writes into those it is handed: seed_room.
    struct Own {
        rawdtw_map::PinBuf<uint64_t> seed_off;           // rawdtw_mapper_round_seeded and the resident rounds: the round's hit offsets, and
        rawdtw_map::PinBuf<rawdtw_seed_hit_t> seed_hits; // its hits (a resident round's only when it falls back)
        rawdtw_map::PinBuf<uint64_t> sig_dst;            // a round from signal: the round's tables, the counts that come home
        rawdtw_map::PinBuf<uint32_t> sig_room, sig_evlen;
        rawdtw_map::PinBuf<uint64_t> decl_soff;          // "chain_decline_reads": the declined reads' seeds from the device
        rawdtw_map::PinBuf<rawdtw_seed_t> decl_seeds;    // (rawdtw_chain_round_declined_seeds)
        void release() { seed_off.release(); seed_hits.release(); sig_dst.release(); sig_room.release(); sig_evlen.release(); decl_soff.release(); decl_seeds.release(); }
    } own;
    std::vector<uint64_t> sig_evoff;
    uint32_t kp_reserved = 0;       // "resident_chains": the store's N as this mapper reserved it
    bool kp_any = false;            // some read may hold kept chains
    uint64_t sig_cap = 0; // the largest events_cap a round from signal ran with: what the seeding's workspace holds already
    bool arena_replaced = false;    // rawdtw_mapper_finish has uploaded the host's copies over the event arena: no slot holds its read's events any more
    bool finish_from_arena = false; // "signal_cigar": a --dtw-output-cigar mapper has committed a round from signal -- the host's copy of a read's
                                    // events is incomplete from then on, and rawdtw_mapper_finish reads every read's events in its slot of the arena
    bool device_text = false;       // rawdtw_mapper_set_device_text: the full-matrix finish gets aln:s: as text from the device (include/rawdtw.h, "aln text")
    bool banded_cigar = false;     // rawdtw_mapper_set_banded_cigar: a global + banded --dtw-output-cigar mapper finishes through the banded traceback
};

namespace rawdtw_map {

inline int fail(rawdtw_mapper *m, int st, const std::string &msg)
{
    if (m) m->err = msg;
    return st;
}

inline double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline rawdtw_select_opt_t select_opt(const rawdtw_mapper *m)
{
    return rawdtw_select_opt_t{(m->opt.flag & 0x2) ? 1 : 0, m->opt.min_bestmap_ratio, m->opt.min_meanmap_ratio, m->opt.min_chain_anchor};
}

inline rawdtw_chain_t record_of(const MChain &c, uint32_t tag)
{
    return rawdtw_chain_t{c.chaining_score, c.alignment_score, c.ref, c.start_position, c.end_position, (uint32_t)c.anchors.size(), c.strand, 0u, tag};
}

// gen_primary_chains + comp_mapq over `post` (rmap.cpp:532-536): the primary chains, best first
inline std::vector<MChain> primary_chains(const rawdtw_mapper *m, std::vector<MChain> &post)
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

inline bool high_confidence(const rawdtw_mapper *m, const std::vector<MChain> &primary)
{
    if (primary.empty()) return false;
    static thread_local std::vector<rawdtw_chain_t> rec;
    rec.resize(primary.size());
    for (size_t k = 0; k < primary.size(); k++) rec[k] = record_of(primary[k], (uint32_t)k);
    const rawdtw_select_opt_t so = select_opt(m);
    return rawdtw_is_mapped_with_high_confidence(rec.data(), (uint32_t)rec.size(), &so) != 0;
}

// the --dtw-log-scores line of a scored chain (rmap.cpp:308-312)
inline std::string log_scores_line(float chaining_score, float alignment_score)
{
    char line[128];
    snprintf(line, sizeof line, "chaining_score=%f alignment_score=%f\n", (double)chaining_score, (double)alignment_score);
    return line;
}

// a context's option as the mapper reads it, through the public ABI: 0 for no context or a refusal
inline int64_t ctx_option(const rawdtw_ctx *ctx, const char *name)
{
    int64_t v = 0;
    return ctx && rawdtw_get_option(ctx, name, &v) == RAWDTW_OK ? v : 0;
}

// a read's slot in its group's event arena: the group's context and the slot's first float -- the one place a read's arena base is computed
inline rawdtw_ctx *slot_of(const rawdtw_mapper *m, const MRead &rd, uint32_t *base)
{
    const uint32_t G = (uint32_t)m->groups.size();
    *base = (G == 2 ? rd.slot / 2 : rd.slot) * m->opt.slot_events;
    return m->groups[rd.slot % G].ctx;
}

// room for `count` records in one of the mapper's own buffers (contents are not kept).  With a context the device writes into them:
// page-locked, or no room -- PinBuf's fall-back to plain memory does not reach them.
template <typename T> bool seed_room(const rawdtw_mapper *m, PinBuf<T> &b, uint64_t count)
{
    return b.ensure(count, m->ctx != nullptr) && (b.pinned || !m->ctx);
}

inline void drop_batches(rawdtw_mapper *m) // (and with them what a round could carry from)
{
    for (Group &g : m->groups) {
        for (RoundArrays &ra : g.buf) {
            if (ra.batch) rawdtw_batch_destroy(ra.batch);
            ra.batch = nullptr;
        }
        g.has_prev = false;
    }
}

} // namespace rawdtw_map
