// rawdtw_mapper_round.cpp -- one chunk round of the mapper (include/rawdtw.h, rawdtw_mapper_round*): the host phase, the round itself
// (struct Round: phases over one state, one commit point) and the five entry points.  The mapper's state and what surrounds the rounds
// (create, destroy, the reads, the stats, the finish, the PAF line) are rawdtw_mapper_state.h and rawdtw_mapper.cpp.
//
// What it restates: the control flow of map_worker_for / ri_map_frag / gen_chains (src/rmap.cpp:667-822, 545-578, 315-541)
// turned inside out so that every chunk round makes ONE device submission per read group (option A).
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
// Event detection and seeding stay in RawAlign (revent.c, rsketch.c, rawindex.cpp) unless a seeded entry is called: the caller hands in
// each chunk's events and seed hits.  Pure host code above the C ABI: no kernel is launched from here directly.
#include <tuple>

#include "rawdtw_mapper_state.h"

using namespace rawdtw_map;

namespace {

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

// a chain as the device chaining records it, and back (the anchors lie beside the record on either side)
rawdtw_chain_rec_t rec_of(const MChain &ch)
{
    return rawdtw_chain_rec_t{ch.chaining_score, ch.ref * 2u + (uint32_t)ch.strand, ch.start_position, ch.end_position, (uint32_t)ch.anchors.size()};
}

void chain_of(const rawdtw_chain_rec_t &rec, const rawdtw_anchor_t *an, MChain &ch)
{
    ch.chaining_score = rec.chaining_score; ch.ref = rec.key >> 1; ch.strand = (int32_t)(rec.key & 1u);
    ch.start_position = rec.start_position; ch.end_position = rec.end_position;
    ch.anchors.assign(an, an + rec.n_anchors);
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

// a chaining round begun on the device and not to be used: ended, its results dropped
void discard_chain_round(rawdtw_ctx *ctx)
{
    const rawdtw_anchor_t *a = nullptr; const uint64_t *rb = nullptr; const uint32_t *qb = nullptr;
    (void)rawdtw_chain_round_end(ctx, &a, &rb, &qb);
}

// a round's sizes in one group (0 where its path does not know them)
struct Sizes { uint64_t reads = 0, chains = 0, anchors = 0, new_anchors = 0, events = 0, seg = 0, seeds = 0; };

// ---- the bytes a round hands to the device beside its anchor lists and events (rawdtw_mapper_timing's slot 7), array by array: entries
// times bytes an entry, over the RoundArrays members that go up.  nr reads, nc chains, nseg event segments (seg_src 8 + seg_dst 4 each). ----
// chains made on the host (lay_out_and_submit): chain_off, anchor_off, ref_base and read_base a chain; with carry the records and new_off
uint64_t host_chained_bytes(uint64_t nr, uint64_t nc, uint64_t nseg, bool carried)
{
    return (nr + 1) * 8 + (nc + 1) * 8 + nc * (8 + 4) + (carried ? nc * sizeof(rawdtw_carry_t) + (nc + 1) * 8 : 0) + nseg * (8 + 4);
}
// chains made on the device (end_device_chain): the seed list (ns seeds), seed_off and chain_off, read_base a read, anchor_off
uint64_t device_chained_bytes(uint64_t nr, uint64_t nc, uint64_t ns, uint64_t nseg)
{
    return ns * sizeof(rawdtw_seed_t) + (nr + 1) * (8 + 8) + nr * 4 + (nc + 1) * 8 + nseg * (8 + 4);
}
// a resident round's own arrays beside those: prev_off; chunk_start and sits_out a read; the seeding's hit offsets; ev_start
uint64_t resident_bytes(uint64_t nr) { return (nr + 1) * 8 + nr * (4 + 1) + (nr + 1) * 8 + nr * 8; }
// "chain_decline_reads", what rawdtw_chain_round_append takes: the nd declined reads' chain offsets; a chain its record, anchor offset,
// reference base and read base (8 + 8 + 4); the chains' anchors
uint64_t declined_bytes(uint64_t nd, uint64_t chains, uint64_t anchors)
{
    return (nd + 1) * 8 + chains * (sizeof(rawdtw_chain_rec_t) + 8 + 8 + 4) + anchors * sizeof(rawdtw_anchor_t);
}
static_assert(sizeof(rawdtw_carry_t) == 24 && sizeof(rawdtw_seed_t) == 12 && sizeof(rawdtw_chain_rec_t) == 20 && sizeof(rawdtw_anchor_t) == 8, "the byte counters' terms");

// where a round's hits and events are when it begins
enum class RoundMode {
    HitsFromCaller, // rawdtw_mapper_round: events and hits in the caller's arrays
    HitsResident,   // rawdtw_mapper_round_seeded_resident: events in the caller's array, the hits on the device (hit_off / hits are absent)
    FromSignal,     // rawdtw_mapper_round_signal_resident / _raw_resident: events and hits on the device (event_off holds the counts the
                    // detection sent home; events, hit_off and hits are absent)
};
struct RoundInput { uint32_t n_reads; const uint32_t *read_ids; const uint64_t *event_off; const float *events; const uint64_t *hit_off; const rawdtw_seed_hit_t *hits; };

// One round after its checks.  The phases write only into the round's own state (rr, the groups' buffers of the round at hand, per,
// cnt); commit() is the one place the result reaches the reads and the mapper, and rollback() drops it.  The exception is the host's
// copy of a read's events, which the external scorer reads during the round: appended early, cut back by the rollback.
struct Round {
    // ---- fixed when the round is built: the constructor is the one place that computes them, and nothing writes them later ----
    rawdtw_mapper *const m;
    const RoundMode mode;
    const uint32_t n_reads;
    const uint32_t *const read_ids; const uint64_t *const event_off; const float *const events;
    const bool resident, signal; // the hits are on the device; the events are too (the device detected them in the arena)
    const uint32_t G;            // (1 or 2)
    const uint64_t id;
    const bool runs_dtw;         // rmap.cpp:509
    const bool on_device;        // the round's arrays are the device path's, page-locked.  A resident round's always: seeding and chaining run
                                 // on the device whether or not a DTW follows them
    // the caller's event array goes to the device as it is when it is page-locked (rawdtw_host_alloc) and one read group takes the whole round:
    // its reads' chunks ARE the segments, in order -- no copy into the mapper's own staging (a third of the host phase)
    const bool events_in_place;
    const bool device_round_end;     // the mapper's own context's options, read once a round
    const uint32_t resident_chains;
    struct GroupOpt { bool decline_reads = false; uint32_t max_chains = 0; }; // the group's context's "chain_decline_reads" and "chain_max_chains"
    // ---- what the phases set during the round ----
    const uint64_t *hit_off; const rawdtw_seed_hit_t *hits; // (a resident round: set only by its fall-back, which fetches them)
    bool fell_back = false;      // a resident round chained on the host after all
    double t0;                   // (the last lap)
    std::vector<RoundRead> rr;
    struct PerGroup { GroupOpt opt; // (read when the round is built)
                      bool chaining = false; uint64_t ns = 0, nev = 0, nseg = 0, extra = 0; // (a chaining begun on the device; seeds, events and segments sent up; other bytes)
                      bool round_end = false, keep = false; // (the round's end enqueued on the device, and the keep launch behind it)
                      uint64_t declined = 0;                // ("chain_decline_reads": the reads declined alone)
                      Counters cnt;                         // the group's share of the round's counters
    } per[2];
    Counters cnt;                // the round's counters: the mapper's at the commit
    int status = RAWDTW_OK;
    std::string msg;

    static bool caller_events_in_place(const rawdtw_mapper *m, RoundMode mode, bool on_device, const RoundInput &in)
    {
        if (mode == RoundMode::FromSignal) return false; // (there is no event array)
        if (mode == RoundMode::HitsFromCaller && !(on_device && m->opt.device_chain && m->groups.size() == 1)) return false;
        return in.event_off[in.n_reads] > 0 && rawdtw_host_is_page_locked(in.events) == 1;
    }
    Round(rawdtw_mapper *m_, RoundMode mode_, const RoundInput &in, double t0_)
        : m(m_), mode(mode_), n_reads(in.n_reads), read_ids(in.read_ids), event_off(in.event_off), events(mode_ == RoundMode::FromSignal ? nullptr : in.events),
          resident(mode_ != RoundMode::HitsFromCaller), signal(mode_ == RoundMode::FromSignal), G((uint32_t)m_->groups.size()), id(m_->cnt.rounds + 1),
          runs_dtw((m_->opt.flag & (0x2 | 0x8)) != 0), on_device(resident || (runs_dtw && !m_->scorer)), events_in_place(caller_events_in_place(m_, mode_, on_device, in)),
          device_round_end(ctx_option(m_->ctx, "device_round_end") != 0), resident_chains((uint32_t)ctx_option(m_->ctx, "resident_chains")),
          hit_off(resident ? nullptr : in.hit_off), hits(resident ? nullptr : in.hits), t0(t0_), rr(in.n_reads)
    {
        for (uint32_t gi = 0; gi < 2; gi++) {
            const rawdtw_ctx *ctx = gi < G ? m->groups[gi].ctx : nullptr;
            per[gi].opt = GroupOpt{ctx_option(ctx, "chain_decline_reads") != 0, (uint32_t)ctx_option(ctx, "chain_max_chains")};
        }
    }

    const GroupOpt &opt_of(const Group &g) const { return per[&g - m->groups.begin()].opt; }
    // the round takes previous seeds from the store of kept chains and keeps its own there: a resident round with the option on whose end
    // is enqueued on the device
    bool use_store() const { return resident && resident_chains != 0 && device_round_end && runs_dtw; }
    MRead &read(uint32_t k) const { return m->reads[read_ids[k]]; }
    uint32_t arena_base(const MRead &rd) const { uint32_t base; (void)slot_of(m, rd, &base); return base; } // its slot in its group's event arena
    bool ok() const { return status == RAWDTW_OK; }
    void failed(int st, const std::string &s) { if (ok()) { status = st; msg = s; } }
    void lap(int slot) { const double t = now_ms(); m->timing[slot] += t - t0; t0 = t; } // (include/rawdtw.h: rawdtw_mapper_timing)

    // the round's reads over the groups, into each group's other buffer, and the buffer's record started over
    void deal()
    {
        for (Group &g : m->groups) { g.cur ^= 1; g.buf[g.cur].ks.clear(); }
        for (uint32_t k = 0; k < n_reads; k++) { Group &g = m->groups[read(k).slot % G]; g.buf[g.cur].ks.push_back(k); }
        for (Group &g : m->groups) { RoundArrays &ra = g.buf[g.cur]; ra.carried = false; ra.round_id = id; ra.n_reads = ra.ks.size(); }
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

    // ---- the round's host arrays: the one place a RoundArrays buffer is sized ----
    // Which path of a round needs which buffer, how many entries (by the group's high-water marks), in what memory, and how many leading
    // entries survive a move.  Both of the group's buffers grow together.  `mid`: what a round meets in its middle -- a batch with declined
    // reads' pseudo-reads and chains behind the device's, a round end -- is grown in the buffer at hand alone, to the batch's own reads and
    // chains where they are above the marks: a round nobody is declined in allocates nothing for declines.
    enum : unsigned { HOST_CHAINED = 1, DEVICE_CHAINED = 2, RESIDENT = 4, STORE = 8, ROUND_END = 16, DECLINED = 32 };
    struct BatchSize { uint64_t reads = 0, chains = 0; };
    bool grow(Group &g, unsigned paths, const BatchSize *mid = nullptr)
    {
        const bool host = paths & HOST_CHAINED, dev = paths & DEVICE_CHAINED, chained = host || dev, res = paths & RESIDENT, store = paths & STORE;
        const bool round_end = paths & ROUND_END, declined = paths & DECLINED;
        // page-locked unless an external scorer takes the round; carry records for host chains that may take costs over; the events' staging
        const bool pin = on_device, carry = host && on_device && m->opt.carry, staged = chained && on_device;
        const uint64_t nr = g.hw_reads + 1, nc = g.hw_chains + 1;
        const uint64_t batch_r = std::max(g.hw_reads, mid ? mid->reads : 0) + 1, batch_c = std::max(g.hw_chains, mid ? mid->chains : 0) + 1;
        for (int b = 0; b < (mid ? 1 : 2); b++) {
            RoundArrays &x = g.buf[g.cur ^ b];
            // the round before's first n_reads + 1 / n_chains + 1 / n_anchors + 1 entries survive (the host chaining's matching reads them)
            const bool kept = b == 1 && host;
            const size_t k_r = kept ? x.n_reads + 1 : 0, k_c = kept ? x.n_chains + 1 : 0, k_a = kept ? x.n_anchors + 1 : 0;
            bool ok = true;
            auto row = [&ok](auto &buf, bool needed, uint64_t entries, bool pinned, size_t survive = 0) {
                if (ok && needed) ok = buf.ensure(entries, pinned, survive);
            };
            //  buffer            needed by             entries                                      memory  survive
            row(x.chain_off,      chained,              nr,                                          pin,    k_r);
            row(x.anchor_off,     chained,              nc,                                          pin,    k_c);
            row(x.read_base,      chained,              nc,                                          pin,    k_c);
            row(x.anchors,        chained,              (dev ? g.hw_seeds : g.hw_anchors) + 1,       pin && !(m->opt.carry && g.has_prev), k_a);
            row(x.score,          chained || declined,  batch_c,                                     pin);
            row(x.keep,           chained || declined,  batch_c,                                     pin);
            row(x.seed_off,       dev,                  nr,                                          pin);
            row(x.seeds,          dev,                  g.hw_seeds + 1,                              pin);
            row(x.recs,           dev,                  nc,                                          pin);
            row(x.ref_base,       host,                 nc,                                          pin,    k_c);
            row(x.new_off,        carry,                nc,                                          pin);
            row(x.new_anchors,    carry,                g.hw_new + 1,                                pin);
            row(x.carry,          carry,                nc,                                          pin);
            row(x.new_events,     staged,               (events_in_place ? 0 : g.hw_events) + 1,     pin);
            row(x.seg_src,        staged,               g.hw_seg + 2,                                pin);
            row(x.seg_dst,        staged,               (dev ? g.hw_reads : g.hw_seg) + 1,           pin);
            row(x.prev_off,       res,                  nr,                                          true);
            row(x.ev_start,       res,                  nr,                                          true);
            row(x.ev_len,         res,                  nr,                                          true);
            row(x.chunk_start,    res,                  nr,                                          true);
            row(x.sits_out,       res,                  nr,                                          true);
            row(x.prev_src,       store,                nr,                                          true);
            row(x.keep_dst,       store,                batch_r,                                     false,  mid ? x.n_reads : 0); // (the reads' entries are written when reads are declined)
            row(x.kept_count,     store,                batch_r,                                     false);
            row(x.re_out,         round_end,            batch_r,                                     false);
            row(x.re_primary,     round_end,            batch_c,                                     false);
            row(x.chain_off_ext,  declined,             (mid ? mid->reads : 0) + 1,                  pin);
            row(x.anchor_off_ext, declined,             (mid ? mid->chains : 0) + 1,                 pin);
            if (!ok) { failed(RAWDTW_ERR_OOM, "host allocation failed"); return false; }
        }
        return true;
    }

    // The group's high-water marks raised to a round's sizes, and its arrays grown to them as the chaining's side needs them: on the device
    // (seed lists in, chains out) or on the host (anchor lists, carry records); either way the events' staging.
    bool size_arrays(Group &g, const Sizes &n, bool dev)
    {
        g.hw_reads = std::max(g.hw_reads, n.reads); g.hw_chains = std::max(g.hw_chains, n.chains); g.hw_anchors = std::max(g.hw_anchors, n.anchors);
        g.hw_new = std::max(g.hw_new, n.new_anchors); g.hw_events = std::max(g.hw_events, n.events); g.hw_seg = std::max(g.hw_seg, n.seg);
        g.hw_seeds = std::max(g.hw_seeds, n.seeds);
        if (dev) { // the device's cap on chains a read: 32, or "chain_max_chains" -- then no more than the seeds can make, min_num_anchors a chain
            const uint32_t many = opt_of(g).max_chains;
            const uint64_t by_seeds = g.hw_seeds / (uint64_t)std::max(1, m->opt.chain.min_num_anchors) + 1;
            g.hw_chains = std::max<uint64_t>(g.hw_chains, many > 0 ? std::min<uint64_t>(g.hw_reads * (uint64_t)many, by_seeds) : g.hw_reads * 32);
        }
        return grow(g, dev ? DEVICE_CHAINED : HOST_CHAINED);
    }

    // ---- a group's first half: the host phase, lay-out and submission; with device chaining the chaining begun instead ----
    void begin_group(uint32_t gi)
    {
        Group &g = m->groups[gi]; RoundArrays &ra = g.buf[g.cur];
        const RoundArrays &pb = g.buf[g.cur ^ 1];
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

    // a chaining begun on the device: what the group sent up, for the byte counters of end_device_chain
    void chaining_begun(uint32_t gi, uint64_t ns, uint64_t nev, uint64_t nseg, uint64_t extra)
    {
        PerGroup &p = per[gi];
        p.chaining = true; p.ns = ns; p.nev = nev; p.nseg = nseg; p.extra = extra;
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
        chaining_begun(gi, n.seeds, n.events, n.seg, 0);
        return true;
    }

    // ---- a resident round's first half (one group): the events go up first, the seeding reads them in the arena and sends the hit counts
    // home -- the one wait --, the arrays are sized by them, and the chaining is begun on seeds the device lays down itself: only the previous
    // chains' anchors go up.  A round the chaining declines fetches the hits and is chained on the host, as device_begin's is.
    void resident_begin(uint32_t gi)
    {
        Group &g = m->groups[gi]; RoundArrays &ra = g.buf[g.cur];
        const size_t nr = ra.ks.size();
        m->pool->run(nr, 64, [&](size_t i) { append_events(ra.ks[i]); });
        Sizes n{nr};
        if (!stage_events(g, n, true, events_in_place)) return;
        const uint64_t nev = n.events, nseg = n.seg;
        if (!grow(g, RESIDENT)) return;
        m->pool->run(nr, 64, [&](size_t i) {
            const uint32_t k = ra.ks[i];
            const RoundRead &r = rr[k];
            ra.ev_start[i] = (uint64_t)arena_base(read(k)) + r.ev_before;
            ra.ev_len[i] = (uint32_t)r.ne;
            if (!events_in_place) stage_chunk(ra, k);
        });
        lap(0);
        int st = upload_events(g, n, events_in_place);
        if (st == RAWDTW_OK) st = rawdtw_seed_resident_begin(g.ctx, (uint32_t)nr, ra.ev_start.p, ra.ev_len.p, m->own.seed_off.p);
        if (st == RAWDTW_OK) st = rawdtw_seed_resident_end(g.ctx, nullptr);
        lap(2);
        if (st != RAWDTW_OK) return failed(st, rawdtw_last_error(g.ctx));
        resident_chain(gi, nev, nseg);
    }

    // ---- a round from signal, first half: detection and seeding ran on the device before the round was set up (rawdtw_mapper_round_signal_*),
    // the events are in the arena and their counts in event_off; what is left of the host phase is the bookkeeping of append_events ----
    void signal_begin(uint32_t gi)
    {
        Group &g = m->groups[gi]; RoundArrays &ra = g.buf[g.cur];
        const size_t nr = ra.ks.size();
        m->pool->run(nr, 64, [&](size_t i) { append_events(ra.ks[i]); });
        if (!size_arrays(g, Sizes{nr}, true) || !grow(g, RESIDENT)) return;
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
        const uint64_t *hoff = m->own.seed_off.p; // (chunk i is read ks[i]: one group, the round's reads in order)
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
            cnt.event_bytes += nev * sizeof(float);
            if (fetch_resident_hits(gi)) host_round(gi, nullptr, true);
            return;
        }
        if (st != RAWDTW_OK) return failed(st, rawdtw_last_error(g.ctx));
        cnt.res_seed_bytes = np * sizeof(rawdtw_seed_t); // (the previous anchors sent up as seeds)
        chaining_begun(gi, np, nev, nseg, resident_bytes(nr));
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
        return grow(g, STORE);
    }

    // the fall-back of a resident round: its hits to the host, once, where host_round reads them
    bool fetch_resident_hits(uint32_t gi)
    {
        const uint64_t tot = m->own.seed_off[n_reads];
        if (!seed_room(m, m->own.seed_hits, tot + 1)) { failed(RAWDTW_ERR_OOM, "no page-locked memory for the round's hits"); return false; }
        const int st = rawdtw_seed_resident_fetch(m->groups[gi].ctx, m->own.seed_hits.p, m->own.seed_hits.cap);
        if (st != RAWDTW_OK) { failed(st, rawdtw_last_error(m->groups[gi].ctx)); return false; }
        hit_off = m->own.seed_off.p; hits = m->own.seed_hits.p;
        fell_back = true; cnt.res_hit_bytes = tot * sizeof(rawdtw_seed_hit_t);
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
            if (resident) { cnt.event_bytes += p.nev * sizeof(float); if (!fetch_resident_hits(gi)) return; }
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
        cnt.event_bytes += p.nev * sizeof(float);
        cnt.other_bytes += device_chained_bytes(nr, nc, p.ns, p.nseg) + p.extra;
        lap(2);
        m->pool->run(nr, 32, [&](size_t i) {
            RoundRead &r = rr[ra.ks[i]];
            if (r.declined) return; // (its chains are the host's already, and chain0 / bpos its pseudo-read's)
            r.bpos = i;
            r.chain0 = ra.chain_off[i];
            r.chains.resize(ra.chain_off[i + 1] - ra.chain_off[i]);
            for (uint64_t c = 0; c < r.chains.size(); c++) chain_of(ra.recs[r.chain0 + c], ra.anchors.p + ra.anchor_off[r.chain0 + c], r.chains[c]);
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
        if (nd == 0) return true; // (and nothing is counted: the decline counters are of rounds that declined reads)
        const uint64_t *soff = ra.seed_off.p; // (a declined read's seeds: [soff[x], soff[x + 1]) of `seeds`, x its position in the group or in the list)
        const rawdtw_seed_t *seeds = ra.seeds.p;
        if (resident) {
            rawdtw_mapper::Own &own = m->own;
            if (!seed_room(m, own.decl_soff, nd + 1)) { failed(RAWDTW_ERR_OOM, "no page-locked memory for the declined reads' seeds"); return false; }
            st = rawdtw_chain_round_declined_seeds(g.ctx, own.decl_soff.p, own.decl_seeds.p, own.decl_seeds.p ? own.decl_seeds.cap : 0);
            if (st == RAWDTW_ERR_RANGE) { // (the offsets are filled: room for what they say, then again)
                if (!seed_room(m, own.decl_seeds, own.decl_soff[nd] + 1)) { failed(RAWDTW_ERR_OOM, "no page-locked memory for the declined reads' seeds"); return false; }
                st = rawdtw_chain_round_declined_seeds(g.ctx, own.decl_soff.p, own.decl_seeds.p, own.decl_seeds.cap);
            }
            if (st != RAWDTW_OK) { failed(st, rawdtw_last_error(g.ctx)); return false; }
            soff = own.decl_soff.p; seeds = own.decl_seeds.p;
            p.cnt.dc_seed_bytes += own.decl_soff[nd] * sizeof(rawdtw_seed_t);
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
            p.declined++; p.cnt.dc_reads_seeds += dwhy[j] & 1u; p.cnt.dc_reads_chains += (dwhy[j] & 6u) ? 1 : 0;
        }
        for (size_t i = 0; i < nr; i++) p.cnt.dc_reads_device += rr[ra.ks[i]].skipped ? 0 : 1; // (the reads that took part ...
        p.cnt.dc_reads_device -= nd;                                                             // ... and were not declined)
        std::vector<rawdtw_chain_rec_t> recs(coff[nd] + 1);
        std::vector<rawdtw_anchor_t> anchors;
        for (uint64_t j = 0; j < nd; j++) {
            const RoundRead &r = rr[ra.ks[dreads[j]]];
            for (size_t c = 0; c < r.chains.size(); c++) {
                recs[coff[j] + c] = rec_of(r.chains[c]);
                anchors.insert(anchors.end(), r.chains[c].anchors.begin(), r.chains[c].anchors.end());
                aoff.push_back(anchors.size());
            }
        }
        anchors.push_back(rawdtw_anchor_t{0, 0}); // (never a null array)
        // room, on demand: the batch's two offset arrays, its per-chain results, and with the store its per-read destinations (whose first
        // nr entries are written already)
        const BatchSize batch{nr + nd, ra.chain_off[nr] + coff[nd]};
        if (!grow(g, DECLINED | (use_store() ? STORE : 0u), &batch)) return false;
        st = rawdtw_chain_round_append(g.ctx, nd, coff.data(), recs.data(), aoff.data(), anchors.data(), ra.chain_off_ext.p, ra.anchor_off_ext.p, d_anchors, d_ref_base,
                                       d_read_base);
        if (st != RAWDTW_OK) { failed(st, rawdtw_last_error(g.ctx)); return false; }
        for (uint64_t j = 0; j < nd; j++) {
            rr[ra.ks[dreads[j]]].chain0 = ra.chain_off_ext[nr + j];
            if (use_store()) { ra.keep_dst[dreads[j]] = RAWDTW_NO_KEEP; ra.keep_dst[nr + j] = RAWDTW_NO_KEEP; }
        }
        p.extra += declined_bytes(nd, coff[nd], anchors.size() - 1);
        return true;
    }

    // "device_round_end": the round's end enqueued right behind the batch, on the chaining workspace's records where they lie
    int begin_round_end(Group &g, RoundArrays &ra, PerGroup &p)
    {
        // (a round that declined reads alone has a pseudo-read for each of them, and their chains behind the device's: ra.n_reads_batch / n_chains)
        const BatchSize batch{ra.n_reads_batch, ra.n_chains};
        if (!grow(g, ROUND_END, &batch)) return RAWDTW_ERR_OOM;
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
            cnt.anchor_bytes += (ra.carried ? n.new_anchors : na) * sizeof(rawdtw_anchor_t);
            cnt.event_bytes += n.events * sizeof(float);
            cnt.other_bytes += host_chained_bytes(nr, nc, n.seg, ra.carried);
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
        PerGroup &p = per[gi];
        if (on_device && ra.batch) {
            const int st = rawdtw_batch_fetch(g.ctx, ra.batch, ra.score.p, ra.keep.p, nullptr); // (also after a failure elsewhere: the arrays it reads go out of use here)
            if (st != RAWDTW_OK) failed(st, rawdtw_last_error(g.ctx));
            uint64_t sc = 0, ru = 0;
            if (ok() && rawdtw_batch_round_stats(g.ctx, ra.batch, &sc, &ru) == RAWDTW_OK) { p.cnt.parts_scored = sc; p.cnt.parts_reused = ru; }
            if (p.round_end) { // (also after a failure: the context's round end is begun and must be ended)
                const int se = rawdtw_batch_round_end_fetch(g.ctx, ra.batch, ra.re_out.p, ra.re_primary.p);
                if (se != RAWDTW_OK) failed(se, rawdtw_last_error(g.ctx));
                if (se == RAWDTW_OK && p.keep) { // (a keep whose round end failed goes with the batch)
                    const int sk = rawdtw_batch_round_keep_fetch(g.ctx, ra.batch, ra.kept_count.p);
                    if (sk != RAWDTW_OK) failed(sk, rawdtw_last_error(g.ctx));
                }
            }
        }
        lap(3);
        if (!ok()) return;
        const bool evaluate = (m->opt.flag & 0x2) != 0, log_scores = (m->opt.flag & 0x8) != 0;
        const bool from_device = p.round_end;
        m->pool->run(ra.ks.size(), 16, [&](size_t i) {
            const uint32_t k = ra.ks[i];
            RoundRead &r = rr[k];
            if (r.skipped) { r.high = high_confidence(m, read(k).chains); return; } // rmap.cpp:569-572: the chains stay as they were
            if (from_device && !(ra.re_out[r.bpos].flags & RAWDTW_ROUND_DECLINED)) { // primary, mapq and the stop rule's answer are the device's: the chains are moved
                const rawdtw_round_out_t &o = ra.re_out[r.bpos]; // (its read in the batch: a read the chaining declined alone has a pseudo-read)
                if (log_scores)
                    for (size_t c = 0; c < r.chains.size(); c++) {
                        const float as = ra.score[r.chain0 + c];
                        if (as != -1e10f) r.log += log_scores_line(r.chains[c].chaining_score, as);
                    }
                r.primary.reserve(o.n_primary);
                for (uint32_t q = 0; q < o.n_primary; q++) {
                    const uint32_t c = ra.re_primary[r.chain0 + q];
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
                    if (log_scores && ch.alignment_score != -1e10f) r.log += log_scores_line(ch.chaining_score, ch.alignment_score);
                }
                if (!evaluate || !runs_dtw || keep) post.push_back(std::move(ch)); // rmap.cpp:525: replaced only under EVALUATE_CHAINS
            }
            r.primary = primary_chains(m, post);
            r.high = high_confidence(m, r.primary);
        });
        if (from_device) // (counted here, not by the pool's threads: sixteen of them adding to one counter cost the round more than its end)
            for (size_t i = 0; i < ra.ks.size(); i++) {
                if (rr[ra.ks[i]].skipped) continue;
                if (ra.re_out[rr[ra.ks[i]].bpos].flags & RAWDTW_ROUND_DECLINED) p.cnt.re_declined++; else p.cnt.re_reads++;
            }
        lap(4);
    }

    // ---- a failed round: the reads' events cut back, each group's round before stays the round before; nothing else was written ----
    // (A round from signal: the device has written the chunk's events into the arena above the read's committed n_events.  That stretch is
    // scratch -- nothing reads a slot beyond n_events -- and the next attempt's detection overwrites it from the same place.)
    // Of the round's counters only the bytes it handed to the device stay: that traffic happened, as the time did (rawdtw_mapper_timing).
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
        Counters sent;
        sent.anchor_bytes = cnt.anchor_bytes; sent.event_bytes = cnt.event_bytes; sent.other_bytes = cnt.other_bytes;
        m->cnt += sent;
        return fail(m, status, msg);
    }

    // ---- commit ----
    void commit()
    {
        cnt.rounds = 1;
        cnt.re_rounds = per[0].round_end || per[1].round_end;
        cnt.dc_rounds = per[0].declined || per[1].declined;
        if (resident) (fell_back ? cnt.res_fallbacks : cnt.res_rounds) = 1;
        for (uint32_t gi = 0; gi < G; gi++) {
            Group &g = m->groups[gi];
            RoundArrays &ra = g.buf[g.cur], &pb = g.buf[g.cur ^ 1];
            if (pb.batch) { rawdtw_batch_destroy(pb.batch); pb.batch = nullptr; }
            g.has_prev = on_device && m->opt.carry && !m->opt.device_chain && ra.batch != nullptr;
            if (!g.has_prev && ra.batch) { rawdtw_batch_destroy(ra.batch); ra.batch = nullptr; }
            cnt += per[gi].cnt;
            for (size_t i = 0; i < ra.ks.size(); i++) { read(ra.ks[i]).last_round = id; read(ra.ks[i]).last_pos = i; }
            // "resident_chains": the one place a read's kept state changes.  A read that sat out keeps its chains and its state; a read whose
            // chains were kept is seeded from that half from now on; every other read's chains are new and not on the device
            // (a mapper that never had the option on has no read to clear: the loop is skipped)
            for (size_t i = 0; (use_store() || m->kp_any) && i < ra.ks.size(); i++) {
                MRead &rd = read(ra.ks[i]); const RoundRead &r = rr[ra.ks[i]];
                if (r.skipped) continue;
                if (use_store() && !fell_back && r.n_prev) { // (a round that fell back was chained on the host, from the host's chains)
                    if (r.from_store) { cnt.kp_reads_dev++; cnt.kp_seeds_dev += r.n_prev; } else { cnt.kp_reads_host++; cnt.kp_seeds_host += r.n_prev; }
                }
                if (per[gi].keep && ra.kept_count[i] != RAWDTW_NOT_KEPT) { rd.kept = MRead::Kept{true, (uint8_t)(ra.keep_dst[i] & 1u), ra.kept_count[i]}; m->kp_any = true; }
                else { rd.kept.valid = false; if (per[gi].keep) cnt.kp_not_kept++; }
            }
        }
        m->cnt += cnt;
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

    // The round itself: the reads dealt, every group's first half as the mode has it (with device chaining every group's is begun before the
    // first is ended), the chains home, each group's round end (group gi's while group gi + 1's batch is on the device), then the one commit
    // point.
    int run()
    {
        deal();
        for (uint32_t gi = 0; gi < G && ok(); gi++) {
            if (mode == RoundMode::HitsFromCaller) begin_group(gi);
            else if (mode == RoundMode::HitsResident) resident_begin(gi);
            else signal_begin(gi);
        }
        for (uint32_t gi = 0; gi < G; gi++) end_device_chain(gi);
        for (uint32_t gi = 0; gi < G; gi++) fetch_and_end(gi);
        if (!ok()) return rollback();
        commit();
        return RAWDTW_OK;
    }
};

// a round's reads, every one checked before anything changes (`hit_off` null: a resident round, whose hits the host never sees;
// `event_off` null: a round from signal, whose event counts the device finds -- it checks them against the slots' room itself)
int check_round(rawdtw_mapper *m, uint32_t n_reads, const uint32_t *read_ids, const uint64_t *event_off, const uint64_t *hit_off, const rawdtw_seed_hit_t *hits)
{
    const uint32_t n_seq = (uint32_t)m->seq_len.size();
    const uint64_t stamp = m->cnt.rounds + 1;
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

// ---- what the three seeded entries share in front of their rounds ----
// their arguments (`args_ok`; `null_msg`: the entry's words for a refusal, null for none), and an index that can be read (its parameters
// out) and holds the mapper's sequences
int seeded_checks(rawdtw_mapper *m, const rawdtw_seed_index *six, bool args_ok, const char *null_msg, rawdtw_seed_pars_t *pars)
{
    if (!args_ok) return null_msg ? fail(m, RAWDTW_ERR_INVALID, null_msg) : RAWDTW_ERR_INVALID;
    uint32_t six_seq = 0;
    if (rawdtw_seed_index_info(six, &six_seq, nullptr, nullptr, nullptr, pars) != RAWDTW_OK) return RAWDTW_ERR_INVALID;
    if (six_seq != m->seq_len.size()) return fail(m, RAWDTW_ERR_INVALID, "the seed index and the mapper hold different numbers of sequences");
    return RAWDTW_OK;
}

// The index on the mapper's context (every round: the context knows its table by the index's serial and does nothing when this index is
// there already -- also right after the caller uploaded another index to the context, or rebuilt one at the old address).  A resident
// round: the one thing the upload refuses there -- a seeding somebody began on the mapper's context and has not ended -- is unsupported.
int upload_index(rawdtw_mapper *m, const rawdtw_seed_index *six, bool resident_round)
{
    const int up = rawdtw_seed_index_upload(m->ctx, six);
    if (up == RAWDTW_OK) return up;
    return fail(m, up == RAWDTW_ERR_INVALID && resident_round ? RAWDTW_ERR_UNSUPPORTED : up, rawdtw_last_error(m->ctx));
}

// a resident round's preconditions (each entry refuses in its own words).  no_cigar: nothing may read the host's copy of a read's events
// later either, which the --dtw-output-cigar traceback (rawdtw_mapper_finish) would
bool resident_round_ok(const rawdtw_mapper *m, const rawdtw_seed_pars_t &pars, bool no_cigar)
{
    return m->ctx && !m->scorer && m->opt.device_chain && m->groups.size() == 1 && (pars.w == 0 || ctx_option(m->ctx, "seed_minimizer") != 0) &&
           !(no_cigar && (m->opt.flag & 0x4));
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
    return Round(m, RoundMode::HitsFromCaller, RoundInput{n_reads, read_ids, event_off, events, hit_off, hits}, t0).run();
}

// The seeding of gen_chains (rmap.cpp:364-391) in front of the round.  Everything the seeding touches is the mapper's own buffers:
// the reads change only inside rawdtw_mapper_round, which runs on the finished hits or not at all.
int rawdtw_mapper_round_seeded(rawdtw_mapper *m, const rawdtw_seed_index *six, uint32_t n_reads, const uint32_t *read_ids,
                               const uint64_t *event_off, const float *events)
{
    const bool args_ok = m && six && !(n_reads && (!read_ids || !event_off)) && !(n_reads && event_off[n_reads] > event_off[0] && !events);
    rawdtw_seed_pars_t pars;
    if (const int st = seeded_checks(m, six, args_ok, nullptr, &pars)) return st;
    if (n_reads == 0) return RAWDTW_OK;
    const bool on_device = m->ctx && (pars.w == 0 || ctx_option(m->ctx, "seed_minimizer") != 0); // (the minimizer sketch is the host's unless "seed_minimizer" is on)
    rawdtw_mapper::Own &own = m->own;
    if (!seed_room(m, own.seed_off, (uint64_t)n_reads + 1)) return fail(m, RAWDTW_ERR_OOM, "no memory for the round's hit offsets");
    if (!on_device) {
        if (rawdtw_seed_index_is_resident(six)) return fail(m, RAWDTW_ERR_UNSUPPORTED, "host seeding needs the index's host copy: rawdtw_seed_index_fetch first");
        int st = rawdtw_seed_hits_host(six, n_reads, event_off, events, own.seed_off.p, nullptr, 0, m->opt.threads); // (counts)
        if (st != RAWDTW_OK && st != RAWDTW_ERR_RANGE) return fail(m, st, "seeding: bad event offsets");
        if (!seed_room(m, own.seed_hits, own.seed_off[n_reads])) return fail(m, RAWDTW_ERR_OOM, "no memory for the round's hits");
        st = rawdtw_seed_hits_host(six, n_reads, event_off, events, own.seed_off.p, own.seed_hits.p, own.seed_hits.cap, m->opt.threads);
        if (st != RAWDTW_OK) return fail(m, st, "seeding failed");
    } else {
        if (const int up = upload_index(m, six, false)) return up;
        // the first guess: what the buffer holds, or four hits an event; a round with more says how many and is seeded once more
        uint64_t want = std::max<uint64_t>(own.seed_hits.cap, 4 * (event_off[n_reads] - event_off[0]) + 1024);
        for (int attempt = 0;; attempt++) {
            if (!seed_room(m, own.seed_hits, want)) return fail(m, RAWDTW_ERR_OOM, "no page-locked memory for the round's hits");
            int st = rawdtw_seed_begin(m->ctx, n_reads, event_off, events, own.seed_off.p, own.seed_hits.p, own.seed_hits.cap);
            if (st == RAWDTW_OK) st = rawdtw_seed_end(m->ctx, nullptr);
            if (st == RAWDTW_ERR_RANGE && attempt == 0 && own.seed_off[n_reads] > own.seed_hits.cap) { want = own.seed_off[n_reads]; continue; }
            if (st != RAWDTW_OK) return fail(m, st, rawdtw_last_error(m->ctx));
            break;
        }
    }
    return rawdtw_mapper_round(m, n_reads, read_ids, event_off, events, own.seed_off.p, own.seed_hits.p);
}

// rawdtw_mapper_round_seeded with the hits left on the device: the events are appended, the seeding reads them in the arena, and the
// chaining's seed list is written where the chaining reads it.  Everything it cannot do is refused before anything changes.
int rawdtw_mapper_round_seeded_resident(rawdtw_mapper *m, const rawdtw_seed_index *six, uint32_t n_reads, const uint32_t *read_ids,
                                        const uint64_t *event_off, const float *events)
{
    const bool args_ok = m && six && !(n_reads && (!read_ids || !event_off)) && !(n_reads && event_off[n_reads] > event_off[0] && !events);
    rawdtw_seed_pars_t pars;
    if (const int st = seeded_checks(m, six, args_ok, nullptr, &pars)) return st;
    if (!resident_round_ok(m, pars, false))
        return fail(m, RAWDTW_ERR_UNSUPPORTED, "a resident round needs a context, device chaining, one read group, no external scorer and a w == 0 index, "
                                               "or a w > 0 one with the context's \"seed_minimizer\" option on (rawdtw_mapper_round_seeded maps the round)");
    if (n_reads == 0) return RAWDTW_OK;
    const double t0 = now_ms();
    const int chk = check_round(m, n_reads, read_ids, event_off, nullptr, nullptr);
    if (chk != RAWDTW_OK) return chk;
    if (!seed_room(m, m->own.seed_off, (uint64_t)n_reads + 1)) return fail(m, RAWDTW_ERR_OOM, "no memory for the round's hit offsets");
    if (const int up = upload_index(m, six, true)) return up;
    return Round(m, RoundMode::HitsResident, RoundInput{n_reads, read_ids, event_off, events, nullptr, nullptr}, t0).run();
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
    const bool args_ok = m && six && !(n_reads && (!read_ids || !off)) && !(n_reads && off[n_reads] > off[0] && (is_raw ? !raw : !sig)) && !(n_reads && is_raw && !chan);
    rawdtw_seed_pars_t pars;
    if (const int st = seeded_checks(m, six, args_ok, "null argument", &pars)) return st;
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
    rawdtw_mapper::Own &own = m->own;
    if (!seed_room(m, own.seed_off, nr + 1) || !own.sig_dst.ensure(nr, false) || !own.sig_room.ensure(nr, false) || !own.sig_evlen.ensure(nr, false))
        return fail(m, RAWDTW_ERR_OOM, "no memory for the round's tables");
    for (uint32_t k = 0; k < n_reads; k++) { // the chunk goes behind the read's committed events, and may fill its slot
        const MRead &rd = m->reads[read_ids[k]];
        uint32_t base = 0;
        (void)slot_of(m, rd, &base);
        own.sig_dst[k] = (uint64_t)base + rd.n_events;
        own.sig_room[k] = m->opt.slot_events - std::min(rd.n_events, m->opt.slot_events);
    }
    if (const int up = upload_index(m, six, true)) return up; // (refused: somebody's seeding is begun on the context)
    // events_cap, the first guess: what the seeding's workspace holds already, or a quarter of the samples; a round with more says how many and
    // runs once more (as rawdtw_mapper_round_seeded does for its hits)
    const uint64_t n_samples = off[n_reads] - off[0];
    const int64_t first_cap = ctx_option(m->ctx, "signal_events_cap");
    uint64_t cap = first_cap > 0 ? (uint64_t)first_cap : std::max<uint64_t>(m->sig_cap, n_samples / 4 + 1024);
    uint64_t total = 0;
    bool retried = false;
    for (int attempt = 0;; attempt++) {
        int st = is_raw ? rawdtw_detect_raw_resident_begin(m->ctx, ev_opt, n_reads, off, raw, chan, own.sig_dst.p, own.sig_room.p, cap)
                        : rawdtw_detect_resident_begin(m->ctx, ev_opt, n_reads, off, sig, own.sig_dst.p, own.sig_room.p, cap);
        if (st != RAWDTW_OK) return fail(m, st, rawdtw_last_error(m->ctx));
        const int sb = rawdtw_seed_detected_begin(m->ctx, own.seed_off.p);
        // the one wait: both ends (the detection's first -- it is ended whatever the seeding's begin said)
        st = rawdtw_detect_resident_end(m->ctx, nullptr, own.sig_evlen.p, &total, nullptr);
        std::string msg = st != RAWDTW_OK ? rawdtw_last_error(m->ctx) : "";
        if (sb != RAWDTW_OK) return fail(m, sb, rawdtw_last_error(m->ctx));
        const int se = rawdtw_seed_resident_end(m->ctx, nullptr);
        if (st == RAWDTW_OK && se == RAWDTW_OK) break;
        if (st == RAWDTW_ERR_RANGE) {
            for (uint32_t k = 0; k < n_reads; k++)
                if (own.sig_evlen[k] > own.sig_room[k]) return fail(m, RAWDTW_ERR_RANGE, "a read outgrew its slot in the event arena");
            if (attempt == 0 && total > cap) { cap = total; retried = true; continue; }
        }
        return st != RAWDTW_OK ? fail(m, st, msg) : fail(m, se, rawdtw_last_error(m->ctx));
    }
    m->sig_cap = std::max(m->sig_cap, cap);
    m->sig_evoff.resize(nr + 1);
    m->sig_evoff[0] = 0;
    for (uint32_t k = 0; k < n_reads; k++) m->sig_evoff[k + 1] = m->sig_evoff[k] + own.sig_evlen[k];
    if (const int st = Round(m, RoundMode::FromSignal, RoundInput{n_reads, read_ids, m->sig_evoff.data(), nullptr, nullptr, nullptr}, t0).run()) return st;
    // (counted here, behind the commit: the samples went up before the round was set up)
    Counters sent;
    sent.sig_rounds = 1; sent.sig_retried = retried ? 1 : 0;
    sent.sig_sample_bytes = n_samples * (is_raw ? sizeof(int16_t) : sizeof(float)) * (retried ? 2 : 1);
    m->cnt += sent;
    if (m->opt.flag & 0x4) m->finish_from_arena = true; // (only with "signal_cigar" on does such a mapper get here)
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

} // extern "C"
