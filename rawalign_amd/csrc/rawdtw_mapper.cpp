// rawdtw_mapper.cpp -- the chunk-round mapper on the library's host side (include/rawdtw.h, rawdtw_mapper_*): what surrounds the rounds.
// The mapper created and destroyed, its reads, the stats, a read's events, --dtw-output-cigar at the end (rawdtw_mapper_finish), the PAF
// line of a read (src/rmap.cpp:696-801, 950-965) and the sequence-until entries.  The rounds themselves are rawdtw_mapper_round.cpp; the
// state both work on is rawdtw_mapper_state.h.
//
// rawalign_amd/mapper.py is the Python mirror of the control flow; tests/test_mapper.py and tests/test_abi_shim.py compare the two and
// the oracle-scored flow line by line.  Pure host code above the C ABI: no kernel is launched from here directly.
#include <cmath>
#include <memory>
#include <new>

#include "rawdtw_mapper_state.h"

using namespace rawdtw_map;

namespace {

std::string fmt_f(double x) // std::to_string(float/double) == printf("%f")
{
    char b[64];
    snprintf(b, sizeof b, "%f", x);
    return b;
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


} // namespace

extern "C" {

int rawdtw_mapper_create(rawdtw_ctx *ctx, const rawdtw_mapper_opt_t *opt, uint32_t n_seq, const char *const *seq_names,
                         const uint32_t *seq_len, rawdtw_mapper **out)
{
    if (!out) return RAWDTW_ERR_INVALID;
    *out = nullptr;
    if (!opt || (n_seq && (!seq_names || !seq_len)) || opt->slot_events == 0 || opt->max_reads == 0) return RAWDTW_ERR_INVALID;
    // rmap.cpp:301-304; 2 (local) where the context opted in (rawdtw_set_border_local) and on a scorer-only mapper, which scores nothing here
    int local_on = 1;
    if (ctx && rawdtw_get_border_local(ctx, &local_on) != RAWDTW_OK) return RAWDTW_ERR_INVALID;
    if (opt->align.border_constraint != 0 && opt->align.border_constraint != 1 && !(opt->align.border_constraint == 2 && local_on)) return RAWDTW_ERR_INVALID;
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
        if (st == RAWDTW_OK) st = rawdtw_set_border_local(m->groups[1].ctx, local_on); // (... under the same border constraints)
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
    m->own.release(); // (pinned memory goes before the context that may own the device)
    for (Group &g : m->groups) {
        for (RoundArrays &ra : g.buf) ra = RoundArrays();
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
    if (rounds) *rounds = m->cnt.rounds;
    if (parts_scored) *parts_scored = m->cnt.parts_scored;
    if (parts_reused) *parts_reused = m->cnt.parts_reused;
    return RAWDTW_OK;
}

int rawdtw_mapper_timing(const rawdtw_mapper *m, double out[8])
{
    if (!m || !out) return RAWDTW_ERR_INVALID;
    for (int i = 0; i < 5; i++) out[i] = m->timing[i];
    out[5] = (double)m->cnt.anchor_bytes; out[6] = (double)m->cnt.event_bytes; out[7] = (double)m->cnt.other_bytes;
    return RAWDTW_OK;
}


int rawdtw_mapper_log(const rawdtw_mapper *m, const char **text)
{
    if (!m || !text) return RAWDTW_ERR_INVALID;
    *text = m->log.c_str();
    return RAWDTW_OK;
}


int rawdtw_mapper_signal_stats(const rawdtw_mapper *m, uint64_t *rounds, uint64_t *retried_rounds, uint64_t *sample_bytes_to_device,
                               uint64_t *event_bytes_crossed)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (rounds) *rounds = m->cnt.sig_rounds;
    if (retried_rounds) *retried_rounds = m->cnt.sig_retried;
    if (sample_bytes_to_device) *sample_bytes_to_device = m->cnt.sig_sample_bytes;
    if (event_bytes_crossed) *event_bytes_crossed = m->cnt.event_bytes; // (the mapper sends events up and fetches none: slot 6 is all that crosses)
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
    if (rounds) *rounds = m->cnt.re_rounds;
    if (reads_device) *reads_device = m->cnt.re_reads;
    if (reads_declined) *reads_declined = m->cnt.re_declined;
    return RAWDTW_OK;
}

int rawdtw_mapper_kept_stats(const rawdtw_mapper *m, uint64_t *reads_from_device, uint64_t *reads_from_host, uint64_t *seeds_from_device,
                             uint64_t *seeds_from_host, uint64_t *reads_not_kept)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (reads_from_device) *reads_from_device = m->cnt.kp_reads_dev;
    if (reads_from_host) *reads_from_host = m->cnt.kp_reads_host;
    if (seeds_from_device) *seeds_from_device = m->cnt.kp_seeds_dev;
    if (seeds_from_host) *seeds_from_host = m->cnt.kp_seeds_host;
    if (reads_not_kept) *reads_not_kept = m->cnt.kp_not_kept;
    return RAWDTW_OK;
}

int rawdtw_mapper_decline_stats(const rawdtw_mapper *m, uint64_t *rounds_with_declines, uint64_t *reads_declined_seeds, uint64_t *reads_declined_chains,
                                uint64_t *reads_chained_device, uint64_t *seed_bytes_to_host)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (rounds_with_declines) *rounds_with_declines = m->cnt.dc_rounds;
    if (reads_declined_seeds) *reads_declined_seeds = m->cnt.dc_reads_seeds;
    if (reads_declined_chains) *reads_declined_chains = m->cnt.dc_reads_chains;
    if (reads_chained_device) *reads_chained_device = m->cnt.dc_reads_device;
    if (seed_bytes_to_host) *seed_bytes_to_host = m->cnt.dc_seed_bytes;
    return RAWDTW_OK;
}

int rawdtw_mapper_resident_stats(const rawdtw_mapper *m, uint64_t *resident_rounds, uint64_t *fallback_rounds, uint64_t *hit_bytes_to_host,
                                 uint64_t *seed_bytes_to_device)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (resident_rounds) *resident_rounds = m->cnt.res_rounds;
    if (fallback_rounds) *fallback_rounds = m->cnt.res_fallbacks;
    if (hit_bytes_to_host) *hit_bytes_to_host = m->cnt.res_hit_bytes;
    if (seed_bytes_to_device) *seed_bytes_to_device = m->cnt.res_seed_bytes;
    return RAWDTW_OK;
}

// The banded path of a global + banded --dtw-output-cigar mapper (include/rawdtw.h, "banded traceback"; the reference stops at
// rmap.cpp:223-225).  Off by default: the refusal, its status and its wording stay.  Sparse mappers are untouched by it
// (rmap.cpp:283-284 always calls DTW_global_tb).  It is NOT faster than switching the run to the full matrix: on 1 024 windows of
// 3 000 x 3 000 at radius 300 the banded call took 1.7 times the full-matrix call ("Banded traceback", Speed); what it
// saves is workspace, a quarter of the direction bytes.
int rawdtw_mapper_set_banded_cigar(rawdtw_mapper *m, int on)
{
    if (!m) return RAWDTW_ERR_INVALID;
    m->banded_cigar = on != 0;
    return RAWDTW_OK;
}

// aln:s: from the device (include/rawdtw.h, "aln text").  Off by default: the finish below is then what it was.  The banded and the local
// finish have traceback units of their own and keep the host formatter whatever this says.
int rawdtw_mapper_set_device_text(rawdtw_mapper *m, int on)
{
    if (!m) return RAWDTW_ERR_INVALID;
    m->device_text = on != 0;
    return RAWDTW_OK;
}

// --dtw-output-cigar (rmap.cpp:715-717): the best chain of every mapped read through DTW_global_tb once more, its path as the
// aln:s: string with the reference's two quirks (rmap.cpp:230-233, 283-289).  All reads' jobs go to the device in ONE call;
// the paths come back as steps and distances (rawdtw_traceback_batch_steps: 5 bytes an element) and the one host formatter
// (rawdtw_aln_text_host) makes every job's text of them -- or, under rawdtw_mapper_set_device_text, the text itself comes back.
int rawdtw_mapper_finish(rawdtw_mapper *m)
{
    if (!m) return RAWDTW_ERR_INVALID;
    if (!(m->opt.flag & 0x4)) return RAWDTW_OK;
    if (!m->ctx) return fail(m, RAWDTW_ERR_NO_DEVICE, "--dtw-output-cigar needs a device context");
    // Where a read's events are: in the host's copy, laid one read behind the other and uploaded by the traceback call -- or, once a round from
    // signal has been committed ("signal_cigar": no host copy of its chunks exists), where every round of a context mapper put them: the read's slot
    // of the arena, which the traceback then reads as it lies.  The event base of a read's jobs and the traceback entry are all that differs.
    const bool arena = m->finish_from_arena;
    // the banded path (rawdtw_mapper_set_banded_cigar): the job the scoring built (radius max(1, (int)(n * frac))), walked as well
    const bool banded = m->banded_cigar && m->opt.align.border_constraint == 0 && m->opt.align.fill_method != 0;
    // local (include/rawdtw.h, "local border"): the chain's one job through DTW_semiglobal_tb; the walk starts at (0, j0)
    const bool local = m->opt.align.border_constraint == 2;
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
        const int st = rawdtw_chain_build_jobs(&m->opt.align, ch.anchors.data(), na, rb, ev_base, banded ? 0 : 1, jobs.data() + j0);
        if (st != RAWDTW_OK) return fail(m, st, st == RAWDTW_ERR_UNSUPPORTED ? "banded global alignment with --dtw-output-cigar is not implemented (rmap.cpp:223-225)" : "job building failed");
        jobs.resize(j0 + nj);
        items.push_back(Item{r, j0, nj, ev_base});
        if (!arena) events.insert(events.end(), rd.events.begin(), rd.events.end());
    }
    if (items.empty()) return RAWDTW_OK;
    const uint64_t nj_all = jobs.size();
    // One rec a job says what every element of its text moves by (include/rawdtw.h, "aln text"): a sparse part's elements all move by
    // its part's start anchor (mode 1, rmap.cpp:286-289); a global chain's last element moves by len times the chain's start anchor
    // (mode 0: the offsets are added to alignment.back() once per element, rmap.cpp:230-233), the banded path alike; a local chain's
    // elements move by the chain's start anchor, the sparse branch's way, and its walk starts at (0, j0).
    std::vector<rawdtw_aln_rec_t> recs(nj_all);
    for (const Item &it : items) {
        const MChain &ch = m->reads[it.read].chains[0];
        const uint32_t na = (uint32_t)ch.anchors.size(), parts = na - 1;
        for (uint32_t k = 0; k < it.nj; k++) {
            const rawdtw_anchor_t &s0 = m->opt.align.border_constraint == 1 ? ch.anchors[parts - k] : ch.anchors[na - 1];
            recs[it.job0 + k] = rawdtw_aln_rec_t{s0.query_position, s0.target_position, 0u, m->opt.align.border_constraint != 0 ? 1u : 0u, 0};
        }
    }
    std::vector<uint64_t> toff(nj_all + 1, 0);
    std::vector<uint32_t> plen(nj_all);
    std::vector<float> cost(nj_all);
    std::unique_ptr<char[]> text; // (not value-initialised: the bound is a few times the text)
    uint64_t bytes = 0;
    if (nj_all && !arena) m->arena_replaced = true;
    if (m->device_text && !local && !banded && nj_all) {
        // rawdtw_mapper_set_device_text: the jobs through the traceback's text form, the paths stay on the device
        const uint64_t cap = rawdtw_aln_text_bound(jobs.data(), recs.data(), nj_all);
        text.reset(new (std::nothrow) char[cap + 1]);
        if (!text) return fail(m, RAWDTW_ERR_OOM, "no memory for the aln:s: text");
        const int st = arena ? rawdtw_traceback_arena_text(m->ctx, jobs.data(), nj_all, recs.data(), cost.data(), plen.data(), toff.data(), text.get(), cap, &bytes)
                             : rawdtw_traceback_batch_text(m->ctx, jobs.data(), nj_all, events.data(), events.size(), recs.data(), cost.data(), plen.data(),
                                                           toff.data(), text.get(), cap, &bytes);
        if (st != RAWDTW_OK) return fail(m, st, rawdtw_last_error(m->ctx));
    } else if (nj_all) {
        // the paths come home as steps and distances, and the host formatter (rawdtw_aln_text_host) makes the text of them
        std::vector<uint64_t> poff(nj_all + 1, 0);
        for (uint64_t k = 0; k < nj_all; k++) poff[k + 1] = poff[k] + jobs[k].n + jobs[k].m - 1;
        std::vector<uint8_t> step(poff[nj_all] + 1);
        std::vector<float> pd(poff[nj_all] + 1);
        std::vector<uint32_t> j0(local ? nj_all : 0);
        int st = local ? rawdtw_semiglobal_traceback_steps(m->ctx, jobs.data(), nj_all, arena ? nullptr : events.data(), events.size(), cost.data(),
                                                           j0.data(), poff.data(), plen.data(), step.data(), pd.data())
                 : banded ? rawdtw_banded_traceback_steps(m->ctx, jobs.data(), nj_all, arena ? nullptr : events.data(), events.size(), cost.data(),
                                                        poff.data(), plen.data(), step.data(), pd.data())
                 : arena ? rawdtw_traceback_arena_steps(m->ctx, jobs.data(), nj_all, cost.data(), poff.data(), plen.data(), step.data(), pd.data())
                       : rawdtw_traceback_batch_steps(m->ctx, jobs.data(), nj_all, events.data(), events.size(), cost.data(), poff.data(), plen.data(), step.data(), pd.data());
        if (st != RAWDTW_OK) return fail(m, st, rawdtw_last_error(m->ctx));
        for (uint64_t k = 0; k < j0.size(); k++) recs[k].j0 = j0[k];
        const uint64_t cap = rawdtw_aln_text_bound(jobs.data(), recs.data(), nj_all);
        text.reset(new (std::nothrow) char[cap + 1]);
        if (!text) return fail(m, RAWDTW_ERR_OOM, "no memory for the aln:s: text");
        st = rawdtw_aln_text_host(step.data(), pd.data(), poff.data(), plen.data(), recs.data(), nj_all, m->pool->threads(), toff.data(), text.get(), cap, &bytes);
        if (st != RAWDTW_OK) return fail(m, st, "the aln:s: text does not fit its bound");
    }
    // The jobs of a read are consecutive, so its aln:s: is one stretch of the text.
    std::vector<std::string> logs(items.size());
    m->pool->run(items.size(), 4, [&](size_t x) {
        const Item &it = items[x];
        MChain &ch = m->reads[it.read].chains[0];
        ch.alignment_score = rawdtw_chain_replay(&m->opt.align, ch.anchors.data(), (uint32_t)ch.anchors.size(), cost.data() + it.job0, -1e10f); // rmap.cpp:306 on the summed costs
        ch.aln.assign(it.nj ? text.get() + toff[it.job0] : "", toff[it.job0 + it.nj] - toff[it.job0]);
        ch.has_aln = true;
        if (m->opt.flag & 0x8) logs[x] = log_scores_line(ch.chaining_score, ch.alignment_score);
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
