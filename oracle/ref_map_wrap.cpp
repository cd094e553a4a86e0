// ref_map_wrap.cpp -- C entry points around the REFERENCE's own mapping code (src/rmap.cpp and the units it calls).
//
// TEST INFRASTRUCTURE.  This file is ours.  oracle/Makefile compiles it together with the reference's units, read where
// they lie and never copied, into oracle/_ref/libref_map0.so (-ffp-contract=off) and libref_map1.so (the reference's own
// flags on an FMA target, where rmap.cpp:306 contracts).  rmap.cpp is compiled INTO this translation unit (the #include
// below), which makes its static map_worker_for callable and brings every declaration this file uses; the one function
// called here that no header of the reference declares is ri_idx_sort (rawindex.cpp:252), declared below.
//
// What is ours here is glue only: an index assembled in memory from signal arrays (the calls rawindex.cpp:127-176 makes,
// minus the FASTA reader), a flat option struct laid over ri_mapopt_init, the hit list of a chunk (the calls of
// rmap.cpp:367-391, unpacked), one chunk round for a read (the calls of ri_map_frag, rmap.cpp:545-578, with events handed in
// instead of detected), align_chain on a caller's chain, and map_worker_for on a caller's raw signal.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "rmap.cpp" // from -I$(REF_SRC): the reference's mapping unit, as it lies

void ri_idx_sort(ri_idx_t *ri, int n_threads); // rawindex.cpp:252 (C++ linkage; in no header)

namespace {

struct RefMap {
    ri_idx_t *ri = nullptr;
    ri_mapopt_t opt;
    pipeline_mt p;
    void *km = nullptr;
    std::vector<ri_reg1_t *> regs;
    std::vector<uint32_t> hits;     // last rm_hits: 4 values a hit
    dtw_result last_tb;             // last rm_align_chain with cigar
    std::string last_tags;          // last rm_map_read
    std::vector<std::string> names;
};

} // namespace

extern "C" {

// must match oracle/loader.py RefMapOpt
struct rm_opt {
    int64_t flag;
    uint32_t chunk_size, min_events, max_num_chunk;
    uint32_t max_gap_length, max_target_gap_length, chaining_band_length, max_num_skips, min_num_anchors, num_best_chains;
    float min_chaining_score;
    uint32_t min_chain_anchor, dtw_border_constraint, dtw_fill_method;
    float dtw_band_radius_frac, dtw_match_bonus, dtw_min_score, min_bestmap_ratio, min_meanmap_ratio;
};

void rm_opt_defaults(rm_opt *o)
{
    ri_mapopt_t m;
    ri_mapopt_init(&m);
    o->flag = m.flag; o->chunk_size = m.chunk_size; o->min_events = m.min_events; o->max_num_chunk = m.max_num_chunk;
    o->max_gap_length = m.max_gap_length; o->max_target_gap_length = m.max_target_gap_length;
    o->chaining_band_length = m.chaining_band_length; o->max_num_skips = m.max_num_skips; o->min_num_anchors = m.min_num_anchors;
    o->num_best_chains = m.num_best_chains; o->min_chaining_score = m.min_chaining_score; o->min_chain_anchor = m.min_chain_anchor;
    o->dtw_border_constraint = m.dtw_border_constraint; o->dtw_fill_method = m.dtw_fill_method;
    o->dtw_band_radius_frac = m.dtw_band_radius_frac; o->dtw_match_bonus = m.dtw_match_bonus; o->dtw_min_score = m.dtw_min_score;
    o->min_bestmap_ratio = m.min_bestmap_ratio; o->min_meanmap_ratio = m.min_meanmap_ratio;
}

void rm_set_opt(void *h, const rm_opt *o)
{
    ri_mapopt_t &m = static_cast<RefMap *>(h)->opt;
    ri_mapopt_init(&m);
    m.flag = o->flag; m.chunk_size = o->chunk_size; m.min_events = o->min_events; m.max_num_chunk = o->max_num_chunk;
    m.max_gap_length = o->max_gap_length; m.max_target_gap_length = o->max_target_gap_length;
    m.chaining_band_length = o->chaining_band_length; m.max_num_skips = o->max_num_skips; m.min_num_anchors = o->min_num_anchors;
    m.num_best_chains = o->num_best_chains; m.min_chaining_score = o->min_chaining_score; m.min_chain_anchor = o->min_chain_anchor;
    m.dtw_border_constraint = o->dtw_border_constraint; m.dtw_fill_method = o->dtw_fill_method;
    m.dtw_band_radius_frac = o->dtw_band_radius_frac; m.dtw_match_bonus = o->dtw_match_bonus; m.dtw_min_score = o->dtw_min_score;
    m.min_bestmap_ratio = o->min_bestmap_ratio; m.min_meanmap_ratio = o->min_meanmap_ratio;
}

// An index over n_seq sequences given as signal arrays (strand 1 = forward, as rawindex.cpp:141-147 sketches them).
void *rm_create(uint32_t n_seq, const float *const *fwd, const float *const *rev, const uint32_t *lens, const char *const *names,
                int b, int w, int e, int n, int q, int lq, int k)
{
    RefMap *m = new RefMap();
    ri_idx_t *ri = ri_idx_init(b, w, e, n, q, lq, k);
    ri->forward_signals = (float **)calloc(n_seq, sizeof(float *));
    ri->reverse_signals = (float **)calloc(n_seq, sizeof(float *));
    ri->signal_lengths = (uint32_t *)calloc(n_seq, sizeof(uint32_t));
    ri->seq = (ri_idx_seq_t *)calloc(n_seq, sizeof(ri_idx_seq_t));
    m->names.resize(n_seq);
    uint64_t sum_len = 0;
    for (uint32_t s = 0; s < n_seq; s++) {
        mm128_v a = {0, 0, 0};
        ri->forward_signals[s] = (float *)malloc(lens[s] * sizeof(float));
        ri->reverse_signals[s] = (float *)malloc(lens[s] * sizeof(float));
        memcpy(ri->forward_signals[s], fwd[s], lens[s] * sizeof(float));
        memcpy(ri->reverse_signals[s], rev[s], lens[s] * sizeof(float));
        ri->signal_lengths[s] = lens[s];
        ri_sketch(0, ri->forward_signals[s], s, 1, (int)lens[s], w, e, n, q, lq, k, &a);
        ri_sketch(0, ri->reverse_signals[s], s, 0, (int)lens[s], w, e, n, q, lq, k, &a);
        ri_idx_add(ri, (int)a.n, a.a);
        ri_kfree(0, a.a);
        m->names[s] = names[s];
        ri->seq[s].name = const_cast<char *>(m->names[s].c_str());
        ri->seq[s].len = lens[s];
        ri->seq[s].offset = sum_len;
        sum_len += lens[s];
    }
    ri->n_seq = n_seq;
    ri->n_sig = n_seq;
    ri_idx_sort(ri, 1);
    m->ri = ri;
    ri_mapopt_init(&m->opt);
    m->p.opt = &m->opt;
    m->p.ri = ri;
    m->p.n_threads = 1;
    m->km = ri_km_init();
    return m;
}

// (the index and the reads live as long as the process: test processes are short, and ri_idx_destroy would free the
// signal arrays through kalloc, which did not allocate them here)
void rm_reset_reads(void *h)
{
    RefMap *m = static_cast<RefMap *>(h);
    for (ri_reg1_t *r : m->regs) {
        if (r->tags) free(r->tags);
        free(r);
    }
    m->regs.clear();
    for (ri_events_t &e : m->p.events) free(e.values);
    m->p.events.clear();
    ri_km_destroy(m->km);
    m->km = ri_km_init();
}

uint32_t rm_new_read(void *h)
{
    RefMap *m = static_cast<RefMap *>(h);
    const uint32_t rid = (uint32_t)m->regs.size();
    ri_reg1_t *reg = (ri_reg1_t *)calloc(1, sizeof(ri_reg1_t)); // rmap.cpp:905-907
    reg->read_id = rid;
    reg->read_name = "read";
    m->regs.push_back(reg);
    ri_events_t ev;                                              // rmap.cpp:888-898
    ev.rid = rid; ev.name = 0; ev.values = 0; ev.length = 0;
    m->p.events.push_back(ev);
    return rid;
}

// The seed hits of a chunk's events in the order gen_chains meets them; 4 values a hit (sequence, strand, target position,
// query position in the chunk).  Returns the count; rm_hits_get copies them out.
uint64_t rm_hits(void *h, const float *events, uint32_t n)
{
    RefMap *m = static_cast<RefMap *>(h);
    const ri_idx_t *ri = m->ri;
    m->hits.clear();
    mm128_v riv = {0, 0, 0};
    ri_sketch(m->km, events, 0, 0, (int)n, ri->w, ri->e, ri->n, ri->q, ri->lq, ri->k, &riv);
    for (size_t i = 0; i < riv.n; i++) {
        int t = 0;
        const uint64_t *cr = ri_idx_get(ri, riv.a[i].x >> RI_HASH_SHIFT, &t);
        const uint32_t qpos = (uint32_t)riv.a[i].y >> RI_POS_SHIFT;
        for (int s = 0; s < t; s++) {
            m->hits.push_back((uint32_t)(cr[s] >> RI_ID_SHIFT));
            m->hits.push_back((uint32_t)(cr[s] & 1));
            m->hits.push_back(((uint32_t)(cr[s] >> RI_POS_SHIFT)) & 0x7fffffffu);
            m->hits.push_back(qpos);
        }
    }
    ri_kfree(m->km, riv.a);
    return m->hits.size() / 4;
}

void rm_hits_get(void *h, uint32_t *out)
{
    RefMap *m = static_cast<RefMap *>(h);
    if (!m->hits.empty()) memcpy(out, m->hits.data(), m->hits.size() * sizeof(uint32_t));
}

// One chunk round of a read: what ri_map_frag does after detect_events (rmap.cpp:553-575), then the stop rule of rmap.cpp:692.
int rm_round(void *h, uint32_t rid, const float *chunk_events, uint32_t n_chunk_events)
{
    RefMap *m = static_cast<RefMap *>(h);
    ri_reg1_t *reg = m->regs[rid];
    ri_events_t &g = m->p.events[rid];
    float *grown = (float *)malloc(((size_t)g.length + n_chunk_events + 1) * sizeof(float));
    if (g.length) memcpy(grown, g.values, g.length * sizeof(float));
    if (n_chunk_events) memcpy(grown + g.length, chunk_events, n_chunk_events * sizeof(float));
    free(g.values);
    g.values = grown;
    g.length += n_chunk_events;
    if (n_chunk_events >= m->opt.min_events) {
        gen_chains(m->km, &m->p, m->ri, chunk_events, n_chunk_events, reg->offset, m->ri->n_seq, reg, &m->opt);
        reg->offset += n_chunk_events;
    }
    return is_mapped_with_high_confidence(reg, &m->opt) ? 1 : 0;
}

void rm_chain_counts(void *h, uint32_t rid, uint32_t *n_chains, uint64_t *n_anchors, uint32_t *offset)
{
    const ri_reg1_t *reg = static_cast<RefMap *>(h)->regs[rid];
    *n_chains = reg->chains ? reg->n_chains : 0;
    *n_anchors = 0;
    for (uint32_t c = 0; c < *n_chains; c++) *n_anchors += reg->chains[c].n_anchors;
    *offset = reg->offset;
}

// reg->chains, flattened; u32 fields a chain: sequence, strand, start, end, n_anchors, mapq; anchors as (target, query) pairs
void rm_chains_get(void *h, uint32_t rid, float *chaining_score, float *alignment_score, uint32_t *fields, uint32_t *anchors)
{
    const ri_reg1_t *reg = static_cast<RefMap *>(h)->regs[rid];
    const uint32_t nc = reg->chains ? reg->n_chains : 0;
    for (uint32_t c = 0; c < nc; c++) {
        const ri_chain_t &ch = reg->chains[c];
        chaining_score[c] = ch.chaining_score;
        alignment_score[c] = ch.alignment_score;
        uint32_t *f = fields + 6 * c;
        f[0] = ch.reference_sequence_index; f[1] = (uint32_t)ch.strand; f[2] = ch.start_position; f[3] = ch.end_position;
        f[4] = ch.n_anchors; f[5] = ch.mapq;
        for (uint32_t a = 0; a < ch.n_anchors; a++) {
            *anchors++ = ch.anchors[a].target_position;
            *anchors++ = ch.anchors[a].query_position;
        }
    }
}

// The reference's align_chain (rmap.cpp:181) on a caller's chain.  anchors: (target, query) pairs, end-first.  With cigar the
// dtw_result stays in the handle (rm_tb_len / rm_tb_get).  Global + banded + cigar is an assert(false) in the reference: not
// to be asked for.
float rm_align_chain(void *h, const uint32_t *anchors, uint32_t n_anchors, uint32_t seq, int strand, const float *read_events,
                     uint32_t n_read_events, int cigar, float min_score)
{
    RefMap *m = static_cast<RefMap *>(h);
    std::vector<ri_anchor_t> an(n_anchors);
    for (uint32_t a = 0; a < n_anchors; a++) { an[a].target_position = anchors[2 * a]; an[a].query_position = anchors[2 * a + 1]; }
    ri_chain_t ch = ri_chain_t();
    ch.reference_sequence_index = seq;
    ch.strand = strand;
    ch.n_anchors = n_anchors;
    ch.anchors = an.data();
    align_chain(ch, m->ri, read_events, n_read_events, 0, &m->opt, cigar != 0, min_score);
    if (cigar) m->last_tb = ch.dtw_result;
    return ch.alignment_score;
}

uint64_t rm_tb_len(void *h, float *cost)
{
    RefMap *m = static_cast<RefMap *>(h);
    *cost = m->last_tb.cost;
    return m->last_tb.alignment.size();
}

void rm_tb_get(void *h, uint64_t *pi, uint64_t *pj, float *pd)
{
    RefMap *m = static_cast<RefMap *>(h);
    for (size_t k = 0; k < m->last_tb.alignment.size(); k++) {
        pi[k] = (uint64_t)m->last_tb.alignment[k].position.i;
        pj[k] = (uint64_t)m->last_tb.alignment[k].position.j;
        pd[k] = m->last_tb.alignment[k].difference;
    }
}

// A whole read through the reference's own chunk loop (map_worker_for, rmap.cpp:667): raw signal in pA in, the record it
// leaves in reg0 out.  out[9]: mapped, ref_id, read_start_position, read_end_position, read_length,
// fragment_start_position, fragment_length, mapq, rev.  The tags stay in the handle (rm_tags), without the wall-clock mt:f:.
void rm_map_read(void *h, const float *sig, uint32_t l_sig, uint32_t *out)
{
    RefMap *m = static_cast<RefMap *>(h);
    const uint32_t rid = rm_new_read(h);
    ri_sig_t s;
    memset(&s, 0, sizeof s);
    s.rid = rid; s.l_sig = l_sig; s.name = const_cast<char *>("read");
    s.sig = const_cast<float *>(sig);
    ri_sig_t *sigs[1] = {&s};
    ri_tbuf_t *buf = ri_tbuf_init();
    ri_tbuf_t *bufs[1] = {buf};
    ri_reg1_t *reg = m->regs[rid];
    ri_reg1_t *regs[1] = {reg};
    step_mt st;
    st.p = &m->p; st.n_sig = 1; st.sig = sigs; st.reg = regs; st.buf = bufs;
    map_worker_for(&st, 0, 0);
    ri_tbuf_destroy(buf);
    reg->chains = 0; reg->n_chains = 0; // (freed by map_worker_for)
    out[0] = reg->mapped; out[1] = reg->ref_id; out[2] = reg->read_start_position; out[3] = reg->read_end_position;
    out[4] = reg->read_length; out[5] = reg->fragment_start_position; out[6] = reg->fragment_length; out[7] = reg->mapq; out[8] = reg->rev;
    std::string tags = reg->tags ? reg->tags : "";
    const size_t tab = tags.find('\t');
    m->last_tags = (tags.compare(0, 5, "mt:f:") == 0) ? (tab == std::string::npos ? "" : tags.substr(tab + 1)) : tags;
}

// the events the reference's detect_events left for the read (p->events[rid]); returns the count, copies when out is given
uint32_t rm_read_events(void *h, uint32_t rid, float *out)
{
    const ri_events_t &e = static_cast<RefMap *>(h)->p.events[rid];
    if (out && e.length) memcpy(out, e.values, e.length * sizeof(float));
    return e.length;
}

uint32_t rm_last_read(void *h) { return (uint32_t)static_cast<RefMap *>(h)->regs.size() - 1; }

const char *rm_tags(void *h) { return static_cast<RefMap *>(h)->last_tags.c_str(); }

// the reference's detect_events (revent.c:190) on one chunk of raw signal
uint32_t rm_detect_events(void *h, const float *sig, uint32_t s_len, float *out)
{
    RefMap *m = static_cast<RefMap *>(h);
    uint32_t n = 0;
    float *ev = detect_events(m->km, s_len, sig, &m->opt, &n);
    if (ev) { memcpy(out, ev, n * sizeof(float)); ri_kfree(m->km, ev); }
    return n;
}

} // extern "C"
