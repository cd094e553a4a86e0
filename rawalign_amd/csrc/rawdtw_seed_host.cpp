// rawdtw_seed_host.cpp -- seeding on the host: ri_sketch (src/rsketch.c:146-284) restated, the seed index of ri_idx_add / ri_idx_sort
// (src/rawindex.cpp:91-97, 194-246) built from signal arrays or read from a .ind file's buckets (rawindex.cpp:297-312, 354-374),
// ri_idx_get (rawindex.cpp:256-273) and the hit loop of gen_chains (src/rmap.cpp:371-391).  The CPU path of seeding and the
// comparator of the device path (rawdtw_seed.hip).  Pure host code, no device.
//
// The index is not khash: one open-addressing table of 16-byte slots over all buckets (rawdtw_seed.h), which is also the image
// the device probes.  Only ri_idx_get's answers are observable, and those are the same.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <new>
#include <string>
#include <thread>

#include "rawdtw_capi.h"
#include "rawdtw_seed.h"
#include "rawdtw_seed_min.h"

using namespace rawdtw;
using namespace rawdtw::seed;

namespace rawdtw {
namespace seed {

int check_pars(const rawdtw_seed_pars_t *p)
{
    if (!p) return RAWDTW_ERR_INVALID;
    if (p->e < 2 || p->e > 9) return RAWDTW_ERR_INVALID;             // rsketch.c:278
    if (p->w >= 256) return RAWDTW_ERR_INVALID;                       // rsketch.c:154
    if (p->q == 0 || p->q > 32 || p->lq > 30) return RAWDTW_ERR_INVALID; // signal >> (32 - q), 1UL << lq
    if ((uint64_t)(p->lq + 2) * p->e >= 64) return RAWDTW_ERR_INVALID;   // 1ULL << (quant_bit * e)
    return RAWDTW_OK;
}

bool entries_sorted(uint64_t n, const uint32_t *hash, const uint64_t *y)
{
    for (uint64_t i = 1; i < n; i++)
        if (hash[i] < hash[i - 1] || (hash[i] == hash[i - 1] && y[i] < y[i - 1])) return false;
    return true;
}

uint64_t next_serial()
{
    static std::atomic<uint64_t> n{0};
    return ++n;
}

// the table from entries grouped by hash, each hash's positions in the order ri_idx_get gives them
int fill_table(rawdtw_seed_index *six, const std::vector<Entry> &a)
{
    uint64_t n_keys = 0, n_multi = 0;
    for (size_t j = 0; j < a.size();) {
        size_t k = j + 1;
        while (k < a.size() && a[k].hash == a[j].hash) k++;
        n_keys++;
        if (k - j > 1) n_multi += k - j;
        j = k;
    }
    uint32_t lg = 4;
    while (lg < 31 && (1ull << lg) < 2 * n_keys) lg++; // (2^31 slots: 32 GiB; the probe's slot number is 32 bits)
    if ((1ull << lg) < 2 * n_keys) return RAWDTW_ERR_RANGE;
    try {
        six->slots.assign((size_t)1 << lg, Slot{0, 0, 0});
        six->pos.clear();
        six->pos.reserve(n_multi);
    } catch (const std::bad_alloc &) { return RAWDTW_ERR_OOM; }
    six->log2_slots = lg;
    const uint32_t mask = (uint32_t)six->slots.size() - 1;
    for (size_t j = 0; j < a.size();) {
        size_t k = j + 1;
        while (k < a.size() && a[k].hash == a[j].hash) k++;
        uint32_t at = first_slot(a[j].hash, lg);
        while (six->slots[at].count) at = (at + 1) & mask;
        if (k - j > 0xffffffffull) return RAWDTW_ERR_RANGE;
        Slot &s = six->slots[at];
        s.key = a[j].hash; s.count = (uint32_t)(k - j);
        if (k - j == 1) s.val = a[j].y;
        else {
            s.val = six->pos.size();
            for (size_t t = j; t < k; t++) six->pos.push_back(a[t].y);
        }
        j = k;
    }
    six->n_keys = n_keys; six->n_positions = a.size();
    return RAWDTW_OK;
}

} // namespace seed
} // namespace rawdtw

namespace {

uint32_t bits_of(float x)
{
    uint32_t b;
    memcpy(&b, &x, 4);
    return b;
}

// ri_sketch_reg (rsketch.c:223-274): emit(hash, i) for every e-mer, i the position of its last event
template <typename F> void sketch_reg(const rawdtw_seed_pars_t &p, const float *s, uint32_t len, F emit)
{
    const uint32_t quant_bit = p.lq + 2;
    const uint64_t mask_events = (1ULL << (quant_bit * p.e)) - 1;
    uint32_t kept = 0, last = 0;
    uint64_t quant = 0;
    for (uint32_t i = 0; i < len; i++) {
        if (skipped(s[i], s[last], i == 0)) continue;
        last = i;
        quant = (quant << quant_bit | code_of(bits_of(s[i]), p.q, p.lq)) & mask_events;
        if (++kept < p.e) continue;
        emit(hash32((uint32_t)quant), i);
    }
}

// ri_sketch_min (rsketch.c:146-221): the minimizer over windows of w e-mers.  x = hash << RI_HASH_SHIFT | span as the reference
// keeps it (the window compares x, and UINT64_MAX is its "none"); y = the position of the e-mer's FIRST event: the ring of e
// entries takes the position before it steps and the hash after (rsketch.c:184-186).
template <typename F> void sketch_min(const rawdtw_seed_pars_t &p, const float *s, uint32_t len, F emit)
{
    struct Item { uint64_t x, y; };
    const uint64_t none = ~0ull;
    const int w = (int)p.w;
    const uint32_t e = p.e, quant_bit = p.lq + 2;
    const uint64_t span = 6 + e - 1, mask_events = (1ULL << (quant_bit * e)) - 1;
    Item buf[256], ring[16], mn = {none, none};
    for (int j = 0; j < w; j++) buf[j] = Item{none, none};
    for (uint32_t j = 0; j < 16; j++) ring[j] = Item{0, 0};
    bool full = false;
    uint32_t ring_pos = 0, last = 0, l = 0;
    int buf_pos = 0, min_pos = 0;
    uint64_t quant = 0;
    auto push = [&](const Item &it) { emit((uint32_t)(it.x >> 6), (uint32_t)it.y); };
    for (uint32_t i = 0; i < len; i++) {
        const float d = s[i] - s[last];
        if (i > 0 && (d < 0.0f ? -d : d) < kLastSigDiff) continue; // (no RI_MASK_SIGNAL test here, rsketch.c:172)
        l++;
        last = i;
        quant = (quant << quant_bit | code_of(bits_of(s[i]), p.q, p.lq)) & mask_events;
        ring[ring_pos].y = i;
        if (++ring_pos == e) { full = true; ring_pos = 0; }
        ring[ring_pos].x = (uint64_t)hash32((uint32_t)quant) << 6 | span;
        if (!full) continue;
        const Item info = ring[ring_pos];
        buf[buf_pos] = info;
        if (l == (uint32_t)w + e - 1 && mn.x != none) { // the first window: identical e-mers are not stored yet
            for (int j = buf_pos + 1; j < w; ++j)
                if (mn.x == buf[j].x && buf[j].y != mn.y) push(buf[j]);
            for (int j = 0; j < buf_pos; ++j)
                if (mn.x == buf[j].x && buf[j].y != mn.y) push(buf[j]);
        }
        if (info.x <= mn.x) { // a new minimum: the old one goes out
            if (l >= (uint32_t)w + e && mn.x != none) push(mn);
            mn = info; min_pos = buf_pos;
        } else if (buf_pos == min_pos) { // the old minimum has left the window
            if (l >= (uint32_t)w + e - 1 && mn.x != none) push(mn);
            mn.x = none;
            for (int j = buf_pos + 1; j < w; ++j)
                if (mn.x >= buf[j].x) { mn = buf[j]; min_pos = j; }
            for (int j = 0; j <= buf_pos; ++j)
                if (mn.x >= buf[j].x) { mn = buf[j]; min_pos = j; }
            if (l >= (uint32_t)w + e - 1 && mn.x != none) {
                for (int j = buf_pos + 1; j < w; ++j)
                    if (mn.x == buf[j].x && mn.y != buf[j].y) push(buf[j]);
                for (int j = 0; j <= buf_pos; ++j)
                    if (mn.x == buf[j].x && mn.y != buf[j].y) push(buf[j]);
            }
        }
        if (++buf_pos == w) buf_pos = 0;
    }
    if (mn.x != none) push(mn);
}

template <typename F> void sketch(const rawdtw_seed_pars_t &p, const float *s, uint32_t len, F emit)
{
    if (p.w) sketch_min(p, s, len, emit); // rsketch.c:282-283
    else sketch_reg(p, s, len, emit);
}

const Slot *find(const rawdtw_seed_index *six, uint32_t hash)
{
    if (six->slots.empty()) return nullptr;
    const uint32_t mask = (uint32_t)six->slots.size() - 1;
    for (uint32_t at = first_slot(hash, six->log2_slots);; at = (at + 1) & mask) {
        const Slot &s = six->slots[at];
        if (s.count == 0) return nullptr;
        if (s.key == hash) return &s;
    }
}

bool by_hash_then_position(const Entry &a, const Entry &b) { return a.hash != b.hash ? a.hash < b.hash : a.y < b.y; }

} // namespace

extern "C" {

int rawdtw_seed_index_build(uint32_t n_seq, const float *const *fwd, const float *const *rev, const uint32_t *len,
                            const rawdtw_seed_pars_t *pars, int threads, rawdtw_seed_index **out)
{
    if (!out) return RAWDTW_ERR_INVALID;
    *out = nullptr;
    if (check_pars(pars) != RAWDTW_OK || (n_seq && (!fwd || !rev || !len))) return RAWDTW_ERR_INVALID;
    for (uint32_t s = 0; s < n_seq; s++)
        if (len[s] && (!fwd[s] || !rev[s])) return RAWDTW_ERR_INVALID;
    rawdtw_seed_index *six = new (std::nothrow) rawdtw_seed_index;
    if (!six) return RAWDTW_ERR_OOM;
    six->pars = *pars; six->n_seq = n_seq; six->serial = next_serial();
    // a list per (sequence, strand), filled in parallel and joined in the reference's order (forward first, rawindex.cpp:141-147);
    // the order of the positions inside a key comes from the sort below either way
    std::vector<std::vector<Entry>> part(2ull * n_seq);
    const int T = std::max(1, std::min(threads, 64));
    std::atomic<uint64_t> next{0};
    std::atomic<bool> oom{false};
    capi::parallel_for(T, [&](int) {
        for (uint64_t j; (j = next.fetch_add(1)) < 2ull * n_seq;) {
            const uint32_t s = (uint32_t)(j / 2), strand = j % 2 == 0 ? 1u : 0u;
            const float *x = strand ? fwd[s] : rev[s];
            try {
                sketch(*pars, x, len[s], [&](uint32_t h, uint32_t i) {
                    part[j].push_back(Entry{h, (uint64_t)s << 32 | (uint32_t)(i << 1) | strand}); // rsketch.c:253
                });
            } catch (const std::bad_alloc &) { oom = true; }
        }
    });
    int st = oom ? RAWDTW_ERR_OOM : RAWDTW_OK;
    std::vector<Entry> all;
    if (st == RAWDTW_OK) {
        try {
            size_t total = 0;
            for (auto &v : part) total += v.size();
            all.reserve(total);
            for (auto &v : part) { all.insert(all.end(), v.begin(), v.end()); std::vector<Entry>().swap(v); }
            std::sort(all.begin(), all.end(), by_hash_then_position);
        } catch (const std::bad_alloc &) { st = RAWDTW_ERR_OOM; }
    }
    if (st == RAWDTW_OK) st = fill_table(six, all);
    if (st != RAWDTW_OK) { delete six; return st; }
    *out = six;
    return RAWDTW_OK;
}

int rawdtw_seed_index_load(const rawdtw_index *idx, rawdtw_seed_index **out)
{
    if (!out) return RAWDTW_ERR_INVALID;
    *out = nullptr;
    if (!idx) return RAWDTW_ERR_INVALID;
    rawdtw_seed_pars_t p{idx->pars[0], idx->pars[1], idx->pars[2], idx->pars[3], idx->pars[4], idx->pars[5]};
    if (check_pars(&p) != RAWDTW_OK) return RAWDTW_ERR_INVALID;
    FILE *f = fopen(idx->path.c_str(), "rb");
    if (!f) return RAWDTW_ERR_INVALID;
    rawdtw_seed_index *six = new (std::nothrow) rawdtw_seed_index;
    if (!six) { fclose(f); return RAWDTW_ERR_OOM; }
    six->pars = p; six->n_seq = (uint32_t)idx->lens.size(); six->serial = next_serial();
    int st = RAWDTW_OK;
    std::vector<Entry> all;
    uint64_t records = 0;
    try {
        bool ok = fseeko(f, (off_t)idx->bucket_pos, SEEK_SET) == 0;
        std::vector<uint64_t> bp, kv;
        for (uint32_t b = 0; ok && b < (1u << 14); b++) { // ri_idx_load: b = 14 (rawindex.cpp:330)
            uint32_t n = 0, size = 0;
            ok = fread(&n, 4, 1, f) == 1;
            if (!ok) break;
            bp.resize(n);
            ok = (n == 0 || fread(bp.data(), 8, n, f) == n) && fread(&size, 4, 1, f) == 1;
            if (!ok) break;
            kv.resize(2ull * size);
            ok = size == 0 || fread(kv.data(), 8, 2ull * size, f) == 2ull * size;
            for (uint32_t j = 0; ok && j < size; j++) {
                const uint64_t key = kv[2 * j], val = kv[2 * j + 1], hash = (key >> 1) << 14 | b;
                if (hash >> 32) { ok = false; break; }
                if (key & 1) all.push_back(Entry{(uint32_t)hash, val});
                else {
                    const uint64_t start = val >> 32, count = (uint32_t)val;
                    if (count == 0 || start + count > n) { ok = false; break; }
                    // (ri_idx_get hands the list out as it lies in the file: ascending where ri_idx_dump wrote it)
                    for (uint64_t t = 0; t < count; t++) all.push_back(Entry{(uint32_t)hash, bp[start + t]});
                }
                records++;
            }
        }
        if (!ok) st = RAWDTW_ERR_INVALID;
        // by hash alone and stable: a key's positions keep the file's order
        if (st == RAWDTW_OK) std::stable_sort(all.begin(), all.end(), [](const Entry &a, const Entry &b) { return a.hash < b.hash; });
    } catch (const std::bad_alloc &) { st = RAWDTW_ERR_OOM; }
    fclose(f);
    if (st == RAWDTW_OK) st = fill_table(six, all);
    if (st == RAWDTW_OK && six->n_keys != records) st = RAWDTW_ERR_INVALID; // a hash listed twice
    if (st != RAWDTW_OK) { delete six; return st; }
    *out = six;
    return RAWDTW_OK;
}

int rawdtw_seed_index_get(const rawdtw_seed_index *six, uint64_t hash, const uint64_t **pos, uint32_t *n)
{
    if (!six || !pos || !n) return RAWDTW_ERR_INVALID;
    *pos = nullptr; *n = 0;
    if (six->resident) return RAWDTW_ERR_UNSUPPORTED; // (no host copy, and "no hit" would be a lie: rawdtw_seed_index_fetch first)
    if (hash >> 32) return RAWDTW_OK; // (no sketch emits such a hash)
    const Slot *s = find(six, (uint32_t)hash);
    if (!s) return RAWDTW_OK;
    *n = s->count;
    *pos = s->count == 1 ? &s->val : six->pos.data() + s->val;
    return RAWDTW_OK;
}

int rawdtw_seed_index_info(const rawdtw_seed_index *six, uint32_t *n_seq, uint64_t *n_keys, uint64_t *n_positions, uint64_t *table_bytes,
                           rawdtw_seed_pars_t *pars)
{
    if (!six) return RAWDTW_ERR_INVALID;
    if (n_seq) *n_seq = six->n_seq;
    if (n_keys) *n_keys = six->n_keys;
    if (n_positions) *n_positions = six->n_positions;
    if (table_bytes) *table_bytes = six->resident ? ((uint64_t)1 << six->log2_slots) * sizeof(Slot) + six->n_list * 8 : six->slots.size() * sizeof(Slot) + six->pos.size() * 8;
    if (pars) *pars = six->pars;
    return RAWDTW_OK;
}

int rawdtw_seed_index_keys(const rawdtw_seed_index *six, uint32_t *hashes)
{
    if (!six || (six->n_keys && !hashes)) return RAWDTW_ERR_INVALID;
    if (six->resident) return RAWDTW_ERR_UNSUPPORTED; // (rawdtw_seed_index_fetch first)
    uint64_t k = 0;
    for (const Slot &s : six->slots)
        if (s.count) hashes[k++] = s.key;
    return RAWDTW_OK;
}

int rawdtw_seed_index_is_resident(const rawdtw_seed_index *six)
{
    return six && six->resident ? 1 : 0;
}

int rawdtw_seed_index_from_entries(const rawdtw_seed_pars_t *pars, uint32_t n_seq, uint64_t n, const uint32_t *hash, const uint64_t *y,
                                   rawdtw_seed_index **out)
{
    if (!out) return RAWDTW_ERR_INVALID;
    *out = nullptr;
    if (check_pars(pars) != RAWDTW_OK || (n && (!hash || !y)) || !entries_sorted(n, hash, y)) return RAWDTW_ERR_INVALID;
    rawdtw_seed_index *six = new (std::nothrow) rawdtw_seed_index;
    if (!six) return RAWDTW_ERR_OOM;
    six->pars = *pars; six->n_seq = n_seq; six->serial = next_serial();
    int st = RAWDTW_OK;
    std::vector<Entry> all;
    try {
        all.resize(n);
        for (uint64_t i = 0; i < n; i++) all[i] = Entry{hash[i], y[i]};
    } catch (const std::bad_alloc &) { st = RAWDTW_ERR_OOM; }
    if (st == RAWDTW_OK) st = fill_table(six, all);
    if (st != RAWDTW_OK) { delete six; return st; }
    *out = six;
    return RAWDTW_OK;
}

int rawdtw_seed_index_destroy(rawdtw_seed_index *six)
{
    delete six;
    return RAWDTW_OK;
}

int rawdtw_seed_sketch(const rawdtw_seed_pars_t *pars, const float *events, uint32_t n, uint32_t *hash_out, uint32_t *pos_out, uint32_t *n_out)
{
    if (check_pars(pars) != RAWDTW_OK || !n_out || (n && (!events || !hash_out || !pos_out))) return RAWDTW_ERR_INVALID;
    uint32_t k = 0;
    // (the minimizer sketch can emit an e-mer again when equal hashes share a window; beyond n elements: RAWDTW_ERR_RANGE)
    sketch(*pars, events, n, [&](uint32_t h, uint32_t i) {
        if (k < n) { hash_out[k] = h; pos_out[k] = i; }
        k++;
    });
    *n_out = k;
    return k <= n ? RAWDTW_OK : RAWDTW_ERR_RANGE;
}

// The parallel form of the minimizer sketch, as rawdtw_seed_build.hip runs it: the kept events (k_sb_filter), every e-mer's hash
// (k_sb_hash), then rawdtw_seed_min.h's step for every m on its own (k_sb_min_count / k_sb_min_write).  w == 0 has no window: ri_sketch_reg.
int rawdtw_seed_sketch_windowed(const rawdtw_seed_pars_t *pars, const float *events, uint32_t len, uint32_t *hash, uint32_t *pos, uint32_t cap,
                                uint32_t *n)
{
    if (check_pars(pars) != RAWDTW_OK || !n || (len && !events) || (cap && (!hash || !pos))) return RAWDTW_ERR_INVALID;
    uint32_t k = 0;
    auto put = [&](uint32_t h, uint32_t i) {
        if (k < cap) { hash[k] = h; pos[k] = i; }
        k++;
    };
    if (pars->w == 0) sketch_reg(*pars, events, len, put);
    else {
        const uint32_t e = pars->e, quant_bit = pars->lq + 2;
        const uint64_t mask_events = (1ULL << (quant_bit * e)) - 1;
        std::vector<uint32_t> kept_pos, kept_code, h;
        try {
            float last = len ? events[0] : 0.0f;
            for (uint32_t i = 0; i < len; i++) {
                if (skipped_min(events[i], last, i == 0)) continue;
                last = events[i];
                kept_pos.push_back(i);
                kept_code.push_back(code_of(bits_of(events[i]), pars->q, pars->lq));
            }
            const uint32_t M = kept_pos.size() >= e ? (uint32_t)kept_pos.size() - e + 1 : 0;
            h.resize(M);
            for (uint32_t m = 0; m < M; m++) {
                uint64_t quant = 0;
                for (uint32_t a = 0; a < e; a++) quant = quant << quant_bit | kept_code[m + a];
                h[m] = hash32((uint32_t)(quant & mask_events));
            }
            for (uint32_t m = 0; m < M; m++)
                min_step_walk(MinHashes{h.data(), 0}, m, M, pars->w, [&](uint32_t i) { put(h[i], kept_pos[i]); });
        } catch (const std::bad_alloc &) { return RAWDTW_ERR_OOM; }
    }
    *n = k;
    return k <= cap ? RAWDTW_OK : RAWDTW_ERR_RANGE;
}

int rawdtw_seed_hits_host(const rawdtw_seed_index *six, uint32_t n_chunks, const uint64_t *event_off, const float *events, uint64_t *hit_off,
                          rawdtw_seed_hit_t *hits, uint64_t hits_cap, int threads)
{
    if (!six || !hit_off || (n_chunks && !event_off)) return RAWDTW_ERR_INVALID;
    if (six->resident) return RAWDTW_ERR_UNSUPPORTED; // (rawdtw_seed_index_fetch first)
    for (uint32_t k = 0; k < n_chunks; k++)
        if (event_off[k + 1] < event_off[k] || event_off[k + 1] - event_off[k] > 0xffffffffull) return RAWDTW_ERR_INVALID;
    if (n_chunks && event_off[n_chunks] > event_off[0] && !events) return RAWDTW_ERR_INVALID;
    const int T = std::max(1, std::min({threads, 256, (int)std::max<uint32_t>(n_chunks, 1)}));
    // two passes over the sketch, as the detection counts before it writes: the chunks' totals, then the hits at their offsets
    std::vector<uint64_t> count;
    try { count.assign(n_chunks, 0); } catch (const std::bad_alloc &) { return RAWDTW_ERR_OOM; }
    auto each_chunk = [&](auto body) {
        std::atomic<uint32_t> next{0};
        capi::parallel_for(T, [&](int) {
            for (uint32_t k; (k = next.fetch_add(1)) < n_chunks;) body(k);
        });
    };
    each_chunk([&](uint32_t k) {
        uint64_t c = 0;
        sketch(six->pars, events + event_off[k], (uint32_t)(event_off[k + 1] - event_off[k]), [&](uint32_t h, uint32_t) {
            if (const Slot *s = find(six, h)) c += s->count;
        });
        count[k] = c;
    });
    hit_off[0] = 0;
    for (uint32_t k = 0; k < n_chunks; k++) hit_off[k + 1] = hit_off[k] + count[k];
    if (hit_off[n_chunks] > hits_cap) return RAWDTW_ERR_RANGE;
    if (hit_off[n_chunks] && !hits) return RAWDTW_ERR_INVALID;
    each_chunk([&](uint32_t k) {
        rawdtw_seed_hit_t *o = hits + hit_off[k];
        sketch(six->pars, events + event_off[k], (uint32_t)(event_off[k + 1] - event_off[k]), [&](uint32_t h, uint32_t i) {
            const Slot *s = find(six, h);
            if (!s) return;
            const uint64_t *y = s->count == 1 ? &s->val : six->pos.data() + s->val;
            for (uint32_t t = 0; t < s->count; t++) // rmap.cpp:385-389
                *o++ = rawdtw_seed_hit_t{(uint32_t)(y[t] >> 32), (int32_t)(y[t] & 1), (uint32_t)(y[t] >> 1) & 0x7fffffffu, i};
        });
    });
    return RAWDTW_OK;
}

} // extern "C"
