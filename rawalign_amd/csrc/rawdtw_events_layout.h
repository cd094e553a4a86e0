// rawdtw_events_layout.h -- where a detection's arrays lie in its two grow-only blocks (rawdtw_events.hip): the device block and the
// page-locked host block, as byte offsets from (raw, arena, n chunks, N samples -- raw samples for a raw detection).  No HIP include: a
// plain compiler takes it (tests/abi/events_layout.cpp).  detect_enqueue lays the blocks out, the two ends and detect_resident_view
// (which rawdtw_seed.hip reads: eoff, dst and the flag word of tot) find their words through the same struct.
//
//   device region      bytes (each rounded up to 256)            float    raw      resident (arena) adds
//   off    the chunks' sample offsets       (n + 1) * 8          uploaded scanned
//   sig    the pA samples                   N * 4                uploaded compacted
//   ps pss prefix sums, chunk k from off[k] + k   (N + n) * 4 each   x    x
//   t1 t2  the t-statistics                 N * 4 each           x        x
//   peaks  chunk k's slots from off[k]      N * 4                x        x
//   npk nev  per chunk                      n * 4 each           x        x
//   eoff   dense event offsets              (n + 1) * 8          x        x
//   tot    kTotEvents kTotSamples kTotFlag  32                   x        x
//   ev     the events, at eoff              N * 4                x        x        (reserved, not written: they go to the arena)
//   raw    the int16 samples as they came   N * 2 + 16           -        uploaded (8 more samples: the last window's last load)
//   roff   the windows' raw offsets         (n + 1) * 8          -        uploaded
//   chan   a channel a window               n * sizeof(rawdtw_channel_t)  -   uploaded
//   slen   kept samples a window            n * 4                -        x
//   dst    the chunks' places in the arena  (n + 1) * 8          -        -        uploaded (n words are used)
//   room   ... and their room               n * 4                -        -        uploaded
// sig, ps, pss, t1, t2, peaks, ev: 28 bytes a sample (30 a raw sample), as include/rawdtw.h says.
//   pinned region (8-byte words)                                 plain             resident
//   tot    word 0: the events' total                             comes home        comes home
//   flag   word 1: kTotFlag's word                               -                 comes home
//   off    n + 1 words, rebased to 0                             from word 1, up   from word 2, up
//   dst    n words behind off                                    -                 goes up
//   room nev cnt   n uint32 each behind dst                      -                 room goes up; nev, and a raw one's cnt (s_len), come home
// A region the kind does not use has `bytes` 0 (its `at` is where the next one starts).
#pragma once
#include "rawdtw_layout.h"

#include "../../include/rawdtw.h"

namespace rawdtw {
namespace events {

using ws::Region;

// the words of `tot`
enum : uint32_t {
    kTotEvents = 0,  // the total of events (k_ev_scan over nev)
    kTotSamples = 1, // a raw detection: the total of kept samples (k_ev_scan over slen), which the host never sees
    kTotFlag = 2,    // a resident detection: bit 0 a chunk over its room, bit 1 the total over events_cap (k_ev_room)
};

struct Layout {
    Region off, sig, ps, pss, t1, t2, peaks, npk, nev, eoff, tot, ev, raw, roff, chan, slen, dst, room; // the device block, in this order
    size_t need = 0;
    Region p_tot, p_flag, p_off, p_dst, p_room, p_nev, p_cnt; // the pinned block, in this order
    size_t pin_need = 0;
};

inline Layout layout(bool raw, bool arena, uint64_t n, uint64_t N)
{
    using ws::al;
    const size_t b_off = al((n + 1) * 8), b_t = al(N * 4), b_ps = al((N + n) * 4), b_cnt = al(n * 4);
    Layout L;
    ws::Take take;
    L.off = take(b_off); L.sig = take(b_t); L.ps = take(b_ps); L.pss = take(b_ps);
    L.t1 = take(b_t); L.t2 = take(b_t); L.peaks = take(b_t);
    L.npk = take(b_cnt); L.nev = take(b_cnt); L.eoff = take(b_off); L.tot = take(al(32)); L.ev = take(b_t);
    L.raw = take(raw ? al(N * 2 + 16) : 0); L.roff = take(raw ? b_off : 0);
    L.chan = take(raw ? al(n * sizeof(rawdtw_channel_t)) : 0); L.slen = take(raw ? b_cnt : 0);
    L.dst = take(arena ? b_off : 0); L.room = take(arena ? b_cnt : 0);
    L.need = take.p;
    ws::Take pin;
    L.p_tot = pin(8); L.p_flag = pin(arena ? 8 : 0); L.p_off = pin((n + 1) * 8);
    L.p_dst = pin(arena ? n * 8 : 0); L.p_room = pin(arena ? n * 4 : 0); L.p_nev = pin(arena ? n * 4 : 0);
    L.p_cnt = pin(raw && arena ? n * 4 : 0);
    L.pin_need = arena ? (4 * n + 4) * 8 : (n + 2) * 8; // (a resident float detection reserves cnt's words too)
    return L;
}

} // namespace events
} // namespace rawdtw
