// rawdtw_seed_layout.h -- where a seeding's arrays lie in its two grow-only blocks (rawdtw_seed.hip): the device block and the
// page-locked host block, as byte offsets from (kind, n chunks, N events, w > 0).  No HIP include: a plain compiler takes it
// (tests/abi/seed_layout.cpp).  seed_enqueue is the one consumer; DESIGN.md 4.10 says what the three kinds are.
//
//   device region      bytes (each rounded up to 256)   plain      resident   detected
//   off    dense event offsets       (n + 1) * 8        uploaded   uploaded   copied from the detection
//   src    source starts (arena)     (n + 1) * 8        -          uploaded   copied from the detection
//   ev     the events                N * 4              uploaded   -          -         (resident kinds read the event arena)
//   code pos cnt  per event          N * 4 each         x          x          x
//   val    per event                 N * 8              x          x          x
//   kept   per chunk                 n * 4              x          x          x
//   chits hoff                       (n + 1) * 8 each   x          x          x
//   tot    [0] total [1] overflow    32                 x          x          x
//   hash spos  the sketch, w > 0     N * 4 each         w > 0      w > 0      w > 0
//   count  the sketch, w > 0         n * 4              w > 0      w > 0      w > 0
// 24 bytes an event (32 with w > 0), as include/rawdtw.h says.
//   pinned region (8-byte words)                        plain      resident   detected
//   tot over   one word each, words 0 and 1             come home  come home  over alone comes home
//   off    n + 1 words from word 2                      goes up    goes up    -
//   src    n words, n + 1 words behind off              -          goes up    -
//   hoff   n + 1 words, 2 (n + 1) words behind off      -          comes home comes home
//   decl   the detection's flag word, behind hoff       -          -          comes home
// A region the kind does not use has `bytes` 0 (its `at` is where the next one starts).
#pragma once
#include "rawdtw_layout.h"

namespace rawdtw {
namespace seed {

enum class Kind { plain, resident, detected };

using ws::Region;
using ws::al;

struct Layout {
    Region off, src, ev, code, pos, cnt, val, kept, chits, hoff, tot, hash, spos, count; // the device block, in this order
    size_t need = 0;
    Region p_tot, p_over, p_off, p_src, p_hoff, p_decl; // the pinned block
    size_t pin_need = 0;
};

inline Layout layout(Kind kind, uint64_t n, uint64_t N, bool sketch)
{
    const bool plain = kind == Kind::plain;
    const size_t b_off = al((n + 1) * 8), b_ev = al(N * 4), b_val = al(N * 8), b_cnt = al(n * 4), b_tot = al(32);
    Layout L;
    ws::Take take;
    L.off = take(b_off); L.src = take(plain ? 0 : b_off); L.ev = take(plain ? b_ev : 0);
    L.code = take(b_ev); L.pos = take(b_ev); L.cnt = take(b_ev); L.val = take(b_val);
    L.kept = take(b_cnt); L.chits = take(b_off); L.hoff = take(b_off); L.tot = take(b_tot);
    L.hash = take(sketch ? b_ev : 0); L.spos = take(sketch ? b_ev : 0); L.count = take(sketch ? b_cnt : 0);
    L.need = take.p;
    const size_t row = (n + 1) * 8;
    L.p_tot = Region{0, 8}; L.p_over = Region{8, 8};
    L.p_off = Region{16, kind == Kind::detected ? 0 : row};
    L.p_src = Region{16 + row, kind == Kind::resident ? n * 8 : 0};
    L.p_hoff = Region{16 + 2 * row, plain ? 0 : row};
    L.p_decl = Region{16 + 3 * row, kind == Kind::detected ? (size_t)8 : 0};
    L.pin_need = plain ? (n + 3) * 8 : (3 * (n + 1) + 4) * 8;
    return L;
}

} // namespace seed
} // namespace rawdtw
