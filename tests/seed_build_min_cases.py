"""Inputs of the minimizer table's device build (rawdtw_seed_index_build_device_min) and of its host restatement
(rawdtw_seed_sketch_windowed), shared by tests/test_seed_build_min_cpu.py and tests/test_seed_build_min_gpu.py: whole strands over the
tie alphabets of tests/seed_min_cases.py, strands at the window's and the tile's edges, and a numpy / Python restatement of the e-mers'
hashes and of the step's five rules that shares nothing with the library.  Everything is seeded; nothing here reads the reference."""
import functools

import numpy as np

from tests import seed_cases as sc
from tests import seed_min_cases as smc

LEVELS, all_kept, motif = smc.LEVELS, smc.all_kept, sc.motif
MASK_SIGNAL = sc.MASK_SIGNAL
SEED = 20261020
TILE = 256                                     # rawdtw_seed_build.hip: kMinTile, the e-mers a workgroup takes at a time
GRID_Y = 1024                                  # ... and `gy = min(tiles, 1024)`: a strand of more tiles takes the grid-stride loop
ALPHABETS = (2, 3, 4, 8)
RANDOM_W = (1, 2, 3, 5, 16, 63, 64, 65, 255)   # the host test's windows
RANDOM_E = (2, 6, 9)
RANDOM_STRANDS = 2000
DEVICE_W = (1, 2, 5, 63, 64, 65, 255)          # the device test's
BOUNDARY_W = (5, 16)                           # boundary_strand's: a minimum that lives w steps among few hash values needs a small w


def distinct_neighbours(n, a, rng):
    """n events over LEVELS[:a], no two neighbours equal: neighbours are 0.5 or more apart, so every event is kept and e-mer m begins
    at event m -- while the e-mers' hashes take few values, so windows are full of ties"""
    idx = np.zeros(n, np.int64)
    if n:
        idx[0] = rng.integers(0, a)
        step = rng.integers(1, a, n)   # (1 .. a - 1: never 0)
        for i in range(1, n):
            idx[i] = (idx[i - 1] + step[i]) % a
    x = LEVELS[idx]
    assert n < 2 or np.abs(np.diff(x)).min() >= 0.5
    return x


def kept_events(ev):
    """ri_sketch_min's filter (rsketch.c:172): the indices of the kept events.  No RI_MASK_SIGNAL clause; a NaN is kept."""
    ev = np.asarray(ev, np.float32)
    kept, last = [], 0
    for i in range(len(ev)):
        if i > 0 and abs(np.float32(ev[i] - ev[last])) < sc.DIFF:
            continue
        kept.append(i)
        last = i
    return np.array(kept, np.int64)


def emer_hashes(ev, p):
    """(hash of every e-mer, position of its first kept event) under ri_sketch_min's filter: numpy integers only"""
    ev = np.asarray(ev, np.float32)
    kept = kept_events(ev)
    M = len(kept) - p.e + 1
    if M <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    bits = ev.view(np.uint32).astype(np.uint64)[kept]
    code = (bits >> np.uint64(30) << np.uint64(p.lq)) | ((bits >> np.uint64(32 - p.q)) & np.uint64((1 << p.lq) - 1))
    qb, m32 = p.lq + 2, np.uint64(0xFFFFFFFF)
    k = np.zeros(M, np.uint64)
    for j in range(p.e):
        k = (k << np.uint64(qb)) | code[j:j + M]
    if qb * p.e < 64:
        k &= np.uint64((1 << (qb * p.e)) - 1)
    k &= m32   # hash64 with the 32-bit mask (rsketch.c:6-15)
    k = (~k + (k << np.uint64(21))) & m32
    k ^= k >> np.uint64(24)
    k = (k + (k << np.uint64(3)) + (k << np.uint64(8))) & m32
    k ^= k >> np.uint64(14)
    k = (k + (k << np.uint64(2)) + (k << np.uint64(4))) & m32
    k ^= k >> np.uint64(28)
    k = (k + (k << np.uint64(31))) & m32
    return k, kept[:M]


def newest_min(h, m, w):
    """S(m): the newest index among max(0, m - w + 1) .. m that carries the smallest hash"""
    lo = max(0, m - w + 1)
    win = h[lo:m + 1]
    return m - int(np.argmin(win[::-1]))


def step_rules(h, m, M, w):
    """what step m emits, as [(e-mer index, rule)] in order: the issue's five rules, written from its text"""
    out = []
    prev = newest_min(h, m - 1, w) if m > 0 else None
    if prev is not None and m + 1 == w:
        out += [(i, 1) for i in range(m) if h[i] == h[prev] and i != prev]
    if prev is None or h[m] <= h[prev]:
        if prev is not None and m >= w:
            out.append((prev, 2))
    elif m - prev == w:
        out.append((prev, 3))
        now = newest_min(h, m, w)
        out += [(i, 30) for i in range(m - w + 1, m + 1) if h[i] == h[now] and i != now]   # (30: rule 3's tie list)
    if m + 1 == M:
        out.append((newest_min(h, m, w), 5))
    return out


def random_strand(it):
    """strand `it` of the host test's RANDOM_STRANDS: (events, a, w, e); the 108 combinations of (a, w, e) take turns.  A combination's
    even turns are uniform draws of 0 .. 700 events (equal neighbours are dropped by the filter); its odd turns have distinct neighbours
    and, for w <= 16, a length that walks the e-mer count M through 0 .. w + 2 over the combinations that share the w -- so every M in
    0 .. w + 1 occurs for every small w -- and for larger w anything up to 700 events."""
    rng = np.random.default_rng(SEED + it)
    combos = len(ALPHABETS) * len(RANDOM_W) * len(RANDOM_E)
    combo, rnd = it % combos, it // combos
    a = ALPHABETS[combo % 4]
    w = RANDOM_W[(combo // 4) % len(RANDOM_W)]
    e = RANDOM_E[combo // (4 * len(RANDOM_W))]
    if rnd % 2 == 0:
        return LEVELS[rng.integers(0, a, int(rng.integers(0, 701)))], a, w, e
    turn = (rnd // 2) * 12 + combo % 4 + 4 * (combo // (4 * len(RANDOM_W)))   # counts the odd turns of this w over its 12 (a, e)
    M = turn % (w + 3) if w <= 16 else int(rng.integers(0, 701 - e + 1))
    n = M + e - 1 if M else int(rng.integers(0, e))
    return distinct_neighbours(min(n, 700), a, rng), a, w, e


def alphabet_reference(a, seed=0):
    """(forward arrays, reverse arrays): the tie alphabet LEVELS[:a] as whole strands of five sequences, an empty one and a one-event
    one among them; the long ones reach past two tiles"""
    rng = np.random.default_rng(SEED + 1000 * a + seed)
    lens = (700, 0, 300, 1, 2 * TILE + 90)
    fwd = [LEVELS[rng.integers(0, a, n)] if s % 2 == 0 else distinct_neighbours(n, a, rng) for s, n in enumerate(lens)]
    rev = [distinct_neighbours(n, a, rng) if s % 2 == 0 else LEVELS[rng.integers(0, a, n)] for s, n in enumerate(lens)]
    return fwd, rev


def edge_reference(w, e, a=3):
    """strands whose every event is kept, so that a strand of n events has exactly max(n - e + 1, 0) e-mers: e-mer counts 0, 1, w - 1, w,
    w + 1, TILE - 1, TILE, TILE + 1 and 2 TILE + 1, strands with fewer events than e, and an empty sequence between two long ones.
    Forward arrays over the tie alphabet, reverse arrays of far-apart real values (hashes all but distinct)."""
    rng = np.random.default_rng(SEED + 7 * w + e)
    Ms = [2 * TILE + 1, 0, TILE + 1, 1, max(w - 1, 0), w, w + 1, TILE - 1, TILE]
    lens = [M + e - 1 for M in Ms]
    lens[1] = 0                       # the empty sequence, between the two longest
    lens += [e - 1, 1, e - 2]         # fewer kept events than e
    fwd = [distinct_neighbours(n, a, rng) for n in lens]
    rev = [all_kept(n, rng) for n in lens]
    return fwd, rev, [max(n - e + 1, 0) for n in lens]


def leaves_at(h, m, w):
    """the minimum leaves the window exactly at e-mer m, and the new minimum's hash is carried by e-mer m and by an older one of the
    new window: rule 3 with a tie list that reaches across m - 1 | m"""
    if m < w:
        return False
    prev = newest_min(h, m - 1, w)
    if m - prev != w or not h[m] > h[prev]:
        return False
    new = h[m - w + 1:m + 1]
    return bool(h[m] == new.min() and np.any(new[:-1] == new.min()))


@functools.lru_cache(maxsize=None)
def boundary_strand(w, e=2, a=3, tile=TILE):
    """an all-kept strand (e-mer index == event index) in which leaves_at holds at e-mer `tile`, a tile's first: cut from a long random
    one at the first place where the property holds"""
    from rawalign_amd.seeding import SeedParams

    rng = np.random.default_rng(SEED + 31 * w)
    x = distinct_neighbours(20000, a, rng)
    h, pos = emer_hashes(x, SeedParams(w=w, e=e))
    assert np.array_equal(pos, np.arange(len(h)))
    for m in range(tile, len(h) - tile):
        if leaves_at(h, m, w):
            return x[m - tile:m + tile + 40].copy()
    raise AssertionError("no such place")
