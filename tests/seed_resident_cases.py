"""Inputs of the resident seed index (rawdtw_seed_index_build_resident, rawdtw_seed_table_from_entries), shared by
tests/test_seed_resident_cpu.py and tests/test_seed_resident_gpu.py: strands at the tiled filter's edges, one strand past the launches'
grid-stride cap, entry lists whose hashes are crafted to meet in chosen slots, and a Python restatement of the kept-event recurrence under
both rules that shares nothing with the library.  Everything is seeded; nothing here reads the reference."""
import functools

import numpy as np

from tests import seed_build_min_cases as bc
from tests import seed_cases as sc

TILE = 2048      # rawdtw_seed_tile.h: kFilterTile, the events of a tile
GRID_Y = 1024    # rawdtw_seed_build.hip: kTileGridY, the blocks a strand in k_sb_next / k_sb_mark; a strand of more tiles takes the grid-stride loop
SEED = 20261101
MASK, DIFF = sc.MASK_SIGNAL, sc.DIFF
MULT = 2654435761                     # rawdtw_seed.h: first_slot's multiplier; odd, so every home slot has hashes
INVERSE = pow(MULT, -1, 2 ** 32)


# ---- the recurrence ---------------------------------------------------------------------------------------------------------------------
def kept_events(ev, masked: bool):
    """rsketch.c:243 (masked: the w = 0 rule, which also skips RI_MASK_SIGNAL) or :172: the indices of the kept events.  The float32
    difference is taken in double -- exact for values of like size -- and rounded to float32 only where it decides: next to 0.3."""
    x = np.asarray(ev, np.float32)
    xs = x.astype(np.float64).tolist()
    kept, D, M = [], float(DIFF), float(MASK)
    last, last32 = (xs[0], x[0]) if xs else (0.0, np.float32(0))
    for i, v in enumerate(xs):
        if i > 0:
            a = abs(v - last)
            if abs(a - D) < 1e-5:
                a = float(abs(np.float32(x[i] - last32)))
            if a < D:          # (a NaN is not below anything: kept)
                continue
        if masked and v == M:
            continue
        kept.append(i)
        last, last32 = v, x[i]
    return np.array(kept, np.int64)


def kept_and_entries(fwd, rev, p):
    """(kept events over all strands, entries of the w = 0 sketch): what the build's statistics say.  With w > 0 the entries are the
    windows' choice and None here."""
    kept = [len(kept_events(x, p.w == 0)) for pair in zip(fwd, rev) for x in pair]
    return sum(kept), (sum(max(k - p.e + 1, 0) for k in kept) if p.w == 0 else None)


# ---- strands at the tiles' edges ----------------------------------------------------------------------------------------------------------
def all_kept(n, rng):
    """n events, neighbours 2 or more apart: every event kept; the values vary, so the e-mers' hashes do"""
    x = np.where(np.arange(n) % 2 == 0, np.array([-4, -2, -1], np.float32)[rng.integers(0, 3, n)], np.array([1, 2, 4], np.float32)[rng.integers(0, 3, n)])
    return x.astype(np.float32)


def shape_strands():
    """[(name, events)]: the CPU program's list at the real tile size"""
    rng = np.random.default_rng(SEED)
    T = TILE
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    out = []
    for n in (T + 1, 0, 2 * T + 1, 1, T - 1, T):   # (the empty ones lie between two long ones)
        out.append(("all_kept_%d" % n, all_kept(n, rng)))
        out.append(("flat_%d" % n, np.full(n, 1.25, np.float32)))
    x = all_kept(3 * T + 40, rng)
    x[T // 2:T // 2 + 2 * T + 9] = 4.0 + 0.0001 * (np.arange(2 * T + 9) % 1000)   # a flat stretch longer than two whole tiles, drifting
    out.append(("flat_stretch", x.astype(np.float32)))
    for name, at in (("kept_at_last", 2 * T - 1), ("kept_at_first", T)):
        x = np.full(3 * T, 2.0, np.float32)
        x[at] = 5.0
        out.append((name, x))
    for sname, special in (("nan", nan), ("pinf", inf), ("ninf", -inf), ("mask", MASK)):
        for where in range(8):
            x = np.full(2 * T + 3, 0.5, np.float32) if where & 4 else all_kept(2 * T + 3, rng)
            if where & 1:
                x[T - 1] = special
            if where & 2:
                x[T] = special
            if where & 3 == 0:
                x[[0, 2 * T - 1, 2 * T, 2 * T + 2]] = special   # position 0, both sides of the second boundary, the strand's end
            if where & 3 == 3:
                x[T + 1] = special
            out.append(("%s_%d" % (sname, where), x))
    x = bc.LEVELS[rng.integers(0, 4, 2 * T + 300)].copy()   # the tie alphabet: equal neighbours are skipped, chains of every length
    out.append(("alphabet", x))
    x = np.cumsum(rng.normal(0, 0.12, 3 * T)).astype(np.float32)   # a slow walk: each event against the last KEPT one, tiles apart
    out.append(("walk", x))
    return out


@functools.lru_cache(maxsize=1)
def shape_reference():
    """(forward arrays, reverse arrays, names): every shape as a forward array beside a filler, then as a reverse array; an empty sequence
    lies between two long ones (all_kept_0 and flat_0 behind flat_T+1, in front of all_kept_2T+1)"""
    rng = np.random.default_rng(SEED + 1)
    shapes = shape_strands()
    filler = [all_kept(len(x), rng) if i % 2 else np.full(len(x), -3.0, np.float32) for i, (_, x) in enumerate(shapes)]
    fwd = [x for _, x in shapes] + filler
    rev = filler + [x for _, x in shapes]
    return fwd, rev, [n for n, _ in shapes]


@functools.lru_cache(maxsize=1)
def long_strand_reference():
    """one sequence of more than GRID_Y tiles: tiles all kept and flat by turns (a flat tile's first event is kept, the rest skipped);
    the reverse array is the same pattern half a tile on, so that its runs begin and end inside tiles"""
    rng = np.random.default_rng(SEED + 2)
    n = (GRID_Y + 6) * TILE + 77
    x = all_kept(n, rng)
    tile = np.arange(n) // TILE
    flat = tile % 2 == 1
    x[flat] = 0.25 + 0.0001 * (tile[flat] % 7)
    y = np.roll(x, TILE // 2 + 5)
    return [x], [y.copy()]


# ---- entries with chosen hashes -----------------------------------------------------------------------------------------------------------
def log2_slots(n_keys):
    lg = 4
    while (1 << lg) < 2 * n_keys:
        lg += 1
    return lg


def hash_at(home, lg, low):
    """a hash whose probe sequence starts at slot `home` of a table of 1 << lg slots; `low` picks among those that share it"""
    return ((int(home) << (32 - lg) | (int(low) & ((1 << (32 - lg)) - 1))) * INVERSE) & 0xFFFFFFFF


def first_slot(h, lg):
    return ((int(h) * MULT) & 0xFFFFFFFF) >> (32 - lg)


def sequential_layout(hashes):
    """(the keys in table order, the keys not in their home slot) after inserting the distinct hashes in ascending order, each into the
    first free slot from its home on"""
    keys = np.unique(np.asarray(hashes, np.uint32)).tolist()
    lg = log2_slots(len(keys))
    tab, away = [None] * (1 << lg), 0
    for h in keys:
        at = first_slot(h, lg)
        away += tab[at] is not None
        while tab[at] is not None:
            at = (at + 1) & ((1 << lg) - 1)
        tab[at] = h
    return [h for h in tab if h is not None], away


def entries(groups):
    """{hash: [y, ...]} -> (hashes, ys) sorted by (hash, y)"""
    hs = np.array([h for h, ys in groups.items() for _ in ys], np.uint32)
    ys = np.array([y for _, ys in groups.items() for y in ys], np.uint64)
    order = np.lexsort((ys, hs))
    return hs[order], ys[order]


def pos(seq, p, strand):
    return seq << 32 | p << 1 | strand


def table_cases():
    """[(name, hashes, ys)]: the small tables: the sizes at fill_table's edges, lists, one home slot, a cluster across the table's end"""
    rng = np.random.default_rng(SEED + 3)
    out = [("empty", np.zeros(0, np.uint32), np.zeros(0, np.uint64))]
    out.append(("one",) + entries({0xDEADBEEF: [pos(0, 7, 1)]}))
    for n in (8, 9):   # (the lg 4 -> 5 edge)
        out.append(("keys_%d" % n,) + entries({int(h): [pos(0, i, i & 1)] for i, h in enumerate(rng.choice(2 ** 32, n, replace=False))}))
    out.append(("all_single",) + entries({int(h): [pos(i % 3, i, 0)] for i, h in enumerate(rng.choice(2 ** 32, 300, replace=False))}))
    out.append(("one_key",) + entries({12345: [pos(s, i, i & 1) for s in range(3) for i in range(500)]}))
    g = {int(h): [pos(0, i, 1)] for i, h in enumerate(rng.choice(2 ** 32, 20, replace=False))}
    g[0x80000001] = [pos(1, 5, 0), pos(0, 9, 1)]
    out.append(("list_of_2",) + entries(g))
    lg = log2_slots(200)
    g = {hash_at(5, lg, i * 7919 + 1): [pos(0, i, 0)] + ([pos(1, i, 1)] if i % 5 == 0 else []) for i in range(200)}   # 200 keys on one home slot
    assert len(g) == 200 and all(first_slot(h, lg) == 5 for h in g)
    out.append(("one_home",) + entries(g))
    lg = log2_slots(40)
    last = (1 << lg) - 1
    g = {hash_at(last, lg, i * 104729 + 3): [pos(0, i, 0)] for i in range(12)}           # a cluster across the table's end ...
    g.update({hash_at(last - 2, lg, i * 31 + 1): [pos(0, 100 + i, 1), pos(2, i, 0)] for i in range(10)})
    g.update({hash_at(i % 4, lg, i * 977 + 5): [pos(1, i, 0)] for i in range(18)})       # ... past keys whose home is the table's start
    assert len(g) == 40
    out.append(("wraps",) + entries(g))
    return out


@functools.lru_cache(maxsize=1)
def big_table():
    """1.2 M keys with random hashes (2^22 slots, load 0.29: probe sequences of many waves run into one another), every tenth key with a
    list of 2 to 4"""
    rng = np.random.default_rng(SEED + 4)
    keys = np.unique(rng.integers(0, 2 ** 32, 1_250_000, dtype=np.uint64).astype(np.uint32))[:1_200_000]
    count = np.where(np.arange(len(keys)) % 10 == 0, 1 + rng.integers(1, 4, len(keys)), 1)
    hs = np.repeat(keys, count)
    ys = np.arange(len(hs), dtype=np.uint64) << np.uint64(1)   # (ascending inside every group)
    return hs, ys
