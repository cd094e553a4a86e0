"""Planted paths: signals whose optimal warping path is known by construction, a model of the window through which the banded walk
(k_band_tb_walk, rawalign_amd/csrc/rawdtw_band_tb.hip) reads its directions, and the job lists built from both.

planted(moves) -> (a, b) for a string over D, V, H.  Both signals start at level 0 and hold integers: D raises the level by 3 and
appends it to a and to b; V appends the current level to a alone (the path moves i + 1); H appends it to b alone (j + 1).  With at
least one D between a V run and an H run every level is one column segment, one row segment or a single cell, so the cells of distance
0 are exactly the planted path: it is the unique optimum and costs 0.0f, every other path costs 3 or more.  A walk that reads one
wrong direction code leaves it.

The window model restates, from the layout in rawdtw_band_tb.h alone, the records k_band_tb_fill writes an antidiagonal sum
(si + ds, sj - ds, lo + ds, hi + ds) and the rule by which k_band_tb_walk (re)loads 128 slots of 64 rows.  It is used to show what a
case list reaches -- chunks, band edges, kinds of window load -- and never as a yardstick for a device result.

A drift reload on the high side (the slot passes 64 row_c + 127 before 64 sums have passed) cannot happen: a load puts the slot at
most at 64 row_c + 95 and a slot number rises by at most one an antidiagonal sum, so 64 sums end the window first; the model counts
the event all the same and the tests assert that the count is 0."""
import functools
import re

import numpy as np

from tests import banded_tb_cases as bc

STEP = 3.0  # a D raises the level by this much


def moves(spec):
    """"D40 V140 D" -> "D" * 40 + "V" * 140 + "D"; blanks are ignored"""
    spec = spec.replace(" ", "")
    assert re.fullmatch(r"([DVH]\d*)*", spec), spec
    return "".join(letter * (int(count) if count else 1) for letter, count in re.findall(r"([DVH])(\d*)", spec))


def transposed(mv):
    return mv.translate(str.maketrans("VH", "HV"))


def separated(mv):
    """no V run touches an H run"""
    return "VH" not in mv and "HV" not in mv


def planted(mv):
    """-> (a, b), float32 and integer-valued"""
    assert separated(mv) and set(mv) <= set("DVH")
    a, b, level = [0.0], [0.0], 0.0
    for c in mv:
        if c == "D":
            level += STEP
        if c != "H":
            a.append(level)
        if c != "V":
            b.append(level)
    return np.array(a, np.float32), np.array(b, np.float32)


def path_of(mv):
    """-> (i, j), uint32, start first: (0, 0) and one element a move"""
    c = np.frombuffer(mv.encode(), np.uint8)
    i = np.concatenate([[0], np.cumsum(c != ord("H"))]).astype(np.uint32)
    j = np.concatenate([[0], np.cumsum(c != ord("V"))]).astype(np.uint32)
    return i, j


# ---- the band's records and the walk's window ---------------------------------------------------------------------------------------
def band_records(n, m, r0):
    """-> (K, rec): rec[s] = (si, sj, lo, hi) of antidiagonal sum s = I + J, in SLOTS: slot x is the cell (I, J) = (si - x, sj + x), I
    indexing the longer sequence, and the cell was evaluated iff lo <= x < hi"""
    N, M = max(n, m), min(n, m)
    R = bc.slanted_radius(n, m, r0)
    P, S = R + (1 if R % 2 == 0 else 0), R + (1 if R % 2 == 1 else 0)
    K, SH = max(P, S), (0 if P > S else 1)
    rec = np.zeros((n + m - 1, 4), np.int64)
    seen = np.zeros(n + m - 1, bool)
    c = P // 2 + SH
    rec[0], seen[0] = (c, -c, c, c + 1), True
    row = rem = 0
    for col in range(1, N):
        rem += M
        adv = rem >= N
        if adv:
            rem -= N
            row += 1
        for pas in ((0, 1) if adv else (1,)):
            ln = S if pas == 0 else P
            si = col + S // 2 - 1 if pas == 0 else col + P // 2
            sj = row - S // 2 if pas == 0 else row - P // 2
            lo, hi = max(0, si - N + 1, -sj), min(ln, si + 1, M - sj)
            ds = 1 if SH == 1 and pas == 1 else 0
            s = si + sj
            assert not seen[s]
            rec[s], seen[s] = (si + ds, sj - ds, lo + ds, hi + ds), True
    assert seen.all() and K == R + 1
    return K, rec


def walk_window(n, m, r0, pi, pj):
    """the window of k_band_tb_walk on the path (pi, pj) (start first, last element included) of a job (n, m, r0) -> dict:
      K, chunks          the band's width in slots and in 64-slot chunks
      inside             every cell of the path lies in the band
      slot_min/slot_max  the smallest and largest slot visited
      loads              window loads;  loads_first: with row_c = 0 chosen because x < 32;  loads_last: with row_c + 1 == chunks
      second             steps whose code came from the window's second chunk
      drift_low/_high    reloads because the slot left the 128 slots before 64 sums had passed
      chunks_read        the chunk indices some step's code was read from"""
    K, rec = band_records(n, m, r0)
    chunks = (K + 63) // 64
    swapped = n < m
    out = dict(K=K, chunks=chunks, inside=True, slot_min=K, slot_max=-1, loads=0, loads_first=0, loads_last=0, second=0, drift_low=0,
               drift_high=0, chunks_read=set())
    row_s, row_c = -1, 0
    for i, j in zip(pi[::-1].tolist(), pj[::-1].tolist()):
        s, I = i + j, (j if swapped else i)
        si, sj, lo, hi = rec[s]
        x = int(si) - I
        if not lo <= x < hi:
            out["inside"] = False
            break
        out["slot_min"], out["slot_max"] = min(out["slot_min"], x), max(out["slot_max"], x)
        if i == 0 or j == 0:   # the border rules read no code
            continue
        fresh = s > row_s or row_s - s >= 64
        if fresh or x < 64 * row_c or x >= 64 * row_c + 128:
            if not fresh:
                out["drift_low" if x < 64 * row_c else "drift_high"] += 1
            row_s, row_c = s, ((x - 32) >> 6 if x >= 32 else 0)
            out["loads"] += 1
            out["loads_first"] += x < 32
            out["loads_last"] += row_c + 1 == chunks
        xx = x - 64 * row_c
        assert 0 <= xx < 128 and row_c + (xx >> 6) < chunks
        out["second"] += xx >> 6
        out["chunks_read"].add(row_c + (xx >> 6))
    return out


# ---- the banded case list -----------------------------------------------------------------------------------------------------------
def _slant_moves():
    """a 3 : 1 staircase (two rows a column) with one H run and one V run in it: the band is slanted, and the V run of 300 takes the
    walk (which goes backwards) down by more than 128 slots in fewer than 64 sums"""
    out = []
    for q in range(300):
        out.append("DVV")
        if q == 100:
            out.append("D" + "H" * 100 + "D")
        if q == 200:
            out.append("D" + "V" * 300 + "D")
    return "".join(out)


# name -> (moves, R, the band holds the planted path).  On a square job with even R the path starts in slot R / 2 and a V or H run
# of 2 q moves shifts it by q slots.  The two widest cases run further to the high side than to the low one, because their last chunk
# holds only the slots 1024 .. 1030 and 4096 .. 4100: a path symmetric about the centre that stays in the band's inner part (slots
# 15 .. 1015, 50 .. 4050) never reads a code from it.
BANDED = {
    "three_chunks": (moves("D40 V140 D100 H280 D100 V140 D40"), 150, True),          # 561 x 561, K 151, slots 5 .. 145
    "five_chunks": (moves("D40 V290 D100 H580 D100 V290 D40"), 300, True),           # 861 x 861, K 301, slots 5 .. 295
    "slot_0": (moves("D10 V149 D300 H298 D300 V149 D10"), 150, True),                # 919 x 919, slots 0 .. 149
    "slot_k_1": (moves("D10 V149 D300 H299 D300 V150 D10"), 150, True),              # one move wider: slots 0 .. K - 1 = 150
    "both_edges": (moves("D10 V150 D300 H300 D300 V150 D10"), 150, True),            # two moves wider: 0 .. 150 in both orientations
    "outside": (moves("D10 V151 D300 H301 D300 V150 D10"), 150, False),              # the narrowest that leaves the band (cost 900)
    "one_chunk": (moves("D40 V60 D100 H120 D100 V60 D40"), 63, True),                # 401 x 401, K 64, slots 2 .. 62
    "two_chunks": (moves("D40 V60 D100 H120 D100 V60 D40"), 64, True),               # K 65, the same slots: chunk 1 is never read
    "two_chunks_high": (moves("D40 V60 D100 H124 D100 V64 D40"), 64, True),          # K 65, slots 2 .. 64
    "past_1024": (moves("D50 V1000 D300 H2020 D300 V1020 D50"), 1030, True),         # 2721 x 2721, K 1031, 17 chunks, slots 15 .. 1025
    "past_4096": (moves("D50 V4000 D300 H8094 D300 V4094 D50"), 4100, True),         # 8795 x 8795, K 4101, 65 chunks, slots 50 .. 4097
    "slant": (_slant_moves(), 300, True),                                             # 1205 x 405, K 501, 8 chunks, slots 250 .. 326
}
EVERY_CHUNK = ("three_chunks", "five_chunks", "past_1024", "past_4096")   # (a, b) as given reads a code from every chunk of the band
MODEL_CELLS = 925 * 925   # the numpy model of the definition (banded_tb_cases.model) is run on matrices up to this: all but the two widest


def banded_list():
    """[(name, moves as the job has them, R, holds, exclude_last)]: every case as (a, b) and as (b, a), exclude_last alternating"""
    out = []
    for name, (mv, R, holds) in BANDED.items():
        for mvo in (mv, transposed(mv)):
            out.append((name, mvo, R, holds, len(out) & 1))
    return out


def banded_jobs(entries=None):
    """-> ([(a, b, R, exclude_last)], [(i, j) planted, last element included]) in banded_list's order"""
    cases, paths = [], []
    for name, mv, R, holds, ex in (banded_list() if entries is None else entries):
        a, b = planted(mv)
        cases.append((a, b, R, ex))
        paths.append(path_of(mv))
    return cases, paths


@functools.lru_cache(maxsize=None)
def banded_host_answers():
    """rawdtw_banded_tb_host on banded_jobs(), computed once a process; read-only"""
    import rawalign_amd as ra

    return tuple(ra.banded_tb_host(a, b, R, ex) for a, b, R, ex in banded_jobs()[0])


def expected(path, ex):
    """the planted path as the traceback returns it: exclude_last pops the last element"""
    i, j = path
    return (i[:-1], j[:-1]) if ex else (i, j)


# ---- the full-matrix global walker --------------------------------------------------------------------------------------------------
# a V run of 700 rows over the 512-row strip edge in mid-matrix, an H run of 300 columns in mid-matrix; the shorter side 513 and 1025
GLOBAL = {
    "short_513": moves("D100 V700 D12 H300 D100"),     # 913 x 513
    "short_1025": moves("D200 V700 D224 H300 D300"),   # 1425 x 1025; transposed, its V run of 300 lies over row 512 as well
}


def global_jobs():
    """-> ([(a, b, exclude_last)], [planted (i, j)]): both orientations"""
    cases, paths = [], []
    for mv in GLOBAL.values():
        for mvo in (mv, transposed(mv)):
            cases.append(planted(mvo) + (len(cases) & 1,))
            paths.append(path_of(mvo))
    return cases, paths


# ---- semiglobal traceback and span --------------------------------------------------------------------------------------------------
SEMI_M = 3000
SEMI_OFFSETS = (0, 63, 64, 65, 1000)
# a V run over row 512 and one over row 1024 (n > 1024: the pipelined class), an H run of 200 columns in the middle strip (rows 512..1023).
# Both begin and end with D: row 0 of the matrix is assigned, so the path starts in the column of the planted b's element 0 only if
# the walk does not run along row 0, and the last row's FIRST minimum is the path's end only if the last level is a single cell.
SEMI = {
    "runs_over_512_and_1024": moves("D300 V300 D100 H200 D100 V300 D50"),   # 1151 rows; the planted b has 751 elements
    "short_v_long_d": moves("D400 V160 D40 H200 D200 V300 D100"),           # 1201 rows: V over 400..560, H in row 600, V over 800..1100
}


def semiglobal_jobs():
    """-> ([(a, b, exclude_last)], [(offset, planted (i, j))]): a the planted a; b integer noise at least 40 below every level with
    the planted b at the offset"""
    cases, plants = [], []
    for q, mv in enumerate(SEMI.values()):
        a, pb = planted(mv)
        for off in SEMI_OFFSETS:
            rng = np.random.default_rng([q, off, 3000])
            b = (-40.0 - rng.integers(0, 50, SEMI_M)).astype(np.float32)
            b[off:off + len(pb)] = pb
            cases.append((a, b, len(cases) & 1))
            plants.append((off, path_of(mv)))
    return cases, plants
