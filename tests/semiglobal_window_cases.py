"""The semiglobal traceback in windows (include/rawdtw.h, "semiglobal, in windows"): what its tests share, all of it numpy or plain
Python and none of it the code under test -- the windows a path enters and how it leaves them, counted from the path; the layout
(rawalign_amd/csrc/rawdtw_semi_window.h) restated; the planted multi-window signals.

A path enters a window wherever the walk stands at a position (i, j) with i > 0 whose window j // C is not the one of the position
before it (the end cell enters the first one).  The position that ends the walk, i == 0, enters none.  A job with m <= C is not
windowed: 0 windows."""
import numpy as np

from tests import semiglobal_cases as sc

C64 = 64


# ---- windows of a path ------------------------------------------------------------------------------------------------------------
def windows_of(pi, pj, m, C):
    """windows entered by the walk whose FULL path (start first, nothing popped) is (pi, pj)"""
    if C == 0 or m <= C:
        return 0
    i, j = np.asarray(pi, np.int64)[::-1], np.asarray(pj, np.int64)[::-1]   # end first, as the walk goes
    inside = i > 0
    w = j // C
    new = np.ones(len(i), bool)
    new[1:] = w[1:] != w[:-1]
    return int((inside & new).sum())


def exits_of(pi, pj, m, C):
    """how the walk left its windows: a list of 'left' / 'diag', one a step from a column c_lo to c_lo - 1"""
    if C == 0 or m <= C:
        return []
    i, j = np.asarray(pi, np.int64)[::-1], np.asarray(pj, np.int64)[::-1]
    out = []
    for q in range(1, len(i)):
        if j[q] // C != j[q - 1] // C:
            assert j[q] == j[q - 1] - 1 and j[q - 1] % C == 0
            out.append("left" if i[q] == i[q - 1] else "diag")
    return out


def full_path(a, b):
    """(pi, pj, end_j) of the numpy model, nothing popped"""
    _, end_j, pi, pj, _ = sc.model(a, b, False)
    return pi, pj, end_j


# ---- the layout restated (rawdtw_semi_window.h, rawdtw_semiglobal.h) -------------------------------------------------------------
def al256(x):
    return (int(x) + 255) // 256 * 256


def rpl_of(n):
    return 1 if n <= 64 else 2 if n <= 128 else 4 if n <= 256 else 8


def semi_dir_bytes(n, m):
    """the n x m form's direction bytes (semi_dir_bytes)"""
    rpl = rpl_of(n)
    strips = (n + 64 * rpl - 1) // (64 * rpl)
    spb = 8 if rpl == 8 else 16
    return strips * ((m + 63 + spb - 1) // spb) * 64 * 16


def windowed(m, C):
    return C != 0 and m > C


def window_dir_bytes(n, m, C):
    return semi_dir_bytes(n, min(C, m))


def checkpoints(m, C):
    return m // C


def ckpt_bytes(n, m, C):
    return al256(checkpoints(m, C) * n * 4)


def job_bytes(n, m, C):
    """what the plan lays out and the split counts for a job on a context whose window is C"""
    if not windowed(m, C):
        return semi_dir_bytes(n, m) + 256          # the split's count of an n x m job
    return al256(window_dir_bytes(n, m, C)) + ckpt_bytes(n, m, C)


def workspace_bytes(n, m, C):
    """what rawdtw_semiglobal_timing reports as a job's direction bytes"""
    if not windowed(m, C):
        return al256(semi_dir_bytes(n, m))
    return job_bytes(n, m, C)


def split(byte_list, budget):
    """job counts of the sub-batches (rawdtw_tb_layout.h: a job joins unless that passes the budget; one over the budget goes alone)"""
    out, k = [], 0
    while k < len(byte_list):
        cnt, tot = 0, 0
        while k + cnt < len(byte_list) and (cnt == 0 or tot + byte_list[k + cnt] <= budget):
            tot += byte_list[k + cnt]
            cnt += 1
        out.append(cnt)
        k += cnt
    return out


# ---- planted multi-window paths -----------------------------------------------------------------------------------------------------
PLANTS = ((70, 3, 40, 50), (30, 5, 64, 64), (129, 2, 1, 63))   # (n, r, left flank, right flank): 70 x 300, 30 x 278, 129 x 322


def plant(n, r, left, right, seed=0):
    """b = flank + np.repeat(a, r) + small noise + flank; the flanks lie forty away from a"""
    rng = np.random.default_rng([n, r, seed, 99])
    a = rng.normal(size=n).astype(np.float32)
    mid = (np.repeat(a, r) + 0.01 * rng.normal(size=n * r)).astype(np.float32)
    lf = (rng.normal(size=left) + 40.0).astype(np.float32)
    rt = (rng.normal(size=right) + 40.0).astype(np.float32)
    return a, np.concatenate([lf, mid, rt])


def planted_cases(C=C64):
    """[(tag, a, b)]: the three plants as they are, and each shifted by its left flank so that end_j falls on k C - 1, k C and k C + 1
    and that j0 == k C.  (The middle of b does not change with the flank's length -- the generator draws a, the noise and then the
    flanks --, and the flanks are far away, so the path moves with the flank: the shift is read off the unshifted plant's path.)"""
    out = []
    for n, r, left, right in PLANTS:
        a, b = plant(n, r, left, right)
        out.append(("plant %dx%d" % (n, r), a, b))
        pi, pj, end_j = full_path(a, b)
        j0 = int(pj[0])
        for tag, at, rem in (("end kC-1", end_j, C - 1), ("end kC", end_j, 0), ("end kC+1", end_j, 1), ("j0 kC", j0, 0)):
            shift = (rem - at) % C
            a2, b2 = plant(n, r, left + shift, right)
            assert np.array_equal(a, a2)
            out.append(("%s %dx%d" % (tag, n, r), a2, b2))
    rng = np.random.default_rng(31)
    out.append(("m == C", rng.normal(size=40).astype(np.float32), rng.normal(size=C).astype(np.float32)))
    out.append(("m == C + 1", rng.normal(size=40).astype(np.float32), rng.normal(size=C + 1).astype(np.float32)))
    return out
