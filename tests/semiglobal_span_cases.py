"""The semiglobal span (include/rawdtw.h, "span"): its forward model in numpy and the job lists of its tests.

The span of a job is (cost, j0, end_j): cost and end_j as tests/semiglobal_cases.py states them, j0 the column of element 0 of
DTW_semiglobal_tb's path.  Stated forwards, with S(i, j) the start column of the path that ends in (i, j): S(0, j) = j; S(i, 0) = 0;
elsewhere, with up = D(i-1, j), lf = D(i, j-1), dg = D(i-1, j-1): up < min(lf, dg) -> S(i-1, j); else lf < min(up, dg) -> S(i, j-1);
else S(i-1, j-1) (up == lf < dg takes the diagonal, the reference's quirk).  j0 = S(n-1, end_j).  exclude_last changes the cost only."""
import numpy as np

from tests import semiglobal_cases as sc

# rows: tests/semiglobal_cases.SWEEP_N and six strips of the widest class, where the four-slot ring of boundary rows reuses slots 0 and 1
SPAN_SWEEP_N = sc.SWEEP_N + (2561,)
PIPELINED_N = tuple(n for n in SPAN_SWEEP_N if n >= 1025)  # the shapes that run on four waves, or on one wave without "full_wg"
PLANT_N, PLANT_M = (400, 513, 1025), 3000


def forward_model(a, b, exclude_last=False):
    """-> (cost, j0, end_j) by the definition above: two rows of D and S"""
    d, D = sc.matrix(a, b)
    n, m = D.shape
    S = np.arange(m, dtype=np.int64)
    for i in range(1, n):
        up, T = D[i - 1], np.empty(m, np.int64)
        cur = D[i]
        T[0] = 0
        for j in range(1, m):
            u, lf, dg = up[j], cur[j - 1], up[j - 1]
            if u < min(lf, dg):
                T[j] = S[j]
            elif lf < min(u, dg):
                T[j] = T[j - 1]
            else:
                T[j] = S[j - 1]
        S = T
    best, end_j = D[n - 1, 0], 0
    for j in range(1, m):
        if D[n - 1, j] < best:
            best, end_j = D[n - 1, j], j
    cost = np.float32(best)
    if exclude_last:
        cost = np.float32(cost - d[n - 1, end_j])
    return cost, int(S[end_j]), end_j


def sweep_cases(ns=SPAN_SWEEP_N, seed=525):
    """[(a, b, exclude_last)]: ns x SWEEP_M and TALL, a normal and an integer-valued pair (ties) a shape"""
    rng = np.random.default_rng(seed)
    shapes = [(n, m) for n in ns for m in sc.SWEEP_M] + list(sc.TALL)
    cases = []
    for q, (n, m) in enumerate(shapes):
        cases.append((rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32), q & 1))
        cases.append((rng.integers(-2, 3, n).astype(np.float32), rng.integers(-2, 3, m).astype(np.float32), 1 - (q & 1)))
    return cases


def planted_starts(n, m=PLANT_M):
    """[(at, j0)]: ends of the planted copy such that the path starts in column 0, 63, 64, 65, and in a column whose 64-column chunk
    lies more than one chunk before end_j's (n >= 400: the copy spans six chunks or more)"""
    far = 1000
    assert (far + n - 1) // 64 - far // 64 > 1 and far + n - 1 < m
    return [(j0 + n - 1, j0) for j0 in (0, 63, 64, 65, far)]


def quirk_case():
    """-> ((a, b), (cost, j0, end_j)): integer signals on whose path up == lf < dg occurs, and all three moves lead to other starts.
        a = (2, 1, 3), b = (2, 0, 1, 3, 0)
        D = [[0, 2, 1, 1, 2],
             [1, 1, 1, 3, 2],
             [2, 4, 3, 1, 4]]
    Row 2's minimum is D(2, 3) = 1.  At (2, 3): up = 3, lf = 3, dg = 1: the diagonal, to (1, 2).  At (1, 2): up = D(0, 2) = 1,
    lf = D(1, 1) = 1, dg = D(0, 1) = 2: up is not below min(lf, dg) = 1 and lf is not below min(up, dg) = 1, so the walk takes the
    diagonal although it is the largest of the three, to (0, 1): j0 = 1.  Moving up instead would give j0 = 2; moving left leads to
    (1, 1), where dg = D(0, 0) = 0 is least: j0 = 0."""
    return (np.array([2, 1, 3], np.float32), np.array([2, 0, 1, 3, 0], np.float32)), (np.float32(1.0), 1, 3)
