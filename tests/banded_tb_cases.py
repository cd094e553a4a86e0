"""The banded global traceback (include/rawdtw.h, "banded traceback"): the definition in numpy, the model of the direction bytes and of
the sub-batch cut (rawalign_amd/csrc/rawdtw_band_tb.h, rawdtw_band_tb.cpp), the value domains and the case lists.

The definition, for a job (a, n, b, m, R), i indexing a and j indexing b:
  cell set   what the oracle's orc_dtw_banded_cellset marks (the cells DTW_global_slantedbanded_antidiagonalwise evaluates)
  matrix     B(0, 0) = d(0, 0); every other cell of S min(min(B(i-1, j), B(i, j-1)), B(i-1, j-1)) + d(i, j) in fp32; a neighbour outside
             the matrix or outside S reads float(1e10)
  walk       DTW_global_tb's (dtw.cpp:625-647) from (n-1, m-1) to (0, 0) with absent neighbours read as 1e10; a step that lands outside
             S: no path
`model` fills by antidiagonals (vectorised, float32 throughout) and walks in plain Python."""
import numpy as np

from tests import value_cases as vc

INF = np.float32(1e10)
RADII = (0, 1, 2, 3, 5)
MAX_K = 13000  # kMaxWaveBandK: slant-corrected radius + 1


def bits(x):
    return np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32)


def model(orc, a, b, R, exclude_last=False):
    """-> dict(cost, i, j, d, has_path, tie): the definition; tie = the walk met L == T < X (the reference's diagonal quirk)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n, m = len(a), len(b)
    _, _, mask = orc.dtw_banded_cellset(a, b, R)  # [longer][shorter]
    if n < m:
        mask = mask.T
    mask = mask.astype(bool)
    assert mask.shape == (n, m) and mask[0, 0] and mask[n - 1, m - 1]
    pad = np.full((n + 1, m + 1), INF, np.float32)  # pad[i + 1, j + 1] = B(i, j); absent cells and the border stay 1e10
    ii, jj = np.nonzero(mask)
    order = np.argsort(ii + jj, kind="stable")
    ii, jj = ii[order], jj[order]
    s = ii + jj
    cut = np.flatnonzero(np.diff(s)) + 1
    for gi, gj in zip(np.split(ii, cut), np.split(jj, cut)):
        d = np.abs(a[gi] - b[gj]).astype(np.float32)
        if gi[0] + gj[0] == 0:
            pad[1, 1] = d[0]
            continue
        best = np.minimum(np.minimum(pad[gi, gj + 1], pad[gi + 1, gj]), pad[gi, gj])
        pad[gi + 1, gj + 1] = (best + d).astype(np.float32)
    cost = pad[n, m]
    i, j = n - 1, m - 1
    pi, pj, tie, has_path = [i], [j], False, True
    while i > 0 or j > 0:
        if i == 0:
            j -= 1
        elif j == 0:
            i -= 1
        else:
            L, T, X = pad[i, j + 1], pad[i + 1, j], pad[i, j]
            if L < min(T, X):
                i -= 1
            elif T < min(L, X):
                j -= 1
            else:
                tie = tie or (L == T and L < X)
                i -= 1
                j -= 1
        if not mask[i, j]:
            has_path = False
            break
        pi.append(i)
        pj.append(j)
    last = np.abs(a[n - 1] - b[m - 1]).astype(np.float32)
    if exclude_last:
        cost = np.float32(cost - last)
    if not has_path:
        return dict(cost=np.float32(cost), i=np.zeros(0, np.uint32), j=np.zeros(0, np.uint32), d=np.zeros(0, np.float32), has_path=False, tie=tie)
    pi, pj = np.array(pi[::-1], np.uint32), np.array(pj[::-1], np.uint32)
    if exclude_last:
        pi, pj = pi[:-1], pj[:-1]
    return dict(cost=np.float32(cost), i=pi, j=pj, d=np.abs(a[pi] - b[pj]).astype(np.float32), has_path=True, tie=tie)


def forward_sum(d):
    """the fp32 sum of a path's distances in path order"""
    acc = np.float32(0.0)
    for x in np.asarray(d, np.float32):
        acc = np.float32(acc + x)
    return acc


# ---- the layout's byte count and the sub-batch cut ----
def slanted_radius(n, m, r0):
    """dtw.cpp:298-300, the product and the sum in unsigned 32-bit arithmetic"""
    N, M = max(n, m), min(n, m)
    return r0 + ((((N - M) * r0) & 0xFFFFFFFF) + N - 1 & 0xFFFFFFFF) // N


def dir_bytes(n, m, r0):
    """one job's directions: a 16-byte record and a row of ceil(K / 64) 16-byte chunks (two 64-bit planes of 64 slots) for every
    antidiagonal sum 0 .. n + m - 2, K = slanted radius + 1"""
    K = slanted_radius(n, m, r0) + 1
    return (n + m - 1) * (16 + (K + 63) // 64 * 16)


def full_matrix_dir_bytes(n, m):
    """what the same window costs as a full matrix at two bits a cell"""
    return n * m // 4


def sub_batches(jobs, workspace_mb):
    """the cut of rawdtw_banded_traceback_steps: a job joins the current sub-batch unless its bytes (rounded up to 256) pass the budget;
    a job over the budget goes alone.  -> the sub-batches' job counts"""
    budget = workspace_mb << 20
    out, cur, used = [], 0, 0
    for j in jobs:
        b = (dir_bytes(int(j["n"]), int(j["m"]), int(j["band_radius"])) + 255) & ~255
        if cur and used + b > budget:
            out.append(cur)
            cur, used = 0, 0
        cur += 1
        used += b
    if cur:
        out.append(cur)
    return out


# ---- value domains and case lists ----
def _normal(rng, size):
    return rng.normal(size=size).astype(np.float32)


def _three(rng, size):
    return rng.integers(-1, 2, size=size).astype(np.float32)


def _three_3e10(rng, size):
    return (rng.integers(-1, 2, size=size) * 3e10).astype(np.float32)


PLAIN = {"normal": _normal, "three": _three}                 # sums stay below 1e10
BIG = {"three3e10": _three_3e10, "s9": vc.DOMAINS["s9"]}     # sums pass 1e10: walks may leave S
# a smallest job without a path (the first found by enumeration over {0, 3e10}-valued windows, shapes in row-major order up to 3 x 3)
SMALLEST_NO_PATH = (np.array([0, 0, 0], np.float32), np.array([0, 3e10, 0], np.float32), 1)
# include/rawdtw.h's walk takes row 0 and column 0 by j-- / i-- (dtw.cpp:626-631), so this job HAS a path, (0, 0), (0, 1): both of its
# cells are in S.  (It would have none under a walk that read three 1e10 neighbours at (0, 1) and stepped diagonally.)
ONE_BY_TWO = (np.array([3e10], np.float32), np.array([0, 0], np.float32), 1)


def grid_cases(domains, top, radii=RADII, salt=0):
    """[(a, b, R)]: every (n, m) in [1, top]^2, one pair of windows a shape and domain, every radius (None stands for n + m)"""
    out = []
    for dn, name in enumerate(sorted(domains)):
        rng = np.random.default_rng([dn, salt, top, 977])
        for n in range(1, top + 1):
            for m in range(1, top + 1):
                a, b = domains[name](rng, n), domains[name](rng, m)
                for R in radii:
                    out.append((a, b, n + m if R is None else R))
    return out


def boundary_radii():
    """K = R + 1 on both sides of the fill kernel's class bounds (64: one wave / four; 1 024, 4 096: LDS classes), of its 256-slot turn,
    of 16, 64, 256 and 8 192, and the limit"""
    ks = set()
    for k in (16, 64, 256, 1024, 4096, 8192):
        ks.update((k - 1, k, k + 1))
    ks.update((128, 192, 512, MAX_K - 1, MAX_K))
    return sorted(k - 1 for k in ks)
