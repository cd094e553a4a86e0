"""Semiglobal (subsequence) DTW: the recurrence in numpy, the ctypes glue to the compiled reference, the recorded fixture and the
shapes of the device tests.

The recurrence (src/dtw.cpp:552-593, 669-753, restated): with d(i, j) = |a[i] - b[j]| in fp32, row 0 is ASSIGNED, D(0, j) = d(0, j);
column 0 is a running sum; elsewhere D(i, j) = min(min(D(i-1, j), D(i, j-1)), D(i-1, j-1)) + d(i, j).  The cost is the minimum of
the last row, end_j the first column that attains it.  The path starts at (n - 1, end_j), walks by the three-way rule of the global
traceback (moves up at j == 0) and stops at i == 0.  exclude_last: _slow and _tb subtract d(n - 1, end_j), _tb also drops the last
element; DTW_semiglobal ignores the flag.

DTW_semiglobal alone carries a float(1e10) sentinel: in the neighbours of its first column and in its running best.  It equals the
sentinel-free recurrence exactly where every prefix sum of column 0 that is an operand (rows 0 .. n - 2) and the result are at most
1e10 -- `sentinel_free(a, b)` decides it from the inputs alone (numpy, not the code under test).  The domains whose scale makes that
impossible for any shape (value_cases.SENTINEL_DOMAINS) are compared with _slow and _tb only; for every other domain each case
that meets the condition is compared with all three, and every such domain has such cases (the tests assert how many).

tests/golden/semiglobal_ref.npz (scripts/make_golden_semiglobal.py) holds, for `fixture_cases()`, the inputs, the three functions'
costs, end_j and DTW_semiglobal_tb's full paths for exclude_last 0 and 1."""
import ctypes as C
import os

import numpy as np

from tests import value_cases as vc
from tests.golden_util import golden_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = "semiglobal_ref.npz"
F32_1E10 = np.float32(1e10)

# rows (n) at every class and strip edge of the kernel: 64 / 128 / 256 rows end a rows-per-lane class, 512 rows are a strip of the
# widest class, 1025 rows are three strips (the four-wave pipelined form), 1537 four; columns (m) around the 64-column chunk
SWEEP_N = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 1025, 1537)
SWEEP_M = (1, 2, 63, 64, 65, 200, 1000)
TALL = ((300, 5), (129, 1))  # n > m: the path runs along j == 0
PLANT_AT = (0, 63, 64, 65, -1)  # end_j planted there (-1: m - 1)
# value domains: all three reference functions / _slow and _tb only
ALL_THREE = tuple(d for d in vc.DOMAIN_NAMES if d not in vc.SENTINEL_DOMAINS)
assert sorted(ALL_THREE) == sorted(("s9", "cross", "spike", "sub38", "sub41", "sub44", "zeros", "ints"))
DOMAIN_SHAPES = ((1, 1), (1, 40), (2, 9), (3, 70), (4, 4), (9, 1), (30, 65), (64, 64), (65, 33), (70, 130), (129, 1), (100, 20))


# ---- the recurrence in numpy -----------------------------------------------------------------------------------------------
def matrix(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n, m = len(a), len(b)
    d = np.abs(a[:, None] - b[None, :]).astype(np.float32)
    D = np.empty((n, m), np.float32)
    D[0] = d[0]
    for i in range(1, n):
        D[i, 0] = D[i - 1, 0] + d[i, 0]
        prev, cur, di = D[i - 1], D[i], d[i]
        for j in range(1, m):
            cur[j] = min(min(prev[j], cur[j - 1]), prev[j - 1]) + di[j]
    return d, D


def model(a, b, exclude_last=False):
    """-> (cost, end_j, path_i, path_j, path_d): _tb's answer; _slow's is (cost, end_j)"""
    d, D = matrix(a, b)
    n, m = D.shape
    best, end_j = D[n - 1, 0], 0
    for j in range(1, m):
        if D[n - 1, j] < best:
            best, end_j = D[n - 1, j], j
    i, j = n - 1, end_j
    pi, pj = [i], [j]
    while i > 0:
        if j == 0:
            i -= 1
        else:
            left, top, tl = D[i - 1, j], D[i, j - 1], D[i - 1, j - 1]
            if left < min(top, tl):
                i -= 1
            elif top < min(left, tl):
                j -= 1
            else:
                i, j = i - 1, j - 1
        pi.append(i)
        pj.append(j)
    pi, pj = np.array(pi[::-1], np.uint32), np.array(pj[::-1], np.uint32)
    pd = d[pi, pj]
    cost = np.float32(best)
    if exclude_last:
        cost = np.float32(cost - d[n - 1, end_j])
        pi, pj, pd = pi[:-1], pj[:-1], pd[:-1]
    return cost, end_j, pi, pj, pd


def sentinel_free(a, b):
    """True where DTW_semiglobal (1e10 in column 0's neighbours and in its running best) equals the sentinel-free recurrence"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    s = np.float32(0.0)
    for i in range(len(a) - 1):
        s = np.float32(s + np.abs(a[i] - b[0]))
        if not s <= F32_1E10:
            return False
    return bool(model(a, b)[0] <= F32_1E10)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- the compiled reference through ctypes -------------------------------------------------------------------------------------
class RefSemiglobal:
    """oracle/_ref/libref_dtw.so's DTW_semiglobal, DTW_semiglobal_slow and DTW_semiglobal_tb (C++ symbols).  _tb returns a dtw_result by
    value: called with a hidden first argument that points at zeroed room, it leaves the cost at offset 0 and its vector's begin and
    end at offsets 8 and 16; an element is 24 bytes (size_t i, size_t j, float difference)."""

    PATH = os.path.join(ROOT, "oracle", "_ref", "libref_dtw.so")
    ELEM = np.dtype([("i", "<u8"), ("j", "<u8"), ("d", "<f4"), ("pad", "<u4")])

    @classmethod
    def available(cls):
        return os.path.exists(cls.PATH)

    def __init__(self):
        lib = C.CDLL(self.PATH)
        args = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_bool]
        self._fast = lib._Z14DTW_semiglobalPKfjS0_jb
        self._slow = lib._Z19DTW_semiglobal_slowPKfjS0_jb
        self._tb = lib._Z17DTW_semiglobal_tbPKfjS0_jb
        self._fast.restype = self._slow.restype = C.c_float
        self._fast.argtypes = self._slow.argtypes = args
        self._tb.restype = None
        self._tb.argtypes = [C.c_void_p] + args

    @staticmethod
    def _arrs(a, b):
        return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)

    def semiglobal(self, a, b, exclude_last=False):
        a, b = self._arrs(a, b)
        return np.float32(self._fast(a.ctypes.data, len(a), b.ctypes.data, len(b), bool(exclude_last)))

    def slow(self, a, b, exclude_last=False):
        a, b = self._arrs(a, b)
        return np.float32(self._slow(a.ctypes.data, len(a), b.ctypes.data, len(b), bool(exclude_last)))

    def tb(self, a, b, exclude_last=False):
        """-> (cost, path_i, path_j, path_d)"""
        a, b = self._arrs(a, b)
        room = (C.c_uint64 * 8)()
        self._tb(C.addressof(room), a.ctypes.data, len(a), b.ctypes.data, len(b), bool(exclude_last))
        cost = np.frombuffer(room, np.float32, 1)[0]
        begin, end = int(room[1]), int(room[2])
        count = (end - begin) // self.ELEM.itemsize
        el = np.frombuffer((C.c_char * (count * self.ELEM.itemsize)).from_address(begin), self.ELEM).copy() if count else np.zeros(0, self.ELEM)
        return np.float32(cost), el["i"].astype(np.uint32), el["j"].astype(np.uint32), el["d"].copy()


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def planted(n, m, ats, seed=0):
    """signals whose last row's minimum lies at the columns `ats`: b is forty away from a everywhere but for a copy of a that ends at
    each of them (cost 0, exactly; an end before column n - 1 takes the copy's tail, and a's head warps onto b[0]).  Several ends are
    equal minima: the first wins."""
    rng = np.random.default_rng([n, m, seed, 77])
    a = rng.normal(size=n).astype(np.float32)
    b = (rng.normal(size=m) + 40.0).astype(np.float32)
    for at in ats:
        at = at % m
        lo = max(0, at - n + 1)
        b[lo:at + 1] = a[n - 1 - (at - lo):]
    return a, b


def fixture_cases():
    """[(tag, a, b)]: every value domain over DOMAIN_SHAPES, random and integer shapes with n < m, n == m and n > m, and ties"""
    out = []
    for name in vc.DOMAIN_NAMES:
        rng = vc.domain_rng(name, salt=41)
        for n, m in DOMAIN_SHAPES:
            out.append((name, vc.DOMAINS[name](rng, n), vc.DOMAINS[name](rng, m)))
    rng = np.random.default_rng(4100)
    for t in range(24):
        n = int(rng.integers(1, 90))
        m = int(rng.integers(1, 140)) if t % 4 else max(1, n // 3)
        if t % 3 == 0:
            out.append(("int", rng.integers(-2, 3, n).astype(np.float32), rng.integers(-2, 3, m).astype(np.float32)))
        else:
            out.append(("normal", rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32)))
    for n, m in TALL:
        out.append(("tall", rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32)))
        out.append(("tall-int", rng.integers(-1, 2, n).astype(np.float32), rng.integers(-1, 2, m).astype(np.float32)))
    a, b = planted(20, 90, (30, 70))
    out.append(("two-minima", a, b))
    return out


class Fixture:
    """semiglobal_ref.npz: per case k the inputs, bits of DTW_semiglobal (fast), of _slow and _tb for exclude_last 0 / 1, end_j, and
    _tb's paths"""

    def __init__(self):
        self.z = np.load(golden_path(FIXTURE))

    def __len__(self):
        return len(self.z["n"])

    def tag(self, k):
        return str(self.z["tag"][k])

    def inputs(self, k):
        z = self.z
        ao, bo = int(z["a_off"][k]), int(z["b_off"][k])
        return z["a"][ao:ao + int(z["n"][k])].copy(), z["b"][bo:bo + int(z["m"][k])].copy()

    def path(self, k, ex):
        z = self.z
        o, ln = int(z["tb_off"][k, ex]), int(z["tb_len"][k, ex])
        return z["path_i"][o:o + ln].astype(np.uint32), z["path_j"][o:o + ln].astype(np.uint32), z["path_d"][o:o + ln]
