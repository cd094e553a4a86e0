"""Cases of the aln text tests (include/rawdtw.h, "aln text"): the lattice of float bit patterns the shared %g formatter is held to, paths
whose lengths and offsets sit on the kernels' edges, and a plain Python model of the text.  tests/test_aln_text_cpu.py runs them against
the C library's snprintf and the host restatement, tests/test_aln_text_gpu.py against the device."""
import functools
import math

import numpy as np

import rawalign_amd as ra

SEED = 20250917
FIXED_MANTISSAS = (0, 1, 2, 0x3fffff, 0x400000, 0x400001, 0x7ffffe, 0x7fffff)
# (input, text) checked with glibc
LITERALS = [(1000005.0, "1e+06"), (1000015.0, "1.00002e+06"), (123456.5, "123456"), (123457.5, "123458"), (999999.5, "1e+06"),
            # (the float nearest 1e-4 and its predecessor 0x1.a36e2cp-14 = 9.99999902e-05 both print 0.0001: the switch to 9.99999e-05 is
            # between 0x1.a36e22p-14 = 9.99999538e-05 and 0x1.a36e20p-14 = 9.99999465e-05)
            (float.fromhex("0x1.a36e2ep-14"), "0.0001"), (float.fromhex("0x1.a36e2cp-14"), "0.0001"), (float.fromhex("0x1.a36e22p-14"), "0.0001"),
            (float.fromhex("0x1.a36e20p-14"), "9.99999e-05"),
            (16777216.0, "1.67772e+07"), (0.0, "0"), (-0.0, "-0"), (math.inf, "inf"), (-math.inf, "-inf"), (1.4e-45, "1.4013e-45")]
PATH_LENS = (0, 1, 63, 64, 65, 128, 129, 4097)


@functools.lru_cache(maxsize=None)
def value_lattice():
    """uint32 bit patterns, unique and sorted: all 512 sign / exponent fields x 4 096 mantissas (the eight fixed ones, the rest from a
    fixed-seed generator), every k + 0.5 for k in [100000, 999999] (the ties of the fixed form's sixth digit), every integer = 5 (mod 10) in
    [10^6, 2^24) (the ties of the exponent form), every decade boundary 1e-45 .. 1e38, the literal cases -- and each of these with its two
    float neighbours."""
    rng = np.random.default_rng(SEED)
    fields = np.arange(512, dtype=np.uint32)[:, None] << np.uint32(23)
    mant = np.concatenate([np.tile(np.array(FIXED_MANTISSAS, np.uint32), (512, 1)), rng.integers(0, 1 << 23, (512, 4096 - len(FIXED_MANTISSAS))).astype(np.uint32)], axis=1)
    parts = [(fields | mant).ravel()]
    parts.append((np.arange(100000, 1000000, dtype=np.float64) + 0.5).astype(np.float32).view(np.uint32))
    parts.append(np.arange(1000005, 1 << 24, 10, dtype=np.float64).astype(np.float32).view(np.uint32))
    parts.append(np.array([float("1e%d" % x) for x in range(-45, 39)], np.float64).astype(np.float32).view(np.uint32))
    parts.append(np.array([x for x, _ in LITERALS], np.float32).view(np.uint32))
    v = np.concatenate(parts)
    v = np.concatenate([v, v + np.uint32(1), v - np.uint32(1)])   # (wraps at the ends of the space: still bit patterns)
    return np.unique(v)


def fmt_g(x):
    """the C library's "%g" of a float, from Python's (which prints a negative NaN without its sign)"""
    x = float(x)
    if math.isnan(x):
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    return "%g" % x


def model_text(step, d, path_off, path_len, recs):
    """(text_off, text) by the definition, in plain Python"""
    out, off = [], [0]
    M = (1 << 64) - 1
    for k in range(len(path_len)):
        n, p0 = int(path_len[k]), int(path_off[k])
        oi, oj, mode = int(recs[k]["off_i"]), int(recs[k]["off_j"]), int(recs[k]["mode"])
        pi, pj = 0, int(recs[k]["j0"])
        s = []
        for q in range(n):
            pi += int(step[p0 + q]) & 1
            pj += (int(step[p0 + q]) >> 1) & 1
            i, j = pi, pj
            if mode:
                i, j = (i + oi) & M, (j + oj) & M
            elif q + 1 == n:
                i, j = (i + n * oi) & M, (j + n * oj) & M
            s.append("(%d,%d,%s)" % (i, j, fmt_g(d[p0 + q])))
        out.append("".join(s))
        off.append(off[-1] + len(out[-1]))
    return np.array(off, np.uint64), "".join(out).encode()


def random_paths(lens, rng, values=None):
    """step bytes (element 0: 0, then 1 .. 3), distances (|N(0,1) - N(0,1)|, or consecutive stretches of `values`' bit patterns), dense
    offsets and lengths for jobs of the given lengths"""
    lens = np.asarray(lens, np.uint32)
    off = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    step = rng.integers(1, 4, max(total, 1)).astype(np.uint8)
    step[off[:-1][lens > 0].astype(np.int64)] = 0
    if values is None:
        d = np.abs(rng.normal(size=max(total, 1)) - rng.normal(size=max(total, 1))).astype(np.float32)
    else:
        assert len(values) >= total
        d = np.ascontiguousarray(values[:max(total, 1)]).view(np.float32)
    return step, d, off, lens


def rec(off_i=0, off_j=0, j0=0, mode=1):
    r = np.zeros(1, ra.ALN_REC_DTYPE)
    r[0] = (off_i, off_j, j0, mode, 0)
    return r


@functools.lru_cache(maxsize=None)
def edge_paths():
    """The path-length and digit-transition cases, as one batch: every length of PATH_LENS under both modes (offsets that are no round
    numbers, j0 != 0 on every third), then paths of 129 whose i crosses 9 -> 10, 999 -> 1000 and 2^32 inside a wave (mode 1: the offset
    sits just below the power), whose j does, and mode-0 jobs whose len * offset is above 2^32 and wraps 2^64.  Distances include the
    literal cases.  -> (step, d, path_off, path_len, recs)"""
    rng = np.random.default_rng(SEED + 1)
    lens, recs = [], []
    for mode in (1, 0):
        for k, n in enumerate(PATH_LENS):
            lens.append(n)
            recs.append(rec(37 + 1000 * k, 123456 + 7 * k, (0, 0, 5)[k % 3], mode))
    for oi, oj in ((3, 0), (990, 0), ((1 << 32) - 40, 0), (0, 9), (0, 995), (5, (1 << 32) - 70), ((1 << 32) - 40, (1 << 32) - 40)):
        lens.append(129)
        recs.append(rec(oi, oj, 2, 1))
    for oi, oj, n in (((1 << 31) + 3, 1 << 30, 129), ((1 << 32) - 1, (1 << 32) - 1, 65), ((1 << 63) + 11, (1 << 62) + 5, 4), (1 << 40, 3, 1)):
        lens.append(n)
        recs.append(rec(oi, oj, 0, 0))
    step, d, off, lens = random_paths(lens, rng)
    lit = np.array([x for x, _ in LITERALS], np.float32)
    d[5:5 + len(lit)] = lit
    return step, d, off, lens, np.concatenate(recs)
