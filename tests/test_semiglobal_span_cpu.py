"""The semiglobal span without a device (include/rawdtw.h, "span"): rawdtw_semiglobal_span_host and the numpy forward model
(tests/semiglobal_span_cases.py) against the reference's own recorded answers (tests/golden/semiglobal_ref.npz: end_j, the _slow cost
and element 0 of DTW_semiglobal_tb's path), against the live reference where oracle/_ref exists, against the O(n m) host path
(rawdtw_semiglobal_tb_host) and against starts known by construction; and the reduction of Engine.semiglobal_place against a loop."""
import math

import numpy as np
import pytest

import rawalign_amd as ra
from tests import semiglobal_cases as sc
from tests import semiglobal_span_cases as sp


@pytest.fixture(scope="module")
def fx():
    return sc.Fixture()


def fixture_answers(fx, k):
    """-> [(cost bits, j0, end_j) for exclude_last 0, 1]: j0 from the recorded path with the last element kept (exclude_last pops
    it: the path of a one-row job is empty then, and j0 does not depend on the flag)"""
    j0 = int(fx.path(k, 0)[1][0])
    return [(int(fx.z["slow"][k, ex]), j0, int(fx.z["end_j"][k])) for ex in (0, 1)]


def test_host_span_equals_the_recorded_reference(fx):
    assert len(fx) == 173
    moved = 0
    for k in range(len(fx)):
        a, b = fx.inputs(k)
        want = fixture_answers(fx, k)
        for ex in (0, 1):
            c, j0, ej = ra.semiglobal_span_host(a, b, ex)
            assert (int(sc.bits(c)[0]), j0, ej) == want[ex], (k, fx.tag(k), ex, c, j0, ej, want[ex])
            assert fx.z["slow"][k, ex] == fx.z["tb_cost"][k, ex]
        moved += want[0][1] != 0
    assert moved >= 100, moved  # (the check cannot pass on zeros)


def test_forward_model_equals_the_recorded_reference(fx):
    """the numpy forward model is a yardstick of its own (it states the definition and nothing of the library), so it is held to the
    reference's recorded answers here; and the library's host span gives the model's answer on every case"""
    for k in range(len(fx)):
        a, b = fx.inputs(k)
        want = fixture_answers(fx, k)
        for ex in (0, 1):
            c, j0, ej = sp.forward_model(a, b, ex)
            assert (int(sc.bits(c)[0]), j0, ej) == want[ex], (k, fx.tag(k), ex)
            hc, hj0, hej = ra.semiglobal_span_host(a, b, ex)
            assert (sc.bits(hc)[0], hj0, hej) == (sc.bits(c)[0], j0, ej), (k, fx.tag(k), ex)


@pytest.mark.skipif(not sc.RefSemiglobal.available(), reason="oracle/_ref is built only where the reference's sources are")
def test_span_equals_live_reference():
    ref = sc.RefSemiglobal()
    rng = np.random.default_rng(4343)
    for t in range(200):
        n, m = int(rng.integers(1, 70)), int(rng.integers(1, 110))
        if t % 5 == 0:
            n, m = m, max(1, n // 4)
        if t % 2:
            a, b = rng.integers(-2, 3, n).astype(np.float32), rng.integers(-2, 3, m).astype(np.float32)
        else:
            a, b = rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32)
        _, _, pj, _ = ref.tb(a, b, False)
        for ex in (0, 1):
            c = ref.tb(a, b, ex)[0]
            want = (int(sc.bits(c)[0]), int(pj[0]), int(pj[-1]))
            hc, hj0, hej = ra.semiglobal_span_host(a, b, ex)
            mc, mj0, mej = sp.forward_model(a, b, ex)
            assert (int(sc.bits(hc)[0]), hj0, hej) == want and (int(sc.bits(mc)[0]), mj0, mej) == want, (t, ex)


def test_host_span_equals_the_matrix_host_path():
    cases = sp.sweep_cases(sc.SWEEP_N)
    for n, m in ((20, 130), (130, 700)):
        for at in sc.PLANT_AT:
            cases.append(sc.planted(n, m, (at,)) + (at & 1,))
        cases.append(sc.planted(n, m, (40, 100)) + (0,))
    assert len(cases) >= 2 * (len(sc.SWEEP_N) * len(sc.SWEEP_M) + len(sc.TALL))
    for k, (a, b, ex) in enumerate(cases):
        r, ej = ra.semiglobal_host(a, b, ex, traceback=True)
        first = r.j[0] if len(r.j) else ra.semiglobal_host(a, b, 0, traceback=True)[0].j[0]  # (n == 1 with its only element popped)
        hc, hj0, hej = ra.semiglobal_span_host(a, b, ex)
        assert sc.bits(hc)[0] == sc.bits(r.cost)[0] and hej == ej and hj0 == first, (k, len(a), len(b), ex)


def test_starts_known_by_construction():
    """a copy of a that ends at column `at` >= n - 1 costs exactly 0 and starts at at - n + 1, whatever else the matrix holds; the last
    shape is one the O(n m) host path should not be asked for (2 000 x 100 000: 200 M direction bytes)"""
    for n, m, at in ((20, 130, 19), (20, 130, 129), (130, 700, 192), (400, 3000, 1399), (2000, 100_000, 70_000)):
        a, b = sc.planted(n, m, (at,))
        for ex in (0, 1):
            c, j0, ej = ra.semiglobal_span_host(a, b, ex)
            assert (sc.bits(c)[0], j0, ej) == (0, at - n + 1, at), (n, m, at, ex, c, j0, ej)
    a, b = sc.planted(20, 130, (40, 100))  # two equal minima: the first end, and its own start
    assert ra.semiglobal_span_host(a, b)[1:] == (21, 40)


def test_edges_and_ties():
    rng = np.random.default_rng(99)
    for m in (1, 2, 65, 300):  # n == 1: the path is one element
        a, b = rng.normal(size=1).astype(np.float32), rng.normal(size=m).astype(np.float32)
        c, j0, ej = ra.semiglobal_span_host(a, b)
        assert j0 == ej == int(np.argmin(np.abs(a[0] - b).astype(np.float32)))
        assert sp.forward_model(a, b)[1:] == (j0, ej)
    for n in (1, 2, 129):  # m == 1: a run along column 0
        a, b = rng.normal(size=n).astype(np.float32), rng.normal(size=1).astype(np.float32)
        assert ra.semiglobal_span_host(a, b)[1:] == (0, 0) and sp.forward_model(a, b)[1:] == (0, 0)
    (a, b), want = sp.quirk_case()  # up == lf < dg takes the diagonal
    got = ra.semiglobal_span_host(a, b)
    assert (sc.bits(got[0])[0], got[1], got[2]) == (sc.bits(want[0])[0], want[1], want[2])
    assert sp.forward_model(a, b) == want
    r, _ = ra.semiglobal_host(a, b, 0, traceback=True)
    assert r.j[0] == want[1]


def test_span_host_outputs_may_be_null_and_bad_arguments_are_refused():
    import ctypes as C

    lib = ra.load_library()
    a, b = sc.planted(20, 130, (70,))
    pa, pb = a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    j0 = C.c_uint32(7)
    assert lib.rawdtw_semiglobal_span_host(pa, len(a), pb, len(b), 0, None, C.byref(j0), None) == 0 and j0.value == 51
    assert lib.rawdtw_semiglobal_span_host(pa, len(a), pb, len(b), 0, None, None, None) == 0
    for x, y in ((a[:0], b), (a, b[:0])):
        with pytest.raises(ra.RawDTWError) as e:
            ra.semiglobal_span_host(x, y)
        assert e.value.status == 1


def place_loop(cost, j0, end_j):
    """semiglobal_place's reduction as its description reads, in plain Python"""
    out = []
    for r in range(len(cost)):
        best = -1
        for t in range(len(cost[r])):
            c = float(cost[r][t])
            if not math.isnan(c) and (best < 0 or c < float(cost[r][best])):
                best = t
        second = math.inf
        for t in range(len(cost[r])):
            c = float(cost[r][t])
            if t != best and not math.isnan(c) and c < second:
                second = c
        out.append((best, math.nan if best < 0 else float(cost[r][best]), 0 if best < 0 else int(j0[r][best]),
                    0 if best < 0 else int(end_j[r][best]), second))
    return out


def test_place_reduction_equals_a_loop():
    nan, inf = np.nan, np.inf
    cost = np.array([[3, 1, 2, 5],        # a plain minimum
                     [2, 1, 1, 1],        # a tie: the lowest target index wins, second equals the cost
                     [nan, 4, nan, 4],    # NaN never wins
                     [nan, nan, nan, nan],  # no target at all
                     [nan, inf, nan, nan],  # +inf is a cost, the only one here
                     [inf, inf, 7, nan],
                     [0, -1, -1, nan]], np.float32)
    rng = np.random.default_rng(5)
    j0 = rng.integers(0, 1000, cost.shape).astype(np.uint32)
    end_j = j0 + rng.integers(0, 1000, cost.shape).astype(np.uint32)
    for c, s, e in ((cost, j0, end_j), (cost[:, :1], j0[:, :1], end_j[:, :1]), (cost[:, 2:3], j0[:, 2:3], end_j[:, 2:3])):
        got = ra.semiglobal_place_reduce(c, s, e)
        assert got["target"].dtype == np.int32
        want = place_loop(c, s, e)
        for r, (t, wc, ws, we, w2) in enumerate(want):
            assert got["target"][r] == t and got["j0"][r] == ws and got["end_j"][r] == we, (r, want[r])
            assert (math.isnan(wc) and math.isnan(got["cost"][r])) or got["cost"][r] == wc, (r, want[r])
            assert got["second"][r] == w2, (r, got["second"][r], w2)
    assert [w[0] for w in place_loop(cost, j0, end_j)] == [1, 1, 1, -1, 1, 2, 1]
    table = rng.normal(size=(50, 6)).astype(np.float32).round(1)  # (rounded: ties)
    table[rng.random(table.shape) < 0.2] = nan
    got = ra.semiglobal_place_reduce(table, np.zeros(table.shape, np.uint32), np.ones(table.shape, np.uint32))
    for r, (t, wc, _, _, w2) in enumerate(place_loop(table, np.zeros(table.shape), np.ones(table.shape))):
        assert got["target"][r] == t and got["second"][r] == np.float32(w2)
