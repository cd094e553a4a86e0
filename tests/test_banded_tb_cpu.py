"""The banded global traceback without a device: the library's host restatement (rawdtw_banded_tb_host) against the numpy model of the
definition (tests/banded_tb_cases.py), bit for bit -- cost, length, i, j, distances, exclude_last's pop; the cost against the oracle's
banded cost (and the compiled reference's where oracle/_ref is built); a band that holds the whole matrix against the oracle's
DTW_global_tb; the forward-sum identity; the domains above 1e10 with their jobs without a path.

A job of one row or one column has a path whatever its values: a = [3e10], b = [0, 0], R = 1 walks (0, 1) to (0, 0) by the i == 0 rule
(dtw.cpp:626-628), which reads no neighbour, and both corners are always in S -- test_one_by_two.  test_above_1e10 plants a smallest
job that has none (banded_tb_cases.SMALLEST_NO_PATH)."""
import numpy as np
import pytest

import rawalign_amd as ra
from oracle.loader import Oracle
from tests import banded_tb_cases as bc


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def hold(orc, a, b, R, ex, what):
    """the host restatement against the model; -> the model's answer"""
    w = bc.model(orc, a, b, R, ex)
    r = ra.banded_tb_host(a, b, R, ex)
    key = (what, len(a), len(b), R, ex)
    assert bc.bits(r.cost)[0] == bc.bits(w["cost"])[0], key + (r.cost, w["cost"])
    assert len(r.i) == len(w["i"]), key
    assert np.array_equal(r.i, w["i"]) and np.array_equal(r.j, w["j"]), key
    assert np.array_equal(bc.bits(r.difference), bc.bits(w["d"])), key
    return w


def test_grid_against_model_and_oracle(orc):
    """(n, m) in [1, 32]^2 x R in {0, 1, 2, 3, 5}, normal and three-valued signals: every job has a path, its cost is the oracle's banded
    cost, and the forward sum of the path's distances is the cost where the walk met no L == T < X tie"""
    cases = bc.grid_cases(bc.PLAIN, 32)
    assert len(cases) == 10240
    summed = 0
    for q, (a, b, R) in enumerate(cases):
        ex = q & 1
        w = hold(orc, a, b, R, ex, "grid")
        assert w["has_path"]
        assert bc.bits(w["cost"])[0] == bc.bits(orc.dtw_banded(a, b, R, ex))[0], (len(a), len(b), R, ex)
        if not ex:
            assert w["i"][0] == 0 and w["j"][0] == 0 and w["i"][-1] == len(a) - 1 and w["j"][-1] == len(b) - 1
        if not w["tie"]:   # (with exclude_last the popped last distance goes back on: the sum is the cost before the subtraction)
            summed += 1
            total = bc.forward_sum(w["d"])
            if ex:
                total = np.float32(total + np.abs(a[-1] - b[-1]).astype(np.float32))
            assert bc.bits(total)[0] == bc.bits(orc.dtw_banded(a, b, R, 0))[0], (len(a), len(b), R, ex)
    print("forward sums held: %d of %d" % (summed, len(cases)))
    assert summed >= 9000   # (ties are rare: normal signals have none, three-valued ones some)


def test_whole_matrix_band_is_global_tb(orc):
    """R = n + m: S is the whole matrix, cost and path are DTW_global_tb's"""
    for q, (a, b, R) in enumerate(bc.grid_cases(bc.PLAIN, 13, radii=(None,))):
        ex = q & 1
        _, cells, mask = orc.dtw_banded_cellset(a, b, R)
        assert cells == len(a) * len(b) and mask.all()
        c, pi, pj, pd = orc.dtw_global_tb(a, b, ex)
        r = ra.banded_tb_host(a, b, R, ex)
        assert bc.bits(r.cost)[0] == bc.bits(c)[0] and np.array_equal(r.i, pi) and np.array_equal(r.j, pj)
        assert np.array_equal(bc.bits(r.difference), bc.bits(pd))
    for n, m in ((1, 80), (80, 1), (80, 80), (37, 80)):
        z = np.zeros(1, np.float32)
        assert orc.dtw_banded_cellset(np.repeat(z, n), np.repeat(z, m), n + m)[2].all()


def test_above_1e10(orc):
    """sums pass 1e10: the cost is still the oracle's banded cost, the host restatement is still the model, and some walks leave S"""
    cases = bc.grid_cases(bc.BIG, 16) + [bc.SMALLEST_NO_PATH]
    none = 0
    for q, (a, b, R) in enumerate(cases):
        w = hold(orc, a, b, R, q & 1, "big")
        assert bc.bits(w["cost"])[0] == bc.bits(orc.dtw_banded(a, b, R, q & 1))[0]
        none += not w["has_path"]
    print("jobs without a path: %d of %d" % (none, len(cases)))
    assert none >= 20
    a, b, R = bc.SMALLEST_NO_PATH
    r = ra.banded_tb_host(a, b, R)
    assert len(r.i) == 0 and not bc.model(orc, a, b, R)["has_path"]
    assert bc.bits(r.cost)[0] == bc.bits(orc.dtw_banded(a, b, R))[0]


def test_one_by_two(orc):
    """a = [3e10], b = [0, 0], R = 1: the walk's i == 0 rule takes (0, 1) to (0, 0), both in S -- a path of two elements"""
    a, b, R = bc.ONE_BY_TWO
    w = hold(orc, a, b, R, 0, "1x2")
    assert w["has_path"] and w["i"].tolist() == [0, 0] and w["j"].tolist() == [0, 1]
    assert orc.dtw_banded_cellset(a, b, R)[2].all()
    assert bc.bits(w["cost"])[0] == bc.bits(orc.dtw_banded(a, b, R))[0]


def test_larger_shape(orc):
    rng = np.random.default_rng(300257)
    a, b = rng.normal(size=300).astype(np.float32), rng.normal(size=257).astype(np.float32)
    for x, y in ((a, b), (b, a)):
        for ex in (0, 1):
            w = hold(orc, x, y, 30, ex, "300x257")
            assert w["has_path"] and bc.bits(w["cost"])[0] == bc.bits(orc.dtw_banded(x, y, 30, ex))[0]


def test_refusals():
    one = np.zeros(1, np.float32)
    for a, b, R in ((one[:0], one, 1), (one, one[:0], 1), (one, one, -1)):
        with pytest.raises(ra.RawDTWError) as err:
            ra.banded_tb_host(a, b, R)
        assert err.value.status == 1
    for R in (bc.MAX_K, 1 << 20, 2 ** 31 - 1):   # a band wider than the device entry takes: a status, no allocation by the radius
        with pytest.raises(ra.RawDTWError) as err:
            ra.banded_tb_host(one, one, R)
        assert err.value.status == 5
    assert len(ra.banded_tb_host(one, one, bc.MAX_K - 1).i) == 1


def test_byte_model():
    """the layout's byte count: about (n + m) (K / 4 + 16) against n m / 4"""
    assert bc.slanted_radius(3000, 3000, 300) == 300 and bc.slanted_radius(3000, 2049, 300) == 396
    assert bc.dir_bytes(3000, 3000, 300) == 5999 * (16 + 5 * 16)
    assert bc.dir_bytes(1, 1, 0) == 32
    assert 3.5 < bc.full_matrix_dir_bytes(3000, 3000) / bc.dir_bytes(3000, 3000, 300) < 4.5
    jobs = np.zeros(5, ra.JOB_DTYPE)
    jobs["n"], jobs["m"], jobs["band_radius"] = 3000, 3000, 300
    assert bc.sub_batches(jobs, 1) == [1, 1, 1, 1, 1] and bc.sub_batches(jobs, 2) == [3, 2] and bc.sub_batches(jobs, 16) == [5]


def _ref_banded():
    import ctypes as C
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_dtw.so")
    if not os.path.exists(path):
        return None
    fn = C.CDLL(path)._Z41DTW_global_slantedbanded_antidiagonalwisePKfjS0_jib
    fn.restype = C.c_float
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_bool]
    return lambda a, b, R, ex: np.float32(fn(a.ctypes.data, len(a), b.ctypes.data, len(b), int(R), bool(ex)))


@pytest.mark.skipif(_ref_banded() is None, reason="oracle/_ref is built only where the reference's sources are")
def test_cost_is_the_live_references():
    ref = _ref_banded()
    for q, (a, b, R) in enumerate(bc.grid_cases(bc.PLAIN, 20, salt=1) + bc.grid_cases(bc.BIG, 12, salt=1)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert bc.bits(ra.banded_tb_host(a, b, R, q & 1).cost)[0] == bc.bits(ref(a, b, R, q & 1))[0], (len(a), len(b), R)
