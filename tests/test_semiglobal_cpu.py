"""Semiglobal DTW without a device: the numpy restatement (tests/semiglobal_cases.py) and the library's host restatement
(rawdtw_semiglobal_host, rawdtw_semiglobal_tb_host) against the answers recorded from the compiled reference
(tests/golden/semiglobal_ref.npz) and, where oracle/_ref exists, against the live reference on fresh inputs -- costs, end_j and whole
paths, bit for bit, for exclude_last 0 and 1.  DTW_semiglobal's own answer (its 1e10 sentinel) must equal the sentinel-free one
exactly where `sentinel_free` says so."""
import numpy as np
import pytest

import rawalign_amd as ra
from tests import semiglobal_cases as sc
from tests import value_cases as vc


@pytest.fixture(scope="module")
def fx():
    return sc.Fixture()


def test_fixture_is_the_generator_s(fx):
    cases = sc.fixture_cases()
    assert len(cases) == len(fx) >= 150
    for k, (tag, a, b) in enumerate(cases):
        fa, fb = fx.inputs(k)
        assert tag == fx.tag(k) and np.array_equal(sc.bits(a), sc.bits(fa)) and np.array_equal(sc.bits(b), sc.bits(fb)), k
    # the reference's three functions agree with one another as the restated semantics say
    z = fx.z
    assert np.array_equal(z["slow"], z["tb_cost"]) and np.array_equal(z["fast"][:, 0], z["fast"][:, 1])
    assert np.all(z["tb_len"][:, 1] == z["tb_len"][:, 0] - 1) and np.all(z["tb_len"][:, 0] <= z["n"] + z["m"] - 1)


def check_against_fixture(fx, k, ex, cost, end_j, pi, pj, pd, what):
    z = fx.z
    wi, wj, wd = fx.path(k, ex)
    assert sc.bits(cost)[0] == z["slow"][k, ex] == z["tb_cost"][k, ex], (what, k, ex, cost)
    assert end_j == z["end_j"][k], (what, k, ex)
    assert np.array_equal(pi, wi) and np.array_equal(pj, wj) and np.array_equal(sc.bits(pd), sc.bits(wd)), (what, k, ex)


def test_numpy_restatement_equals_fixture(fx):
    for k in range(len(fx)):
        a, b = fx.inputs(k)
        for ex in (0, 1):
            check_against_fixture(fx, k, ex, *sc.model(a, b, ex), "numpy")


def test_host_restatement_equals_fixture(fx):
    for k in range(len(fx)):
        a, b = fx.inputs(k)
        for ex in (0, 1):
            c, ej = ra.semiglobal_host(a, b, ex)
            r, ej2 = ra.semiglobal_host(a, b, ex, traceback=True)
            assert sc.bits(c)[0] == sc.bits(r.cost)[0] and ej == ej2
            check_against_fixture(fx, k, ex, r.cost, ej, r.i, r.j, r.difference, "host")


def test_sentinel_condition_on_fixture(fx):
    """DTW_semiglobal equals the sentinel-free recurrence on every case `sentinel_free` admits; each domain that is compared with all three
    functions has such cases, and the sentinel domains have cases where it does differ (so the split is not vacuous)"""
    free, differs = {}, {}
    for k in range(len(fx)):
        a, b = fx.inputs(k)
        same = fx.z["fast"][k, 0] == fx.z["slow"][k, 0]
        if sc.sentinel_free(a, b):
            assert same, (k, fx.tag(k))
            free[fx.tag(k)] = free.get(fx.tag(k), 0) + 1
        elif not same:
            differs[fx.tag(k)] = differs.get(fx.tag(k), 0) + 1
    assert all(free.get(d, 0) >= 3 for d in sc.ALL_THREE), free
    assert all(differs.get(d, 0) >= 3 for d in vc.SENTINEL_DOMAINS), differs


def test_host_refuses_bad_arguments():
    a = np.zeros(3, np.float32)
    for x, y in ((a[:0], a), (a, a[:0])):
        with pytest.raises(ra.RawDTWError) as e:
            ra.semiglobal_host(x, y)
        assert e.value.status == 1


@pytest.mark.skipif(not sc.RefSemiglobal.available(), reason="oracle/_ref is built only where the reference's sources are")
def test_restatements_equal_live_reference():
    ref = sc.RefSemiglobal()
    rng = np.random.default_rng(4242)
    n_free = 0
    for t in range(300):
        n, m = int(rng.integers(1, 70)), int(rng.integers(1, 110))
        if t % 5 == 0:
            n, m = m, max(1, n // 4)  # n > m
        if t % 2:
            a, b = rng.integers(-2, 3, n).astype(np.float32), rng.integers(-2, 3, m).astype(np.float32)  # ties
        else:
            a, b = rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32)
        for ex in (0, 1):
            slow = ref.slow(a, b, ex)
            c, pi, pj, pd = ref.tb(a, b, ex)
            assert sc.bits(slow)[0] == sc.bits(c)[0]
            mc, mej, mi, mj, md = sc.model(a, b, ex)
            r, ej = ra.semiglobal_host(a, b, ex, traceback=True)
            for what, (gc, gi, gj, gd) in (("numpy", (mc, mi, mj, md)), ("host", (r.cost, r.i, r.j, r.difference))):
                assert sc.bits(gc)[0] == sc.bits(c)[0], (what, t, ex)
                assert np.array_equal(gi, pi) and np.array_equal(gj, pj) and np.array_equal(sc.bits(gd), sc.bits(pd)), (what, t, ex)
            assert ej == mej and (ex or len(pj) == 0 or pj[-1] == ej)
        if sc.sentinel_free(a, b):
            n_free += 1
            assert sc.bits(ref.semiglobal(a, b))[0] == sc.bits(ref.slow(a, b, 0))[0]
    assert n_free == 300  # (unit-scale inputs: far below the sentinel)
