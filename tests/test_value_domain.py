"""The oracle on the value domains of tests/value_cases.py against the compiled reference's recorded answers
(tests/golden/dtw_ref_values.npz, scripts/make_golden_values.py), and the proof that those domains can tell a right DTW body
from a subtly wrong one: two plain numpy DPs, each once with the reference's neutral value and once with the other.

  full DP (dtw.cpp:37-66, 595-667): no sentinel -- row 0 and column 0 are running sums.  A body that reads the virtual
  borders as 1e10 differs as soon as a border sum passes 1e10; with +inf borders it is the reference.
  banded DP (dtw.cpp:273-520): every guarded or clipped neighbour is the literal 1e10, which wins the min once costs pass
  it.  Over the band's cell set with 1e10 outside it is the reference; with +inf outside it differs.

Then the accept/cut thresholds met exactly (value_cases.threshold_batch): the plain-Python model against the oracle's
align_chain and the library's host replay, with counters that show every equality and every near miss is there."""
import ctypes as C

import numpy as np
import pytest

from tests import value_cases as vc
from tests.golden_util import bits, golden_path, path_digest

INF = np.float32(np.inf)
FILL = np.float32(1e10)


@pytest.fixture(scope="module")
def fixture():
    return np.load(golden_path("dtw_ref_values.npz"))


@pytest.fixture(scope="module")
def cases():
    return {name: vc.fixture_cases(name) for name in vc.DOMAIN_NAMES}


def model_dp(a, b, exclude_last, absent, mask=None):
    """cell = min3(top, left, topleft) + |a_i - b_j| in float32, antidiagonal by antidiagonal; every neighbour that is not a
    cell -- beyond the matrix, or outside `mask` -- reads as `absent`; the corner's topleft is 0."""
    n, m = len(a), len(b)
    D = np.full((n + 1, m + 1), absent, np.float32)
    D[0, 0] = 0.0
    for k in range(n + m - 1):
        i = np.arange(max(0, k - m + 1), min(n - 1, k) + 1)
        j = k - i
        v = np.minimum(np.minimum(D[i, j + 1], D[i + 1, j]), D[i, j]) + np.abs(a[i] - b[j])
        if mask is not None:
            v = np.where(mask[i, j], v, absent)
        D[i + 1, j + 1] = v
    cost = D[n, m]
    return np.float32(cost - np.abs(a[-1] - b[-1])) if exclude_last else np.float32(cost)


def band_mask(oracle, a, b, R0):
    """the band's cell set, rows over a (the oracle lays it longer side first)"""
    _, _, mask = oracle.dtw_banded_cellset(a, b, R0)
    return mask.astype(bool) if len(a) >= len(b) else mask.astype(bool).T


def test_inputs_are_those_the_answers_were_recorded_for(fixture, cases):
    assert vc.inputs_sha256(cases) == fixture["inputs_sha256"].tobytes(), "the seeded inputs differ from those the answers were recorded for"
    for name in vc.DOMAIN_NAMES:
        assert len(cases[name]) == vc.N_FIXTURE_CASES
        assert {ex for _, _, ex in cases[name]} == {0, 1}
        for a, b, _ in cases[name]:
            assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
            assert vc.sums_stay_finite((a, b), len(a), len(b))
    tiny = float(np.finfo(np.float32).tiny)
    for name in ("sub38", "sub41", "sub44"):  # subnormal inputs; at 1e-38 the sums cross into the normal range, below it they never do
        xs = np.concatenate([x for a, b, _ in cases[name] for x in (a, b)])
        assert np.mean((xs != 0) & (np.abs(xs) < tiny)) > (0.5 if name == "sub38" else 0.9)
        assert name == "sub38" or float(np.max(np.abs(xs))) * 240 < tiny
    assert all(np.all(x == 0) for a, b, _ in cases["zeros"] for x in (a, b))
    assert any(np.any(np.signbit(x)) and not np.all(np.signbit(x)) for a, _, _ in cases["zeros"] for x in (a,))


@pytest.mark.parametrize("name", vc.DOMAIN_NAMES)
def test_oracle_equals_the_compiled_reference(oracle, fixture, cases, name):
    from oracle.loader import RefDTW

    d = vc.DOMAIN_NAMES.index(name)
    ref = RefDTW() if RefDTW.available() else None
    for t, (a, b, ex) in enumerate(cases[name]):
        g = bits(oracle.dtw_global(a, b, ex))
        assert g == int(fixture["global_"][d, t]), (name, t)
        for k, R in enumerate(vc.fixture_radii(len(a))):
            bd = bits(oracle.dtw_banded(a, b, R, ex))
            assert bd == int(fixture["banded"][d, t, k]), (name, t, R)
            if ref is not None:
                assert bd == bits(ref.dtw_banded(a, b, R, ex)), (name, t, R)
        if ref is not None:
            assert g == bits(ref.dtw_global(a, b, ex)), (name, t)
        if t % vc.TB_EVERY == 0:
            k = t // vc.TB_EVERY
            c1, i1, j1, d1 = oracle.dtw_global_tb(a, b, ex)
            assert bits(c1) == int(fixture["tb_cost"][d, k]) and len(i1) == int(fixture["tb_len"][d, k]), (name, t)
            assert path_digest(i1, j1, d1) == fixture["tb_digest"][d, k].tobytes(), (name, t)
            if ref is not None:
                c2, i2, j2, d2 = ref.dtw_global_tb(a, b, ex)
                assert bits(c1) == bits(c2) and np.array_equal(i1, i2) and np.array_equal(j1, j2)
                assert np.array_equal(d1.view(np.uint32), d2.view(np.uint32))
    if name == "zeros":  # every cost is +0.0
        assert not fixture["global_"][d].any() and not fixture["banded"][d].any() and not fixture["tb_cost"][d].any()


@pytest.mark.parametrize("name", vc.DOMAIN_NAMES)
def test_domains_separate_a_right_body_from_a_wrong_one(oracle, fixture, cases, name):
    """The right model equals the reference on every case of every domain; on the domains of scale >= 3e9 the wrong one
    differs on at least half of the cases (if a case set falls below that, its shapes change, not the bound)."""
    d = vc.DOMAIN_NAMES.index(name)
    full_wrong = band_wrong = 0
    for t, (a, b, ex) in enumerate(cases[name]):
        want_full, want_band = int(fixture["global_"][d, t]), int(fixture["banded"][d, t, 0])
        assert bits(model_dp(a, b, ex, INF)) == want_full, (name, t)
        mask = band_mask(oracle, a, b, vc.fixture_radii(len(a))[0])
        assert bits(model_dp(a, b, ex, FILL, mask)) == want_band, (name, t)
        full_wrong += bits(model_dp(a, b, ex, FILL)) != want_full
        band_wrong += bits(model_dp(a, b, ex, INF, mask)) != want_band
    print(f"{name}: 1e10 borders change {full_wrong} of {vc.N_FIXTURE_CASES} full costs, +inf outside the band changes {band_wrong} banded costs")
    if name in vc.SENTINEL_DOMAINS:
        assert 2 * full_wrong >= vc.N_FIXTURE_CASES and 2 * band_wrong >= vc.N_FIXTURE_CASES
    if name in ("sub38", "sub41", "sub44", "zeros", "ints"):
        assert full_wrong == 0 and band_wrong == 0  # (costs far below 1e10: the neutral value never decides)


# ------------------------------------------------------------------------------------------------
# thresholds met exactly
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def threshold(oracle):
    batch = vc.threshold_batch()
    costs = vc.threshold_part_costs(oracle, batch)
    return batch, costs, vc.threshold_model(batch, costs)


def test_threshold_batch_meets_every_comparison_exactly(threshold):
    batch, costs, model = threshold
    assert len(batch[2]) - 1 == 600 and len(model) == 2400
    step = vc.THRESHOLD_BONUS
    tied_gate = sum(1 for x in model if x["best"] > 0 and x["gate"] == x["best"])
    near_gate = sum(1 for x in model if x["best"] > 0 and x["gate"] == x["best"] - step)
    on_min = sum(1 for x in model if x["score"] == vc.THRESHOLD_MIN_SCORE)
    under_min = sum(1 for x in model if x["score"] == vc.THRESHOLD_MIN_SCORE - step)
    tied_best = sum(1 for x in model if not x["cut"] and x["best"] > 0 and x["score"] == x["best"])
    print(f"gate == best {tied_gate}, gate == best - {step} {near_gate}, score == min_score {on_min}, score == min_score - {step} {under_min}, "
          f"score == best {tied_best}")
    assert min(tied_gate, near_gate, on_min, under_min) >= 10
    for x in model:
        assert x["cut"] == (x["gate"] < x["best"])  # costs are not negative: the last test is the one that decides
        if x["best"] > 0 and x["gate"] == x["best"]:
            assert not x["cut"]
        if x["best"] > 0 and x["gate"] == x["best"] - step:
            assert x["cut"] and x["score"] == -1e10 and not x["keep"]
        if x["score"] == vc.THRESHOLD_MIN_SCORE:
            assert x["keep"]
        if x["score"] == vc.THRESHOLD_MIN_SCORE - step:
            assert not x["keep"]


@pytest.mark.parametrize("fused", [0, 1])
def test_threshold_model_equals_align_chain(oracle, threshold, fused):
    from oracle.loader import OrcOpt

    (events, ref, chain_off, anchor_off, anchors, read_base), _, model = threshold
    oopt = OrcOpt(1, 1, 0.10, vc.THRESHOLD_BONUS, vc.THRESHOLD_MIN_SCORE, fused)
    for c, x in enumerate(model):
        a = anchors[int(anchor_off[c]):int(anchor_off[c + 1])]
        got = oracle.align_chain(a, ref, events[int(read_base[c]):], oopt, x["best"])
        assert bits(got) == bits(np.float32(x["score"])), (c, got, x)
        assert bool(got >= np.float32(vc.THRESHOLD_MIN_SCORE)) == x["keep"]


@pytest.mark.parametrize("fused", [0, 1])
def test_threshold_model_equals_batch_replay(threshold, fused):
    from rawalign_amd._lib import AlignOpt, load_library

    (events, ref, chain_off, anchor_off, anchors, read_base), costs, model = threshold
    lib = load_library()
    opt = AlignOpt(1, 1, 0.10, vc.THRESHOLD_BONUS, vc.THRESHOLD_MIN_SCORE, fused)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    job_off = np.concatenate([[0], np.cumsum([len(x) for x in costs])]).astype(np.uint64)
    cost = np.concatenate(costs).astype(np.float32)
    anchors = np.ascontiguousarray(anchors)
    nc = len(model)
    score, keep = np.zeros(nc, np.float32), np.zeros(nc, np.uint8)
    assert lib.rawdtw_batch_replay(C.byref(opt), len(chain_off) - 1, p(chain_off), p(anchor_off), p(anchors), p(job_off), p(cost),
                                   p(score), p(keep)) == 0
    want = np.array([x["score"] for x in model], np.float32)
    assert np.array_equal(score.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(keep.astype(bool), np.array([x["keep"] for x in model]))
