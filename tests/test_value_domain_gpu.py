"""Every DTW body of the HIP path on the value domains of tests/value_cases.py, bit for bit against the oracle (which
tests/test_value_domain.py pins to the compiled reference on the same domains): costs below, around and far above the banded
DP's 1e10 literal, subnormals, zeros of either sign, integers -- and the accept/cut comparisons met exactly.

The shapes are the smallest that still reach each body: the lane and micro bodies, the lane / wave hand-over, a band of
K = R + 1 slots on both sides of every register layout of the wave-per-job bodies, every rows-per-lane class of the full
matrix with the four-wave pipeline, the traceback fill and walk, and the sync-free batch path with its carried rounds."""
import ctypes as C

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch

    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import rawalign_amd as ra
from rawalign_amd.align import CandidateBatch
from tests import value_cases as vc
from tests.golden_util import bits
from tests.test_chunk_classes import _batch, _tile
from tests.test_stream_path import _chains, _degenerate, _match, _medium, _oracle_check, _sprinkled, _tiny, _two_rounds, _wide
from tests.util import assert_bits_equal, default_radius, make_arena_jobs, oracle_costs, planner_options

pytestmark = pytest.mark.gpu

REF_LEN = 60000


@pytest.fixture(scope="module")
def engine():
    eng = ra.Engine(0)
    yield eng
    eng.close()


def run(engine, jobs, events, ref):
    pad = np.zeros(8, np.float32)
    engine.upload_reference([np.concatenate([ref, pad])], [np.concatenate([ref, pad])])
    jobs = jobs.copy()
    jobs["ref_off"] += engine.reference_offset(0, 1)
    return engine.score_batch(jobs, events)


def check_jobs(engine, oracle, cases, what):
    jobs, ev, rf = make_arena_jobs(cases)
    n, m = max(len(a) for a, _, _, _ in cases), max(len(b) for _, b, _, _ in cases)
    assert vc.sums_stay_finite((ev, rf), n, m)
    want = oracle_costs(oracle, jobs, ev, rf)
    assert np.all(np.isfinite(want))
    assert_bits_equal(run(engine, jobs, ev, rf), want, what)


# ------------------------------------------------------------------------------------------------
# the job-list path (rawdtw_score_batch)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.DOMAIN_NAMES)
def test_lane_and_micro_bodies(engine, oracle, name):
    rng, draw = vc.domain_rng(name, 1), vc.DOMAINS[name]
    cases = []
    for t in range(400):
        n = int(rng.integers(1, 131))
        m = max(1, int(round(n * rng.uniform(0.3, 1.6))))
        R0 = default_radius(n) if t % 3 else int(rng.integers(0, 9))
        cases.append((draw(rng, n), draw(rng, m), R0, (t >> 1) & 1))
    check_jobs(engine, oracle, cases, f"{name}: lane and micro bodies")


WAVE_K = (64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 448, 449, 512, 513, 1025, 2049)
SLANTED_K = (150, 193, 321, 449, 512)


@pytest.mark.parametrize("name", vc.DOMAIN_NAMES)
def test_wave_per_job_bands(engine, oracle, name):
    """the lane / wave hand-over radii, then bands of K = R + 1 slots on both sides of every register layout (one register a
    lane up to 64 slots, two up to 128, three, five, seven, nine, the register-only body beyond), square and slanted"""
    rng, draw = vc.domain_rng(name, 2), vc.DOMAINS[name]
    cases = [(draw(rng, 150), draw(rng, 140), R0, R0 & 1) for R0 in range(5, 16)]
    for K in WAVE_K:
        n = int(1.6 * K) + 7
        cases.append((draw(rng, n), draw(rng, n), K - 1, K & 1))
    for K in SLANTED_K:
        n = 2300 + K
        m = n - n // 10
        r0 = max(r for r in range(1, K) if r + ((n - m) * r + n - 1) // n + 1 <= K)  # (the radius that the slant of m = 0.9 n widens to K slots: dtw.cpp:298-300)
        cases.append((draw(rng, n), draw(rng, m), r0, K & 1))
        cases.append((draw(rng, m), draw(rng, n), r0, 1 - (K & 1)))
    check_jobs(engine, oracle, cases, f"{name}: wave-per-job bands")


FULL_SHAPES = ((1, 1), (2, 2), (1, 50), (50, 1), (63, 64), (65, 64), (129, 300), (257, 256), (513, 514), (700, 520), (1537, 1536), (3000, 2049))


@pytest.mark.parametrize("name", vc.DOMAIN_NAMES)
def test_full_matrix(engine, oracle, name):
    """DTW_global (dtw.cpp:37-66) has no sentinel: row 0 and column 0 are running sums, whatever they pass.  Every
    rows-per-lane class and the four-wave pipeline.

    Before the borders of k_full_wave read as +inf (they read as 1e10) this failed on s9, s3e9, s10, s12, s30, cross and
    spike -- see the measured counts in DESIGN.md section 5."""
    rng, draw = vc.domain_rng(name, 3), vc.DOMAINS[name]
    cases = [(draw(rng, n), draw(rng, m), -1, ex) for n, m in FULL_SHAPES for ex in (0, 1)]
    check_jobs(engine, oracle, cases, f"{name}: full matrix")


TB_SHAPES = ((1, 1), (1, 7), (7, 1), (30, 20), (65, 100), (130, 129), (260, 300), (600, 513), (1100, 2600))


@pytest.mark.parametrize("name", vc.DOMAIN_NAMES)
def test_traceback(engine, oracle, name):
    """DTW_global_tb (dtw.cpp:595-667): cost, path and distances"""
    rng, draw = vc.domain_rng(name, 4), vc.DOMAINS[name]
    cases = [(draw(rng, n), draw(rng, m), -1, k & 1) for k, (n, m) in enumerate(TB_SHAPES)]
    jobs, ev, rf = make_arena_jobs(cases)
    assert vc.sums_stay_finite((ev, rf), 1100, 2600)
    engine.upload_reference([rf], [rf])
    jobs["ref_off"] += engine.reference_offset(0, 1)
    res = engine.traceback_batch(jobs, ev)
    bad = []
    for (a, b, _, ex), r in zip(cases, res):
        c, pi, pj, pd = oracle.dtw_global_tb(a, b, ex)
        ok = (bits(r.cost) == bits(c) and np.array_equal(r.i, pi) and np.array_equal(r.j, pj)
              and np.array_equal(r.difference.view(np.uint32), pd.view(np.uint32)))
        if not ok:
            bad.append((len(a), len(b), ex, float(r.cost), float(c)))
    assert not bad, f"{name}: {len(bad)} of {len(cases)} tracebacks differ: {bad}"


# ------------------------------------------------------------------------------------------------
# the sync-free path (rawdtw_batch_create planned on the device)
# ------------------------------------------------------------------------------------------------
def _reference(rng, draw, ref_len=REF_LEN):
    return [draw(rng, ref_len), draw(rng, ref_len)]


def _run_batch(engine, oracle, ref, arrays, min_score=5.0):
    events, chain_off, anchor_off, anchors, slot, read_base = arrays
    engine.upload_reference([ref[0]], [ref[1]])
    strand_of = [1 if s == 0 else 0 for s in slot]  # slot 0 = forward array (strand 1, rmap.cpp:182-188)
    ref_base = np.array([engine.reference_offset(0, st) for st in strand_of], np.uint64)
    cb = CandidateBatch(events, chain_off, anchor_off, anchors, ref_base, read_base)
    engine.upload_events(events)
    opt = ra.MapOpt(dtw_min_score=min_score)
    b = ra.Batch(engine, opt, cb)
    try:
        assert b.verify_plan() is True  # the sync-free path took the batch, and its records pass the self-check
        b.run()
        score, keep, jc = b.fetch(with_job_costs=True)
        assert np.all(np.isfinite(jc)) and np.all(np.isfinite(score))
        _oracle_check(oracle, cb, {1: ref[0], 0: ref[1]}, strand_of, score, keep, jc, opt)
        return b.info()
    finally:
        b.close()


@pytest.mark.parametrize("shapes", [_tiny, _medium, _sprinkled, _degenerate, _wide], ids=lambda f: f.__name__.lstrip("_"))
@pytest.mark.parametrize("name", vc.DOMAIN_NAMES)
def test_stream_path_shapes(engine, oracle, name, shapes):
    rng, draw = vc.domain_rng(name, 10 + [_tiny, _medium, _sprinkled, _degenerate, _wide].index(shapes)), vc.DOMAINS[name]
    ref = _reference(rng, draw)
    assert vc.sums_stay_finite(ref, 401 * 40, 641 * 40)  # (a chain's sum of up to 40 parts included)
    _run_batch(engine, oracle, ref, _chains(rng, 120, REF_LEN, shapes, draw=draw))


@pytest.mark.parametrize("name", vc.DOMAIN_NAMES)
def test_tile_of_exact_composition(engine, oracle, name):
    """the lane bodies of radius 1 and 2 and the quads of radius 3 in one tile of 17 + 65 + 127 parts behind a full tile of
    radius 1 (tests/test_chunk_classes.py)"""
    rng, draw = vc.domain_rng(name, 20), vc.DOMAINS[name]
    ref = _reference(rng, draw)
    chains = [_tile(0, 0, 512, seed=3), _tile(17, 65, 127, seed=22)]
    info = _run_batch(engine, oracle, ref, _batch(chains, draw=draw))
    assert info["n_jobs"] == 512 + 17 + 65 + 127


# (dq, dt) whose radius puts K = R + 1 on both sides of every change of k_wide's register layout: the list of
# tests/test_stream_path.py::test_wave_per_job_bands_at_the_register_layouts_edges
WIDE_EDGES = [(629, 629), (639, 639), (571, 630), (1269, 1269), (1279, 1279), (1160, 1280), (2549, 2549), (2320, 2570), (700, 630), (1915, 1915),
              (1925, 1925), (1740, 1926)]


@pytest.mark.parametrize("name", vc.DOMAIN_NAMES)
def test_wide_bands_at_the_register_layouts_edges(engine, oracle, name):
    rng, draw = vc.domain_rng(name, 21), vc.DOMAINS[name]
    ref = _reference(rng, draw)
    assert vc.sums_stay_finite(ref, 2600 * 14, 2600 * 14)
    state = {"k": 0}

    def shapes(r):
        state["k"] += 1
        return WIDE_EDGES[(state["k"] // 9) % len(WIDE_EDGES)] if state["k"] % 9 == 4 else _tiny(r)
    info = _run_batch(engine, oracle, ref, _chains(rng, 40, REF_LEN, shapes, (1, 14), draw=draw))
    assert info["n_wave_band_jobs"] >= len(WIDE_EDGES)


@pytest.mark.parametrize("name", ["s10", "spike", "sub41"])
def test_carried_round(oracle, name):
    """rawdtw_batch_submit_carry: the device takes a former last part's last distance off the carried cost (a subtraction of
    values around the fill value, or of subnormals).  Costs, scores and keeps equal the from-scratch batch of round 2, and
    that batch equals the oracle."""
    rng, draw = vc.domain_rng(name, 30), vc.DOMAINS[name]
    ref = _reference(rng, draw, 90000)
    eng = ra.Engine(0)
    try:
        eng.upload_reference([ref[0]], [ref[1]])
        lib = eng.lib
        cb1, cb2, prev_read, expect = _two_rounds(rng, eng, n_reads=60, draw=draw)
        nc = cb2.n_chains
        eng.upload_events(cb2.events)
        opt = ra.MapOpt(dtw_min_score=5.0)
        copt = opt.c_struct()
        vp = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
        b1 = ra.Batch(eng, opt, cb1)
        b1.run()
        b1.fetch()
        assert lib.rawdtw_batch_can_carry(eng._ctx, b1._h, C.byref(copt)) == 1
        plain = ra.Batch(eng, opt, cb2)
        assert plain.verify_plan() is True
        plain.run()
        want = plain.fetch(with_job_costs=True)
        plain.close()
        slot_of = {eng.reference_offset(0, 1): 1, eng.reference_offset(0, 0): 0}
        _oracle_check(oracle, cb2, {1: ref[0], 0: ref[1]}, [slot_of[int(x)] for x in cb2.ref_base], want[0], want[1], want[2], opt)
        arr, carry, new_off, new_anchors = _match(lib, cb2, cb1, prev_read)
        assert np.array_equal(carry["parts"].astype(np.int64), expect) and int(expect.sum()) > 200
        h = C.c_void_p()
        eng._check(lib.rawdtw_batch_submit_carry(eng._ctx, C.byref(copt), cb2.n_reads, vp(arr[0]), vp(arr[1]), vp(arr[2]), vp(new_off), vp(new_anchors),
                                                 vp(arr[3]), vp(arr[4]), b1._h, vp(carry), C.byref(h)))
        score, keep, jc = np.zeros(nc, np.float32), np.zeros(nc, np.uint8), np.zeros(len(want[2]), np.float32)
        eng._check(lib.rawdtw_batch_fetch(eng._ctx, h, vp(score), vp(keep), vp(jc)))
        sc, ru = C.c_uint64(), C.c_uint64()
        eng._check(lib.rawdtw_batch_round_stats(eng._ctx, h, C.byref(sc), C.byref(ru)))
        lib.rawdtw_batch_destroy(h)
        b1.close()
        assert ru.value == int(expect.sum())  # (the parts were taken over, not scored again)
        assert_bits_equal(jc, want[2], f"{name}: carried part costs")
        assert_bits_equal(score, want[0], f"{name}: carried scores")
        assert np.array_equal(keep, want[1])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------
# thresholds met exactly
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def threshold(oracle):
    """the batch of value_cases.threshold_batch and the oracle's sequential loop over it (rmap.cpp:515-524): scores, keeps"""
    from oracle.loader import OrcOpt

    batch = vc.threshold_batch()
    events, ref, chain_off, anchor_off, anchors, read_base = batch
    oopt = OrcOpt(1, 1, 0.10, vc.THRESHOLD_BONUS, vc.THRESHOLD_MIN_SCORE, 1)
    score, keep = np.zeros(len(anchor_off) - 1, np.float32), np.zeros(len(anchor_off) - 1, np.uint8)
    for r in range(len(chain_off) - 1):
        best = np.float32(0.0)
        for c in range(int(chain_off[r]), int(chain_off[r + 1])):
            a = anchors[int(anchor_off[c]):int(anchor_off[c + 1])]
            s = oracle.align_chain(a, ref, events[int(read_base[c]):], oopt, float(best))
            score[c], keep[c] = s, s >= np.float32(vc.THRESHOLD_MIN_SCORE)
            if keep[c] and s > best:
                best = s
    assert keep.any() and not keep.all() and np.any(score == np.float32(-1e10))
    return batch, score, keep


@pytest.mark.parametrize("device_plan", [0, 1])
def test_thresholds_met_exactly(engine, threshold, device_plan):
    """gate == best is not cut and gate == best - 0.5 is, score == min_score is kept and score == min_score - 0.5 is not
    (tests/test_value_domain.py counts them) -- in k_read_select, k_fold_select and the host replay, under every fold form,
    with the final score fused or not (exact arithmetic: both give the same number)."""
    (events, ref, chain_off, anchor_off, anchors, read_base), want_score, want_keep = threshold
    engine.upload_reference([ref], [ref[::-1].copy()])
    ref_base = np.full(len(anchor_off) - 1, engine.reference_offset(0, 1), np.uint64)
    cb = CandidateBatch(events, chain_off, anchor_off, anchors, ref_base, read_base)
    engine.upload_events(events)
    try:
        with planner_options(engine, device_plan=device_plan, device_plan_min_jobs=0):
            for fold_mode in range(5):
                engine.set_option("fold_mode", fold_mode)
                for fused in (False, True):
                    opt = ra.MapOpt(dtw_match_bonus=vc.THRESHOLD_BONUS, dtw_min_score=vc.THRESHOLD_MIN_SCORE, fused_score=fused)
                    b = ra.Batch(engine, opt, cb)
                    assert b.verify_plan() is bool(device_plan)
                    b.run()
                    score, keep = b.fetch()
                    b.close()
                    assert_bits_equal(score, want_score, f"device_plan {device_plan}, fold_mode {fold_mode}, fused {fused}: scores")
                    bad = np.nonzero(keep != want_keep)[0]
                    assert len(bad) == 0, (device_plan, fold_mode, fused, bad[:5], score[bad[:5]], want_score[bad[:5]])
    finally:
        engine.set_option("fold_mode", ra.DEFAULT_FOLD_MODE)
