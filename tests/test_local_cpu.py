"""The local border constraint on the host (include/rawdtw.h, "local border"): rawdtw_chain_job_count / _build_jobs / _replay and the batch
forms for border_constraint == 2 against the numpy restatement (tests/local_cases.py) and the recorded answers of the reference's own
DTW_semiglobal_slow / DTW_semiglobal_tb (tests/golden/local_ref.npz); a scorer-only mapper; the Python option record; and the premise of the
GPU property test, fixed here.  No device."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapper, synth
from rawalign_amd._lib import AlignOpt, load_library
from rawalign_amd.dtw import ANCHOR_DTYPE, JOB_DTYPE
from rawalign_amd.mapping import StopOpt
from tests import local_cases as lc
from tests import semiglobal_cases as sc
from tests.util import assert_bits_equal


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def case():
    return lc.make_case()


@pytest.fixture(scope="module")
def fx(case):
    f = lc.Fixture()
    assert f.same_inputs(case), "rawalign_amd/synth.py or tests/local_cases.py drifted: regenerate with scripts/make_golden_local.py"
    return f


def test_the_restatement_equals_the_references_own_functions_on_every_chain(case, fx):
    cb = case.cb
    assert cb.n_chains == len(fx.z["slow"]) >= 24
    assert_bits_equal(lc.job_costs(cb, case.arena), fx.z["slow"].view(np.float32), "DTW_semiglobal_slow")
    assert np.array_equal(fx.z["slow"], fx.z["tb_cost"])   # (the cost bits of the CIGAR are the score-only job's)
    for c in range(cb.n_chains):
        a, b, s, e = lc.windows(cb, case.arena, c)
        cost, pi, pj, pd, j0, end_j = lc.cigar(a, b, s)
        wi, wj, wd = fx.path(c)
        assert sc.bits(cost)[0] == fx.z["tb_cost"][c] and j0 == fx.z["j0"][c] and end_j == fx.z["end_j"][c]
        assert np.array_equal(pi, wi + np.uint64(s["query_position"])) and np.array_equal(pj, wj + np.uint64(s["target_position"]))
        assert_bits_equal(pd, wd, "path differences of chain %d" % c)
        # the first element is (s.q, s.t + j0), the last (e.q, s.t + end_j)
        assert (int(pi[0]), int(pj[0])) == (int(s["query_position"]), int(s["target_position"]) + j0)
        assert (int(pi[-1]), int(pj[-1])) == (int(e["query_position"]), int(s["target_position"]) + end_j)


def test_job_count_and_jobs_for_border_2(case):
    lib, cb = load_library(), case.cb
    want, want_off = lc.jobs(cb)
    for fill in (0, 1):   # (fill_method and band_radius_frac are not looked at)
        opt = AlignOpt(2, fill, 0.25, 0.4, 20.0, 1)
        assert lib.rawdtw_chain_job_count(C.byref(opt), 0) == 0
        for na in (1, 2, 7):
            assert lib.rawdtw_chain_job_count(C.byref(opt), na) == 1
        for cigar in (0, 1):
            for c in range(cb.n_chains):
                a = np.ascontiguousarray(cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])], ANCHOR_DTYPE)
                j = np.zeros(1, JOB_DTYPE)
                assert lib.rawdtw_chain_build_jobs(C.byref(opt), _p(a), len(a), int(cb.ref_base[c]), int(cb.read_base[c]), cigar, _p(j)) == 0
                assert j.tobytes() == want[c:c + 1].tobytes(), (fill, cigar, c, j, want[c])
        job_off, nj = np.zeros(cb.n_chains + 1, np.uint64), C.c_uint64()
        jobs = np.zeros(len(want), JOB_DTYPE)
        args = (C.byref(opt), cb.n_chains, _p(cb.anchor_off), _p(cb.anchors), _p(cb.ref_base), _p(cb.read_base), _p(job_off))
        assert lib.rawdtw_batch_build_jobs(*args, _p(jobs), len(jobs), C.byref(nj)) == 0
        assert nj.value == len(want) and np.array_equal(job_off, want_off) and jobs.tobytes() == want.tobytes()
    for bad in (3, -1):   # any other value is refused as before
        opt = AlignOpt(bad, 0, 0.1, 0.4, 20.0, 1)
        a, j = np.zeros(2, ANCHOR_DTYPE), np.zeros(1, JOB_DTYPE)
        assert lib.rawdtw_chain_build_jobs(C.byref(opt), _p(a), 2, 0, 0, 0, _p(j)) == 1


def test_one_anchor_and_empty_chains():
    lib = load_library()
    opt = AlignOpt(2, 1, 0.1, 0.4, 20.0, 1)
    a = np.array([(7, 3)], ANCHOR_DTYPE)
    j = np.zeros(1, JOB_DTYPE)
    assert lib.rawdtw_chain_build_jobs(C.byref(opt), _p(a), 1, 100, 10, 0, _p(j)) == 0
    assert j.tobytes() == np.array([(107, 13, 1, 1, -1, 0, 0)], JOB_DTYPE).tobytes()
    # a batch with an empty chain in the middle: no job for it, score 0
    anchors = np.array([(9, 5), (4, 2), (30, 8), (30, 8)], ANCHOR_DTYPE)
    aoff, coff = np.array([0, 2, 2, 4], np.uint64), np.array([0, 3], np.uint64)
    rb, qb = np.zeros(3, np.uint64), np.zeros(3, np.uint32)
    job_off, nj, jobs = np.zeros(4, np.uint64), C.c_uint64(), np.zeros(2, JOB_DTYPE)
    assert lib.rawdtw_batch_build_jobs(C.byref(opt), 3, _p(aoff), _p(anchors), _p(rb), _p(qb), _p(job_off), _p(jobs), 2, C.byref(nj)) == 0
    assert nj.value == 2 and job_off.tolist() == [0, 1, 1, 2] and jobs["n"].tolist() == [4, 1] and jobs["m"].tolist() == [6, 1]


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("min_score", [20.0, 5.0, -50.0])
def test_replay_for_border_2_against_the_restatement_and_the_fixture(case, fx, fused, min_score):
    lib, cb = load_library(), case.cb
    opt = AlignOpt(2, 1, 0.1, 0.4, min_score, fused)
    mo = ra.MapOpt(dtw_border_constraint=2, dtw_min_score=min_score, fused_score=bool(fused))
    costs = fx.z["slow"].view(np.float32).copy()
    want_score, want_keep = lc.fold(cb, costs, mo)
    _, job_off = lc.jobs(cb)
    score, keep = np.zeros(cb.n_chains, np.float32), np.zeros(cb.n_chains, np.uint8)
    assert lib.rawdtw_batch_replay(C.byref(opt), cb.n_reads, _p(cb.chain_off), _p(cb.anchor_off), _p(cb.anchors), _p(job_off), _p(costs), _p(score),
                                   _p(keep)) == 0
    assert_bits_equal(score, want_score, "scores")
    assert np.array_equal(keep, want_keep)
    assert 0 < keep.sum() < cb.n_chains and (score == np.float32(-1e10)).any()   # (both outcomes, and the early exit against a read's running best)
    lib.rawdtw_chain_replay.restype = C.c_float
    for c in range(cb.n_chains):   # a chain alone: the global branch's early exit against a running best
        a = np.ascontiguousarray(cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])], ANCHOR_DTYPE)
        n = int(a[0]["query_position"]) - int(a[-1]["query_position"]) + 1
        for best in (-1e10, float(np.float32(n) * np.float32(0.4)), float(np.nextafter(np.float32(n) * np.float32(0.4), np.float32(np.inf)))):
            got = np.float32(lib.rawdtw_chain_replay(C.byref(opt), _p(a), len(a), _p(costs[c:c + 1]), C.c_float(best)))
            want = np.float32(-1e10) if np.float32(np.float32(n) * np.float32(0.4)) < np.float32(best) else lc.final_score(n, 0.4, costs[c], fused)
            assert got.view(np.uint32) == np.float32(want).view(np.uint32), (c, best, got, want)


def test_the_python_option_record():
    assert ra.MapOpt(dtw_border_constraint=2).c_struct().border_constraint == 2
    for bad in (3, -1):
        with pytest.raises(SystemExit):
            ra.MapOpt(dtw_border_constraint=bad).c_struct()


def test_the_setter_needs_a_context():
    lib = load_library()
    on = C.c_int(7)
    assert lib.rawdtw_set_border_local(None, 1) == 1 and lib.rawdtw_get_border_local(None, C.byref(on)) == 1 and on.value == 7


def test_a_scorer_only_mapper_with_border_2_gives_the_python_mirrors_lines():
    """rawdtw_mapper_create(ctx = NULL) accepts 2; its rounds, scored through the callback on the restatement, write the lines of
    mapper.map_reads with LocalScorer -- chaining, the accept/cut loop, primary chains, MAPQ, the stop rule and the PAF columns unchanged"""
    ref = synth.make_reference([6000], seed=77)
    n = 10
    seeds = mapper.SyntheticSeeds(ref, n, seed=4, max_chunks=3, events_per_chunk=260)
    opt = ra.MapOpt(dtw_border_constraint=2)
    scorer = lc.LocalScorer(ref)
    want, rounds = mapper.map_reads(seeds, list(range(n)), scorer, opt, StopOpt(min_events=20))
    cm = mapper.CMapper(None, opt, StopOpt(min_events=20), ["seq0"], [len(ref.forward[0])], slot_events=4096, max_reads=n, threads=2)
    cm.set_scorer(scorer.callback(opt))
    got, rounds_c = mapper.map_reads_c(seeds, list(range(n)), cm)
    cm.close()
    assert got == want and rounds_c == rounds >= 2
    assert sum(ln.split("\t")[4] in "+-" for ln in want) >= n // 2   # (they map: not a comparison of empty lines)

    class Three(ra.MapOpt):   # any other value is refused as before
        def c_struct(self):
            return AlignOpt(3, 1, 0.1, 0.4, 20.0, 1)

    with pytest.raises(RuntimeError):
        mapper.CMapper(None, Three(), StopOpt(), ["seq0"], [10], slot_events=64, max_reads=1)


def test_the_premise_of_the_property_test(case):
    """on the shared case the restatement gives local <= global (full matrix) for every chain, as floats, and strictly below for at least a
    quarter of them: the end anchors over-reach on the reference by DISPLACE.  Equal when m == 1."""
    cb = case.cb
    loc = lc.job_costs(cb, case.arena)
    glo = np.array([lc.global_cost(*lc.windows(cb, case.arena, c)[:2]) for c in range(cb.n_chains)], np.float32)
    print("local", loc, "global", glo)
    assert (loc <= glo).all()
    assert (loc < glo).sum() * 4 >= cb.n_chains
    rng = np.random.default_rng(3)
    for n in (1, 2, 40):
        a, b = rng.normal(size=n).astype(np.float32), rng.normal(size=1).astype(np.float32)
        assert sc.bits(lc.cost(a, b))[0] == sc.bits(lc.global_cost(a, b))[0]
