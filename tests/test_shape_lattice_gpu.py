"""Every part shape of tests/shape_lattice_cases.py on the device, bit for bit against the oracle (uint32 views; no tolerance
anywhere): the job-list lattice through Engine.score_batch under the planner's knob sets, the stream lattice through the
device-planned batch path at six band radius fractions in three arrangements, and the fold over correlated signals, where the
running best of gen_chains (rmap.cpp:515-524) decides between keep and cut.

Expected part costs: oracle.batch_costs on the jobs rawdtw_batch_build_jobs emits; chain scores and keeps: oracle.align_chain
under the read's running best.  What the inputs are, and that they are what they claim: tests/test_shape_lattice_cpu.py.

The chunk classes of chunk_profile(): 0 quad_dp_r3, 1 lane_dp_r2, 3 lane_dp_r1, 4 lane_dp_gen are reached wherever the CPU table
has the radius (lane_dp_gen: where a pass holds more than 64 radius-3 parts -- the sorted arrangement at 0.04 and 0.10).  Class 2,
lane_dp_r12, is NOT reached by any arrangement, the shuffled one included: since a pass's radius-1 run has a chunk boundary of
its own (rawdtw_chunks.h) no wave holds both radii, and the tests assert that it stays empty.  chunk_profile() reports sums over
chunks, so a class's longest side is read where the sum is exact -- the `peaks` batch, one chunk a class, all of the table's
longest N -- and bounded by chunks x longest N in the full arrangements."""
import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch

    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import rawalign_amd as ra
from rawalign_amd._lib import load_library
from tests import shape_lattice_cases as L

pytestmark = pytest.mark.gpu


def _same_bits(got, want, what, describe=None):
    g, w = np.asarray(got, np.float32).view(np.uint32), np.asarray(want, np.float32).view(np.uint32)
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(g)} differ, first at {bad[:5]}: got {np.asarray(got)[bad[:5]]} want {np.asarray(want)[bad[:5]]}"
                           + (f"; {describe(bad[:5])}" if describe else ""))


def _describe_jobs(jobs, frac=None):
    def f(idx):
        return [(int(j["n"]), int(j["m"]), int(j["band_radius"]), int(j["exclude_last"])) + ((L.tile_record(int(j["n"]), int(j["m"]), frac),) if frac else ())
                for j in jobs[idx]]
    return f


# ------------------------------------------------------------------------------------------------------------------------
# A. the job list
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def job_lattice(oracle):
    jobs, events, rf = L.job_lattice()
    return jobs, events, rf, oracle.batch_costs(jobs, events, rf, nthreads=8)


@pytest.mark.parametrize("knobs", L.KNOB_SETS, ids=L.knob_id)
def test_job_list_lattice(job_lattice, knobs):
    """(n, m, R0, exclude_last) over [1, 100]^2 x 0..9 x {0, 1}, and bands of radius n, n + m and 200 -- far wider than the matrix,
    every antidiagonal clipped -- at the sides where the micro, 8-lane, 16-lane and wave bodies change: every cost, under the
    planner's defaults and with each class switched off, narrowed or (lane_hi) added; a fresh context a set"""
    jobs, events, rf, want = job_lattice
    eng = ra.Engine(0)
    for k, v in knobs.items():
        eng.set_option(k, v)
    eng.upload_reference([rf], [rf])
    j = jobs.copy()
    j["ref_off"] += eng.reference_offset(0, 1)
    got = eng.score_batch(j, events)
    eng.close()
    _same_bits(got, want, f"job list under {knobs}", _describe_jobs(jobs))


# ------------------------------------------------------------------------------------------------------------------------
# B. the stream path
# ------------------------------------------------------------------------------------------------------------------------
def _engine(case, opts):
    eng = ra.Engine(0)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.upload_reference([case.ref[0]], [case.ref[1]])
    assert {st: eng.reference_offset(0, st) for st in (0, 1)} == L.REF_OFFSET
    eng.upload_events(case.cb.events)
    return eng


def _run(case, opt, opts, compact=False, device_planned=True):
    """one batch on a fresh context: (score, keep, part costs, chunk profile, info); the plan's self-check before the run and
    after the fetch -- a batch that ran out of pass slots would be redone through the job list there, and empty the test"""
    eng = _engine(case, opts)
    b = ra.Batch(eng, opt, case.cb, compact=compact)
    assert b.verify_plan() is device_planned
    prof = b.chunk_profile()
    b.run()
    score, keep, jc = b.fetch(with_job_costs=True)
    assert b.verify_plan() is device_planned
    info = b.info()
    b.close()
    eng.close()
    return score, keep, jc, prof, info


_STREAM = {}


def _stream(oracle, frac, name):
    """the arrangement's batches run and checked against the oracle, once a session: (results a batch, the profile summed)"""
    if (frac, name) in _STREAM:
        return _STREAM[frac, name]
    ref = L.reference()
    opt = ra.MapOpt(dtw_band_radius_frac=frac, dtw_min_score=5.0)
    results, total = [], {c: {"jobs": 0, "chunks": 0, "chunk_columns": 0} for c in ra.Batch.CHUNK_CLASSES}
    for chains, per_read in L.arrangement(name, frac):
        case = L.make_case(chains, ref, per_read)
        score, keep, jc, prof, info = _run(case, opt, L.ARRANGEMENT_OPTS[name])
        jobs, _ = L.build_jobs(load_library(), case.cb, opt)
        n_parts = sum(len(c) for c in chains)
        assert info["n_jobs"] == n_parts == len(jc) == len(jobs)
        want_score, want_keep, want_jc = L.oracle_expect(oracle, case, jobs, opt)
        _same_bits(jc, want_jc, f"part costs, {name} at {frac}", _describe_jobs(jobs, frac))
        _same_bits(score, want_score, f"scores, {name} at {frac}")
        assert np.array_equal(keep, want_keep)
        n_tile = sum(L.tile_record(n, m, frac) is not None for c in chains for n, m in c)
        assert sum(prof[c]["jobs"] for c in ra.Batch.CHUNK_CLASSES) == n_tile, (prof, n_tile)
        assert info["n_lane_jobs"] + info["n_wave_band_jobs"] == n_parts, info
        for c in ra.Batch.CHUNK_CLASSES:
            for k in total[c]:
                total[c][k] += prof[c][k]
        results.append((case, score, keep, jc))
    _STREAM[frac, name] = results, total
    return _STREAM[frac, name]


def test_side_list_over_its_capacity_is_redone_through_the_job_list(oracle):
    """the whole sorted lattice at 0.25 in one batch: 5 825 parts are the side list's, which holds min(na, na / 4 + 4096) = 5 699
    of a batch of 6 413 anchors -- the device-planned path declines the batch and the job list gives the oracle's results"""
    frac = 0.25
    assert L.TABLE[frac][3] > (len(L.STREAM_LATTICE) + 13) // 4 + 4096
    (chains, per_read), = L.arrangement("sorted_whole", frac)
    case = L.make_case(chains, L.reference(), per_read)
    opt = ra.MapOpt(dtw_band_radius_frac=frac, dtw_min_score=5.0)
    score, keep, jc, prof, info = _run(case, opt, L.ARRANGEMENT_OPTS["sorted_whole"], device_planned=False)
    jobs, _ = L.build_jobs(load_library(), case.cb, opt)
    want_score, want_keep, want_jc = L.oracle_expect(oracle, case, jobs, opt)
    assert prof == {} and info["n_jobs"] == len(jobs) == len(L.STREAM_LATTICE)
    _same_bits(jc, want_jc, "part costs", _describe_jobs(jobs, frac))
    _same_bits(score, want_score, "scores")
    assert np.array_equal(keep, want_keep)


def _check_profile(frac, prof, whole):
    """the classes against the CPU table: radius 1 runs under lane_dp_r1 alone; radius 3 under the quads or, beyond a pass's first 64
    records, the generic body, which then also takes the radius-2 parts that share its waves; no class met a side longer than
    the table's"""
    (n1, l1), (n2, l2), (n3, l3), _ = L.TABLE[frac]
    name = ra.Batch.CHUNK_CLASSES
    q, r2, r12, r1, gen = (prof[name[c]] for c in range(5))
    assert r12["jobs"] == 0
    if whole:
        assert r1["jobs"] == n1 and q["jobs"] + r2["jobs"] + gen["jobs"] == n2 + n3 and q["jobs"] + gen["jobs"] >= n3 >= q["jobs"]
    for cls, longest in ((q, l3), (r2, l2), (r1, l1), (gen, max(l2, l3))):
        assert cls["chunk_columns"] <= cls["chunks"] * longest


@pytest.mark.parametrize("name", ["sorted", "shuffled", "singles"])
@pytest.mark.parametrize("frac", L.FRACS)
def test_stream_lattice(oracle, frac, name):
    """all (n, m) in [1, 80]^2 at the fraction: part costs, scores and keeps at dtw_min_score 5, the job count, and the plan's
    self-check before the run and after the fetch.  sorted: tiles of one radius, longest first, in batches of six chains with an image of 16 384 floats
    (a pass of more than 64 radius-3 parts: quads and the generic body); shuffled: at the defaults, in two batches; singles: a
    chain a part (exclude_last = 0 everywhere, hundreds of chain starts a tile, a hundred chains a read)"""
    _, prof = _stream(oracle, frac, name)
    print(f"\n{frac} {name}: " + ", ".join(f"{c} {prof[c]['jobs']} jobs / {prof[c]['chunks']} chunks / {prof[c]['chunk_columns']} columns" for c in ra.Batch.CHUNK_CLASSES))
    _check_profile(frac, prof, whole=True)
    if name == "sorted":
        assert (prof["lane_gen"]["jobs"] > 0) == (L.TABLE[frac][2][0] > 64) and (prof["quad_r3"]["jobs"] > 0) == (L.TABLE[frac][2][0] > 0)


@pytest.mark.parametrize("frac", L.FRACS)
def test_stream_lattice_reaches_every_body_at_its_longest(oracle, frac):
    """over the fraction's three arrangements every class the CPU table says is reachable has jobs; in the `peaks` batch (a chunk a
    class, parts of the table's longest side only) the chunk's columns are that side: lane_dp_r1 at N = 73 (0.01) and 49 (0.04)
    against 19 at the default fraction, radius 3 at N = 73 (0.04) against 58"""
    profs = [_stream(oracle, frac, name)[1] for name in ("sorted", "shuffled", "singles")]
    jobs = {c: sum(p[c]["jobs"] for p in profs) for c in ra.Batch.CHUNK_CLASSES}
    (n1, l1), (n2, l2), (n3, l3), _ = L.TABLE[frac]
    assert (jobs["lane_r1"] > 0) == (n1 > 0) and (jobs["lane_r2"] > 0) == (n2 > 0) and (jobs["quad_r3"] > 0) == (n3 > 0)
    assert (jobs["lane_gen"] > 0) == (n3 > 64) and jobs["lane_r12"] == 0
    _, peaks = _stream(oracle, frac, "peaks")
    _check_profile(frac, peaks, whole=False)
    held = {L.tile_record(c[0][0], c[0][1], frac)[2]: len(c) for c in L.peak_parts(frac)}
    for cls, R, (count, longest) in (("lane_r1", 1, (n1, l1)), ("lane_r2", 2, (n2, l2)), ("quad_r3", 3, (n3, l3))):
        want = (held[R], 1, longest) if count else (0, 0, 0)
        assert (peaks[cls]["jobs"], peaks[cls]["chunks"], peaks[cls]["chunk_columns"]) == want, (cls, peaks[cls], want)


@pytest.mark.parametrize("how", [{"compact": True}, {"stream_tile_radius": 1}, {"stream_tile_radius": 2}], ids=["compact", "tile_radius1", "tile_radius2"])
@pytest.mark.parametrize("frac", [0.04, 0.5])
def test_shuffled_lattice_other_hand_overs(oracle, frac, how):
    """the shuffled arrangement through the compact hand-over, and with the tiles kept to radius 1 / 2 so that radii 2 and 3 go to
    the side list's lane classes: results equal the plain run's (which test_stream_lattice pins to the oracle)"""
    plain, _ = _stream(oracle, frac, "shuffled")
    opt = ra.MapOpt(dtw_band_radius_frac=frac, dtw_min_score=5.0)
    opts = {k: v for k, v in how.items() if k != "compact"}
    for case, score, keep, jc in plain:
        s2, k2, j2, prof, _ = _run(case, opt, opts, compact=how.get("compact", False))
        _same_bits(j2, jc, f"part costs, shuffled at {frac} under {how}")
        _same_bits(s2, score, f"scores, shuffled at {frac} under {how}")
        assert np.array_equal(k2, keep)
        if "stream_tile_radius" in opts:   # the tiles hold no wider radius
            limit = opts["stream_tile_radius"]
            assert prof["quad_r3"]["jobs"] == 0 and prof["lane_gen"]["jobs"] == 0 and (limit == 2 or prof["lane_r2"]["jobs"] == 0)


# ------------------------------------------------------------------------------------------------------------------------
# C. the fold
# ------------------------------------------------------------------------------------------------------------------------
_FOLD = {}


def _fold_cases(frac):
    if frac not in _FOLD:
        _FOLD[frac] = [case for case, _ in L.fold_cases(frac, L.fold_reference())]
    return _FOLD[frac]


@pytest.mark.parametrize("bonus,min_score,fused", L.FOLD_PARAMS)
@pytest.mark.parametrize("frac", L.FOLD_FRACS)
def test_fold_over_correlated_signals(oracle, frac, bonus, min_score, fused):
    """reads of 3..12 chains of 1..120 parts (two batches a fraction) whose events follow their reference windows under a noise level a chain: a quarter or
    more of the chains are kept and most others cut by the read's running best, which rises several times a read
    (tests/test_shape_lattice_cpu.py pins those shares).  Scores, the -1e10 of cut chains and keeps equal the oracle's sequential
    loop, under both forms of rmap.cpp:306 and on both paths ("device_plan" 1 and 0).  At dtw_min_score -1e9 nothing falls below
    the bound: a chain is kept unless the running best -- which starts at 0 whatever the bound, rmap.cpp:515 -- cut it, and
    every chain that was not cut has the full fold of its parts."""
    opt = ra.MapOpt(dtw_band_radius_frac=frac, dtw_match_bonus=bonus, dtw_min_score=min_score, fused_score=fused)
    for case in _fold_cases(frac):
        jobs, _ = L.build_jobs(load_library(), case.cb, opt)
        want_score, want_keep, want_jc = L.oracle_expect(oracle, case, jobs, opt)
        cut = want_score == np.float32(-1e10)
        print(f"\nfold at {frac}, bonus {bonus}, min_score {min_score:g}, fused {int(fused)}: {case.cb.n_chains} chains, kept {want_keep.mean():.2f}, cut {cut.mean():.2f}")
        for device_plan in (1, 0):
            score, keep, jc, _, info = _run(case, opt, {"device_plan": device_plan}, device_planned=bool(device_plan))
            assert info["n_jobs"] == len(jobs)
            _same_bits(jc, want_jc, f"part costs, device_plan {device_plan}", _describe_jobs(jobs, frac))
            _same_bits(score, want_score, f"scores, device_plan {device_plan}")
            assert np.array_equal(keep, want_keep)
            if min_score < -1e8:
                full = L.full_fold(oracle, case, opt)
                assert np.array_equal(keep.astype(bool), ~cut) and keep.any() and cut.any()
                _same_bits(score[~cut], full[~cut], "uncut chains: the full fold")
