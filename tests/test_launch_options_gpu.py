"""Options that shape launches change no bit, and the figures the timed entry points return agree with each other.

The rows of rawdtw_options.h set here, and RAWDTW_SIDE_STREAMS, only decide which instantiation scores a job, on which stream and in
which order: "tile_threads" 512 / 1024 (k_band_tile<0, 3, true, 512> and <..., 1024> through launch_band_tile; no k_band_merged, no
sync-free path), the side streams run_all_launches forks a plan's launches over, where k_wide sits among a sync-free batch's launches
("wide_order", "wide_at_create", "wide_beside", "wide_blocks"), the persistent grid of k_runs ("stream_blocks_per_cu",
"stream_threads").  Every result is held to the oracle, bit for bit; every case asserts, from the plan's own report, that the branch it
names was taken.  Then: rawdtw_batch_run_timed / _collect / _launch_stats / _info / _plan_ms / _wide_ms against each other and against
the oracle's cell count."""
import math

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd.align import CandidateBatch
from tests.replay_cases import case, expected_counts, random_job_cases
from tests.test_gpu_parity import run
from tests.test_stream_path import _chains, _tiny
from tests.util import assert_bits_equal, make_arena_jobs, oracle_costs

pytestmark = pytest.mark.gpu

KIND_LANE, KIND_FOLD, KIND_SELECT, KIND_WREG, KIND_MERGED = 1, 6, 7, 8, 10  # rawdtw_internal.h: kKindBandLane .. kKindBandMerged


def _dtw(stats):
    return [s for s in stats if s["kind"] not in (KIND_FOLD, KIND_SELECT)]


# ---- the job-list path ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def job_set(oracle):
    """the 3 000 random jobs (every radius class, both exclude_last values) and the oracle's costs, taken once"""
    jobs, ev, rf = make_arena_jobs(random_job_cases())
    assert set(np.unique(jobs["band_radius"])) >= set(range(12)) and set(np.unique(jobs["exclude_last"])) == {0, 1}
    return jobs, ev, rf, oracle_costs(oracle, jobs, ev, rf)


def _plan_kinds(eng, jobs, ev, rf):
    """the launches of the job set's plan on `eng`, as rawdtw_plan_run_timed names them, and the plan's record"""
    pad = np.zeros(8, np.float32)
    eng.upload_reference([np.concatenate([rf, pad])], [np.concatenate([rf, pad])])
    eng.upload_events(ev)
    j = jobs.copy()
    j["ref_off"] += eng.reference_offset(0, 1)
    plan = eng.plan(j)
    info = plan.info()
    launches = plan.run_timed()
    cost = plan.fetch()
    plan.close()
    return launches, info, cost


@pytest.mark.parametrize("setting", [
    {"tile_threads": 512},
    {"tile_threads": 1024},
    {"tile_threads": 1024, "sort_n": 17, "sort_r1_n": 9, "sort_r3": 1},
    {"tile_threads": 512, "sort_n": 5, "sorted_tile_jobs": 128},
    {"tile_threads": 1024, "tile_lds_floats": 2048, "tile_max_jobs": 64},     # tiles of fewer jobs than threads
    {"tile_threads": 512, "tile_lds_floats": 30000, "tile_max_jobs": 4096},
    # (a random job is a span pair of its own: 96 spans cut the tiles above at some 60 jobs.)  Several rounds a tile: all jobs in ONE
    {"tile_threads": 512, "tile_lds_floats": 30000, "tile_max_jobs": 4096, "tile_max_spans": 4096},
    {"tile_max_spans": 8},
], ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()))
def test_tile_kernel_geometry_changes_no_cost(job_set, setting):
    """The tile kernel at 512 and 1024 threads (tile_block's staging takes THREADS / 8 span groups: its index arithmetic follows the
    workgroup size), alone, with the shape-sorted tiles, with tiles smaller and larger than a workgroup; and tiles cut at 8 spans."""
    jobs, ev, rf, want = job_set
    eng = ra.Engine(0)
    for k, v in setting.items():
        eng.set_option(k, v)
    assert eng.get_option("tile_threads") == setting.get("tile_threads", 256)
    assert_bits_equal(run(eng, jobs, ev, rf), want, f"options {setting}")
    launches, info, cost = _plan_kinds(eng, jobs, ev, rf)
    assert_bits_equal(cost, want, f"options {setting}, through the plan")
    # the tile kernel had jobs, in a launch of its own (rawdtw_plan_run_timed names the launches as planned)
    assert info["n_lane_jobs"] > 512 and any(k == KIND_LANE for k, _, _ in launches), (info, launches)
    if setting.get("tile_max_spans") == 4096:  # more jobs in the one tile than the workgroup has threads: a second round
        from rawalign_amd.dtw import plan_dry_run

        planner = {k: v for k, v in setting.items() if k != "tile_threads"}
        assert plan_dry_run(jobs, len(ev), len(rf) + 8, options=planner)[1] == 1 and info["n_lane_jobs"] > setting["tile_threads"]
    eng.close()


SIDE_SETTINGS = [(n, {"serial_launches": s}) for n in (1, 2, 3) for s in (0, 1)] + [(3, {"merge_small": 0})]


@pytest.mark.parametrize("n_side,setting", SIDE_SETTINGS, ids=lambda v: str(v).replace(" ", ""))
def test_side_streams_fork_and_join(oracle, job_set, monkeypatch, n_side, setting):
    """RAWDTW_SIDE_STREAMS (read at rawdtw_create): run_all_launches deals a plan's launches over the side streams and joins them
    through ev_join before the fold -- a fold that ran ahead of a join would read costs not yet written.  The random job set through
    rawdtw_score_batch, then a batch of the same shapes through fold and select: at least three launches, so the fork forks, and
    none of them merged unless the launches are serial."""
    monkeypatch.setenv("RAWDTW_SIDE_STREAMS", str(n_side))
    jobs, ev, rf, want = job_set
    eng = ra.Engine(0)
    for k, v in setting.items():
        eng.set_option(k, v)
    assert_bits_equal(run(eng, jobs, ev, rf), want, f"RAWDTW_SIDE_STREAMS={n_side} {setting}")
    eng.close()
    cs = case("job_shapes")
    eng = cs.engine(device_plan=0, **setting)
    b = cs.batch(eng)
    assert b.verify_plan() is False
    dtw = _dtw(b.launch_stats())
    assert len(dtw) >= 3, dtw
    merged = [s for s in dtw if s["kind"] == KIND_MERGED]
    serial = bool(setting.get("serial_launches"))
    assert len(merged) == (1 if serial else 0), dtw
    b.run()
    cs.check(oracle, b.fetch(with_job_costs=True), "A", "A", what=f"RAWDTW_SIDE_STREAMS={n_side} {setting}")
    cs.upload(eng, "B")
    b.run()  # (and once more: the fork event and the joins are the context's, used again)
    cs.check(oracle, b.fetch(with_job_costs=True), "B", "A", what=f"RAWDTW_SIDE_STREAMS={n_side} {setting}, replayed")
    eng.close()


@pytest.mark.parametrize("env,options", [(None, {"tile_threads": 512}), ("2", {"device_plan": 0})], ids=["tile_threads=512", "side_streams=2"])
def test_sparse_batch_through_the_job_list_under_launch_options(oracle, monkeypatch, env, options):
    """the sparse + banded batch of the replay tests: "tile_threads" 512 keeps it off the sync-free path (stream_eligible) and off
    k_band_merged (merge_of); two side streams fork its launches"""
    if env is not None:
        monkeypatch.setenv("RAWDTW_SIDE_STREAMS", env)
    cs = case("medium")
    eng = cs.engine(**options)
    b = cs.batch(eng)
    assert b.verify_plan() is False
    dtw = _dtw(b.launch_stats())
    assert not any(s["kind"] == KIND_MERGED for s in dtw) and any(s["kind"] == KIND_LANE and s["n_jobs"] > 0 for s in dtw), dtw
    b.run()
    cs.check(oracle, b.fetch(with_job_costs=True), "A", "A", what=str(options))
    eng.close()


# ---- the sync-free path -----------------------------------------------------------------------------------------------------------
STREAM_SETTINGS = [{"wide_order": o, "wide_beside": w} for o in (0, 1, 2) for w in (0, 1)] + [
    {"wide_at_create": 1, "wide_order": 0},
    {"stream_blocks_per_cu": 0}, {"stream_blocks_per_cu": 1}, {"stream_blocks_per_cu": 16},
    {"wide_blocks": 1}, {"wide_blocks": 65535},
    {"stream_threads": 512, "stream_blocks_per_cu": 0},
]


@pytest.mark.parametrize("submit", [False, True], ids=["create", "submit"])
@pytest.mark.parametrize("which", ["wide", "sprinkled"])
@pytest.mark.parametrize("setting", STREAM_SETTINGS, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()))
def test_stream_launch_options_change_no_bit(oracle, setting, which, submit):
    """Where k_wide sits (between the planning launches, in front of k_runs, behind it; in line or on the context's second stream),
    how many workgroups it has, and the persistent grid of k_runs (what the occupancy query gives, one workgroup a CU, more than the
    query allows): a first run after a plain create and inside rawdtw_batch_submit, and one replay over other arenas after each.
    (No upload comes between the create and the first run: "wide_at_create" asks for that.)"""
    cs = case(which)
    eng = cs.engine(**setting)
    for k, v in setting.items():
        assert eng.get_option(k) == v
    b = cs.batch(eng, submit=submit)
    b.run()
    cs.check(oracle, b.fetch(with_job_costs=True), "A", "A", what=f"{setting} first run")
    assert b.verify_plan() is True  # still a sync-free batch: k_wide and k_runs scored it
    assert which != "wide" or b.stream_counters()["side_jobs"] > 1000  # (four of _wide's six lengths give a radius above the tiles' 3)
    cs.upload(eng, "B")
    b.run()
    cs.check(oracle, b.fetch(with_job_costs=True), "B", "A", what=f"{setting} replay")
    assert cs.costs_mostly_differ(("A", "A"), ("B", "A"))
    eng.close()


def test_two_batches_in_flight_share_the_wide_stream(oracle):
    """"wide_beside": ev_wide_fork and ev_wide_join are one pair a context.  Two batches submitted back to back -- the second's fork
    recorded before the first's join is waited for by anything on the host -- and fetched in order: both equal the oracle.  (One event
    arena holds both batches' events: the second batch's reads lie behind the first's.)"""
    cs = case("wide")
    eng = cs.engine(wide_beside=1)
    n_ev = len(cs.events["A"])
    eng.upload_events(np.concatenate([cs.events["A"], cs.events["B"]]))
    cb_x = cs.candidate_batch(eng)
    cb_y = CandidateBatch(cb_x.events, cb_x.chain_off, cb_x.anchor_off, cb_x.anchors, cb_x.ref_base, (cb_x.read_base + np.uint32(n_ev)).astype(np.uint32))
    x = ra.Batch(eng, cs.opt, cb_x, submit=True)
    y = ra.Batch(eng, cs.opt, cb_y, submit=True)
    got_x = x.fetch(with_job_costs=True)
    got_y = y.fetch(with_job_costs=True)
    assert x.verify_plan() is True and y.verify_plan() is True and x.stream_counters()["side_jobs"] > 0
    cs.check(oracle, got_x, "A", "A", what="first of two in flight")
    cs.check(oracle, got_y, "B", "A", what="second of two in flight")
    eng.close()


# ---- the figures the calls return ---------------------------------------------------------------------------------------------------
FIGURE_BATCHES = {
    "stream": ("wide", {}, None),
    "stream_tiles_only": ("tiny", {}, None),
    "job_list": ("medium", {"device_plan": 0}, None),
    "job_list_side_streams": ("medium", {"device_plan": 0}, "2"),
    "job_list_full": ("full", {}, None),
}


def _pairs(launches):
    return [(k, p) for k, p, _ in launches]


def _times_hold(launches, stats, what):
    assert len(launches) == len(stats)
    for (k, p, ms), s in zip(launches, stats):
        assert math.isfinite(ms) and ms >= 0.0, (what, launches)
        if s["kind"] not in (KIND_FOLD, KIND_SELECT) and s["n_jobs"] > 0:  # (a launch that travels inside the merged one reports no jobs)
            assert ms > 0.0, (what, k, p, s)


@pytest.mark.parametrize("name", list(FIGURE_BATCHES))
def test_timed_runs_launch_stats_and_info_agree(oracle, monkeypatch, name):
    which, options, env = FIGURE_BATCHES[name]
    if env is not None:
        monkeypatch.setenv("RAWDTW_SIDE_STREAMS", env)
    cs = case(which)
    eng = cs.engine(**options)
    b = cs.batch(eng)
    jobs = b.build_jobs()[0]
    stats = b.launch_stats()
    info = b.info()
    # the kinds: the same list from the timed run, from the collected runs and from the static report; fold and select last
    want_pairs = [(s["kind"], s["param"] & 0xFFFFFF) for s in stats]  # (a launch word holds the parameter's low 24 bits)
    assert [k for k, _ in want_pairs[-2:]] == [KIND_FOLD, KIND_SELECT] and len(want_pairs) >= 3
    timed = b.run_timed()
    assert _pairs(timed) == want_pairs
    _times_hold(timed, stats, f"{name} run_timed")
    cs.check(oracle, b.fetch(with_job_costs=True), "A", "A", what=f"{name} run_timed", jobs=jobs)
    reps = b.run_reps(3, timed=True)
    assert _pairs(reps) == want_pairs
    _times_hold(reps, stats, f"{name} run_reps")
    for _ in range(3):
        b.enqueue(True)
    collected, runs = b.collect()
    assert runs == 3 and _pairs(collected) == want_pairs
    _times_hold(collected, stats, f"{name} collect")
    again, runs = b.collect()   # nothing enqueued since: no runs, no time
    assert runs == 0 and _pairs(again) == want_pairs and all(ms == 0.0 for _, _, ms in again)
    # jobs and cells: every job and every cell in exactly one DTW launch; the totals are the batch's and the oracle's
    dtw = _dtw(stats)
    n_jobs, cells = expected_counts(oracle, jobs)
    assert sum(s["n_jobs"] for s in dtw) == info["n_jobs"] == n_jobs == len(jobs)
    assert sum(s["cells"] for s in dtw) == info["cells"] == cells
    assert all(s["cells"] == 0 for s in stats[-2:]) and stats[-2]["n_jobs"] == info["n_chains"] and stats[-1]["n_jobs"] == info["n_reads"]
    if name.startswith("stream"):
        assert b.verify_plan() is True
        assert [s["kind"] for s in dtw] == [KIND_WREG, KIND_MERGED] and dtw[0]["param"] == 0 and dtw[1]["param"] > 0  # (k_wide; k_runs and its image's floats)
        # launch 0 is the side list's: the jobs outside the tile class, and their cells
        tile_radius = min(eng.get_option("lane_max_radius"), eng.get_option("stream_tile_radius"))
        _, _, n_side, c_side = expected_counts(oracle, jobs, tile_radius, eng.get_option("lane_max_n"))
        assert (dtw[0]["n_jobs"], dtw[0]["cells"]) == (n_side, c_side) and n_side == b.stream_counters()["side_jobs"]
        assert (n_side > 0) == (name == "stream")
    else:
        assert b.verify_plan() is False
        merged = [s for s in dtw if s["kind"] == KIND_MERGED]
        assert len(merged) == (1 if name == "job_list" else 0), dtw   # (side streams: nothing is merged; full-matrix jobs: nothing to merge)
        if name == "job_list_full":
            assert info["n_full_jobs"] == n_jobs
    eng.close()


def test_plan_and_wide_brackets(oracle):
    """"time_plan": rawdtw_batch_plan_ms and rawdtw_batch_wide_ms are finite and not negative for a sync-free batch created under it --
    with the side list's launch inside the second bracket ("wide_at_create", as the benchmark's timed passes set it) and without --,
    exactly 0 with the option off and for a job-list batch, and the option changes no result."""
    cs = case("wide")
    for options in ({"time_plan": 1}, {"time_plan": 1, "wide_at_create": 1}):
        eng = cs.engine(**options)
        b = cs.batch(eng)
        b.run()
        cs.check(oracle, b.fetch(with_job_costs=True), "A", "A", what=str(options))
        assert b.verify_plan() is True
        plan_ms, wide_ms = b.plan_ms(), b.wide_ms()
        assert math.isfinite(plan_ms) and plan_ms >= 0.0 and math.isfinite(wide_ms) and wide_ms >= 0.0, (plan_ms, wide_ms)
        eng.close()
    eng = cs.engine()
    b = cs.batch(eng)
    b.run()
    cs.check(oracle, b.fetch(with_job_costs=True), "A", "A", what="time_plan off")
    assert b.verify_plan() is True and b.plan_ms() == 0.0 and b.wide_ms() == 0.0
    eng.close()
    eng = cs.engine(time_plan=1, device_plan=0)
    b = cs.batch(eng)
    b.run()
    cs.check(oracle, b.fetch(with_job_costs=True), "A", "A", what="time_plan, job list")
    assert b.verify_plan() is False and b.plan_ms() == 0.0 and b.wide_ms() == 0.0
    eng.close()


def _tiny_batch_with(rng, eng, ref_len, special=None, spoil=False):
    state = {"k": 0}

    def shapes(r):
        state["k"] += 1
        return special if special is not None and state["k"] == 17 else _tiny(r)
    events, chain_off, anchor_off, anchors, slot, read_base = _chains(rng, 30, ref_len, shapes)
    if spoil:  # a chain whose positions do not descend along its list: no path scores it
        anchors = anchors.copy()
        first_long = int(np.argmax(np.diff(anchor_off.astype(np.int64)) >= 3))
        anchors["query_position"][int(anchor_off[first_long]) + 1] += 5000
    strand_of = [1 if s == 0 else 0 for s in slot]
    ref_base = np.array([eng.reference_offset(0, st) for st in strand_of], np.uint64)
    eng.upload_events(events)
    return CandidateBatch(events, chain_off, anchor_off, anchors, ref_base, read_base), strand_of


def test_collect_after_the_batch_changed_form_or_died(oracle):
    """rawdtw_batch_fetch redoes a batch the sync-free path declined through the job list, and a batch that cannot be redone (invalid
    anchors) is left with neither form.  rawdtw_batch_collect afterwards: for the redone batch, the launches of the form it has now and
    no runs (the timed runs enqueued before were the declined form's, with another number of launches); for the dead one, the refusal
    every other entry point gives."""
    from tests.test_stream_path import _oracle_check

    rng = np.random.default_rng(77)
    ref = [rng.normal(size=40000).astype(np.float32), rng.normal(size=40000).astype(np.float32)]
    eng = ra.Engine(0)
    eng.upload_reference([ref[0]], [ref[1]])
    opt = ra.MapOpt(dtw_min_score=5.0)
    cb, strand_of = _tiny_batch_with(rng, eng, 40000, special=(3000, 2800))  # n = 3001: a band of 301 offsets, wider than k_wide takes
    b = ra.Batch(eng, opt, cb)
    for _ in range(2):
        b.enqueue(True)
    score, keep, jc = b.fetch(with_job_costs=True)
    assert b.verify_plan() is False  # now a job-list batch
    _oracle_check(oracle, cb, {1: ref[0], 0: ref[1]}, strand_of, score, keep, jc, opt)
    stats = b.launch_stats()
    launches, runs = b.collect()
    assert runs == 0 and _pairs(launches) == [(s["kind"], s["param"] & 0xFFFFFF) for s in stats] and all(ms == 0.0 for _, _, ms in launches)
    timed = b.run_timed()
    assert _pairs(timed) == _pairs(launches)
    b.close()
    cb_bad, _ = _tiny_batch_with(rng, eng, 40000, spoil=True)
    bad = ra.Batch(eng, opt, cb_bad)
    bad.enqueue(True)
    with pytest.raises(ra.RawDTWError) as e:
        bad.fetch()
    assert "job " in str(e.value)
    for call in (bad.collect, bad.run, lambda: bad.enqueue(False), lambda: bad.run_reps(1, timed=False), bad.fetch, bad.info):
        with pytest.raises(ra.RawDTWError) as e:
            call()
        assert e.value.status == 1, call  # RAWDTW_ERR_INVALID
    bad.close()
    eng.close()
