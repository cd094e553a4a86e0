"""A batch that runs again does all of its work again.  The suite's other tests fetch a batch's FIRST run; every figure of the
benchmark's kernel_replay comes from later ones, through rawdtw_batch_run on a batch that has run, rawdtw_batch_run_timed,
rawdtw_batch_run_reps and rawdtw_batch_enqueue / rawdtw_batch_collect -- where the sync-free path clears the tile queue's heads
(stream_run's reset_queue), launches k_wide from batch_enqueue_one instead of with the planning launches, and the job-list path
walks run_all_launches again.  A replay that did nothing, or part of the work, would leave the first run's outputs in memory and
every fetch right: so the arenas change between the runs (include/rawdtw.h: a run reads the context's arenas as they are when it is
enqueued) to contents under which the oracle gives another cost for EVERY part, and the replay is held to the oracle on those."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from tests.replay_cases import case, same_bits
from tests.test_stream_path import _match, _two_rounds

pytestmark = pytest.mark.gpu

KIND_FOLD, KIND_SELECT, KIND_MERGED = 6, 7, 10  # rawdtw_internal.h: kKindChainFold, kKindReadSelect, kKindBandMerged


def _sync_free(b):
    assert b.verify_plan() is True  # the sync-free path took the batch, and its records pass the self-check


def _sync_free_with_side_list(b):
    assert b.verify_plan() is True
    assert b.stream_counters()["side_jobs"] > 0  # k_wide has work: the hand-over of its launch matters


def _job_list_merged_and_more(b):
    assert b.verify_plan() is False
    dtw = [s for s in b.launch_stats() if s["kind"] not in (KIND_FOLD, KIND_SELECT)]
    assert any(s["kind"] == KIND_MERGED for s in dtw) and len(dtw) >= 2, dtw


def _job_list_full(b):
    assert b.verify_plan() is False and b.info()["n_full_jobs"] > 0


# name: (case, context options, ra.Batch keywords, what holds before the replay, the replay meets a second reference as well)
BATCHES = {
    "sprinkled": ("sprinkled", {}, {}, _sync_free, True),  # (nearly all parts in the tiles' passes; the slanted radius-3 ones beside them)
    "side_list": ("wide", {}, {}, _sync_free_with_side_list, True),
    "compact": ("medium", {}, {"compact": True}, _sync_free_with_side_list, True),  # (k_wide went out with the planning launches: every replay launches it itself)
    "submitted": ("wide", {}, {"submit": True}, _sync_free_with_side_list, True),   # (rawdtw_batch_submit, as the benchmark's loop creates its batches)
    "job_list": ("medium", {"device_plan": 0}, {}, _job_list_merged_and_more, True),
    "job_list_full": ("full", {}, {}, _job_list_full, False),
}
ENTRIES = ("run", "run_timed", "reps", "reps_timed", "enqueue", "enqueue_timed")


def _replay(b, entry):
    if entry == "run":
        b.run()
    elif entry == "run_timed":
        assert len(b.run_timed()) >= 3
    elif entry == "reps":
        assert b.run_reps(3, timed=False) == []
    elif entry == "reps_timed":
        assert len(b.run_reps(3, timed=True)) >= 3
    elif entry == "enqueue":
        b.enqueue(False)
        b.enqueue(False)
    else:
        for _ in range(3):
            b.enqueue(True)
        launches, runs = b.collect()
        assert runs == 3 and len(launches) >= 3


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(BATCHES))
def test_replay_scores_the_arenas_as_they_are_then(oracle, name, entry):
    """Run over A, fetch, hold to the oracle on A; upload B; replay through `entry`; fetch: every part cost, score and keep flag is the
    oracle's on B, and no part cost of B equals A's at its index -- so a replay in which stream_run, stream_wide_fork or
    run_all_launches did nothing (the first run's costs still in the cost array) cannot pass, in any part of any launch."""
    which, options, create, before, second_reference = BATCHES[name]
    cs = case(which)
    eng = cs.engine(**options)
    b = cs.batch(eng, **create)
    b.run()
    first = b.fetch(with_job_costs=True)
    jobs = b.build_jobs()[0]
    cs.check(oracle, first, "A", "A", what=name, jobs=jobs)
    before(b)
    # (under new events alone a part now and then costs what it did: an event between two reference values r0 <= e <= r1 gives
    # |e - r0| + |e - r1| = r1 - r0 wherever it lies; so the sparse cases' replays meet a second reference of the same lengths too)
    ref = "B" if second_reference else "A"
    cs.upload(eng, "B", "B" if second_reference else None)
    _replay(b, entry)
    again = b.fetch(with_job_costs=True)
    cs.check(oracle, again, "B", ref, what=f"{name} replayed through {entry}", jobs=jobs)
    assert cs.costs_differ_everywhere(("A", "A"), ("B", ref))
    b.close()
    eng.close()


@pytest.mark.parametrize("name", ["side_list", "compact", "job_list"])
def test_five_replays_over_alternating_arenas(oracle, name):
    """A, B, A, B, A (events and reference): the state a replay leaves -- counters, work list, pass slots, queue heads, the side list's
    hand-over flag -- is the state it found, whichever contents it ran over."""
    which, options, create, before, _ = BATCHES[name]
    cs = case(which)
    eng = cs.engine(**options)
    b = cs.batch(eng, **create)
    for k, ab in enumerate("ABABA"):
        if k:
            cs.upload(eng, ab, ab)
        b.run()
        got = b.fetch(with_job_costs=True)
        cs.check(oracle, got, ab, ab, what=f"{name} run {k}", jobs=None)
        if k == 0:
            before(b)
    assert cs.costs_differ_everywhere(("A", "A"), ("B", "B"))
    b.close()
    eng.close()


def test_replay_draws_its_passes_from_the_tile_queue_again(oracle):
    """k_runs deals a workgroup's first two passes by block index and every later one from the tile queue (cnt[kCntHeads ..]), which
    the first run leaves advanced and stream_run clears for a run that is not the first.  The batches above have fewer passes than
    twice the grid: here one workgroup a CU ("stream_blocks_per_cu" 1) and a small image ("tile_lds_floats" 2048: several passes a
    tile, their slots from the pool) put most passes behind the queue.  A replay that met the heads where the first run left them
    would draw no ticket inside the list and leave those passes' parts at the first run's costs: the replay, over other events, is
    held to the oracle, and no part's cost under either contents equals its cost under the other."""
    torch = pytest.importorskip("torch")
    cs = case("queue")
    eng = cs.engine(stream_blocks_per_cu=1, tile_lds_floats=2048)
    grid = torch.cuda.get_device_properties(0).multi_processor_count  # (one workgroup a CU)
    b = cs.batch(eng)
    b.run()
    first = b.fetch(with_job_costs=True)
    assert b.verify_plan() is True
    cnt = b.stream_counters()
    assert cnt["todo"] + cnt["pool"] > 2 * grid + 64, (cnt, grid)  # passes the queue deals
    cs.upload(eng, "B", "B")
    b.run()
    again = b.fetch(with_job_costs=True)
    cs.check(oracle, again, "B", "B", what="replay through the queue")
    assert np.all(first[2].view(np.uint32) != again[2].view(np.uint32))
    for k in range(2):  # and twice more without a fetch in between, then over the first contents again
        b.enqueue(False)
    cs.upload(eng, "A", "A")
    b.run()
    third = b.fetch(with_job_costs=True)
    same_bits(third, first, "back over the first events")
    b.close()
    eng.close()


def test_carried_round_replayed_over_unchanged_arenas():
    """rawdtw_batch_submit_carry, then the batch again through rawdtw_batch_run, rawdtw_batch_enqueue and rawdtw_batch_run_reps with
    the arenas as they were (the parts taken over are the previous batch's costs: stale by contract once events change): the same
    bits as its first run -- which equal a from-scratch batch of the round --, and rawdtw_batch_round_stats says what it said."""
    rng = np.random.default_rng(1999)
    ref = [rng.normal(size=90000).astype(np.float32), rng.normal(size=90000).astype(np.float32)]
    eng = ra.Engine(0)
    eng.upload_reference([ref[0]], [ref[1]])
    lib = eng.lib
    cb1, cb2, prev_read, expect = _two_rounds(rng, eng, n_reads=60)
    nc = cb2.n_chains
    eng.upload_events(cb2.events)
    opt = ra.MapOpt(dtw_min_score=5.0)
    copt = opt.c_struct()
    vp = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    plain = ra.Batch(eng, opt, cb2)
    plain.run()
    want = plain.fetch(with_job_costs=True)
    plain.close()
    b1 = ra.Batch(eng, opt, cb1)
    b1.run()
    b1.fetch()
    arr, carry, new_off, new_anchors = _match(lib, cb2, cb1, prev_read)
    assert np.array_equal(carry["parts"].astype(np.int64), expect) and int(expect.sum()) > 200
    h = C.c_void_p()
    eng._check(lib.rawdtw_batch_submit_carry(eng._ctx, C.byref(copt), cb2.n_reads, vp(arr[0]), vp(arr[1]), vp(arr[2]), vp(new_off), vp(new_anchors), vp(arr[3]),
                                             vp(arr[4]), b1._h, vp(carry), C.byref(h)))

    def fetch():
        score, keep, jc = np.zeros(nc, np.float32), np.zeros(nc, np.uint8), np.zeros(len(want[2]), np.float32)
        eng._check(lib.rawdtw_batch_fetch(eng._ctx, h, vp(score), vp(keep), vp(jc)))
        sc, ru = C.c_uint64(), C.c_uint64()
        eng._check(lib.rawdtw_batch_round_stats(eng._ctx, h, C.byref(sc), C.byref(ru)))
        return (score, keep, jc), (sc.value, ru.value)

    got, stats = fetch()
    same_bits(got, want, "carried round, first run")
    assert stats == (len(want[2]) - int(expect.sum()), int(expect.sum()))
    replays = (lambda: lib.rawdtw_batch_run(eng._ctx, h), lambda: lib.rawdtw_batch_enqueue(eng._ctx, h, 0),
               lambda: lib.rawdtw_batch_run_reps(eng._ctx, h, 2, None, None, 0, None))
    for k, replay in enumerate(replays):
        eng._check(replay())
        got, stats_k = fetch()
        same_bits(got, want, f"carried round, replay {k}")
        assert stats_k == stats
    lib.rawdtw_batch_destroy(h)
    b1.close()
    eng.close()
