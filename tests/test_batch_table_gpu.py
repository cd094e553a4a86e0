"""What the batch's launch table, its input record and its one statistics fetch must keep (rawdtw_batch.cpp, rawdtw_launches.h), on the
`tiny` and `medium` cases of tests/replay_cases.py:

  a caller's buffer smaller than the launch count gets the full count and exactly `cap` entries;
  rawdtw_batch_submit_device leaves the context as it found it -- "resident_arrays" and whether a later plain create sends the side
  list's launch with the planning launches -- also when it fails;
  rawdtw_batch_launch_stats asked again, with and without cells, says the same, and rawdtw_batch_info after it says what it says on a
  batch nobody asked before.

"No side-list launch at create" is observed through the results, not through rawdtw_batch_wide_ms: that call returns the time between
two events recorded one behind the other when no launch lies between them, and two such events are never 0.0 apart (5.6 us on an MI355X,
with this library and with the one before it alike).  A run over events uploaded AFTER the create shows the same thing exactly: a side
list scored at create would carry the costs of the events of the create."""
import ctypes as C
import math

import numpy as np
import pytest

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

import rawalign_amd as ra
from tests.replay_cases import case

pytestmark = pytest.mark.gpu

KIND_FOLD, KIND_SELECT, KIND_WREG, KIND_MERGED = 6, 7, 8, 10  # rawdtw_launches.h: kKindChainFold, kKindReadSelect, kKindBandWreg, kKindBandMerged
SENTINEL_MS, SENTINEL_KIND = np.float32(-7.5), np.uint32(0xDEADBEEF)


def vp(x):
    return C.c_void_p(x.ctypes.data)


def _timed(eng, b, call, cap):
    """call(ctx, batch, ms, kind, cap, &n, ...) on arrays of cap + 3 entries: (n, ms, kind, what the call's further outputs hold)"""
    ms, kind = np.full(cap + 3, SENTINEL_MS, np.float32), np.full(cap + 3, SENTINEL_KIND, np.uint32)
    n, runs = C.c_uint32(), C.c_uint32(12345)
    extra = (C.byref(runs),) if call == "rawdtw_batch_collect" else ()
    eng._check(getattr(eng.lib, call)(eng._ctx, b._h, vp(ms), vp(kind), cap, C.byref(n), *extra))
    return n.value, ms, kind, runs.value


@pytest.mark.parametrize("which,options", [("tiny", {}), ("medium", {"device_plan": 0})], ids=["stream", "job_list"])
def test_small_caller_buffer(oracle, which, options):
    cs = case(which)
    eng = cs.engine(**options)
    b = cs.batch(eng)
    assert b.verify_plan() is (not options)
    n_full, ms_full, kind_full, _ = _timed(eng, b, "rawdtw_batch_run_timed", 64)
    assert 3 <= n_full <= 64 and list(kind_full[n_full - 2:n_full] & 0xFF) == [KIND_FOLD, KIND_SELECT]
    assert np.all(kind_full[n_full:] == SENTINEL_KIND) and np.all(ms_full[n_full:] == SENTINEL_MS)
    n, ms, kind, _ = _timed(eng, b, "rawdtw_batch_run_timed", 1)
    assert n == n_full and kind[0] == kind_full[0] and math.isfinite(ms[0]) and ms[0] >= 0.0
    assert np.all(kind[1:] == SENTINEL_KIND) and np.all(ms[1:] == SENTINEL_MS)
    for _ in range(2):
        b.enqueue(True)
    n, ms, kind, runs = _timed(eng, b, "rawdtw_batch_collect", 1)
    assert (n, runs) == (n_full, 2) and kind[0] == kind_full[0] and math.isfinite(ms[0]) and ms[0] >= 0.0
    assert np.all(kind[1:] == SENTINEL_KIND) and np.all(ms[1:] == SENTINEL_MS)
    n, ms, kind, runs = _timed(eng, b, "rawdtw_batch_collect", 64)  # (nothing enqueued since: the full list, no time)
    assert (n, runs) == (n_full, 0) and np.array_equal(kind[:n], kind_full[:n_full]) and np.all(ms[:n] == 0.0)
    cs.check(oracle, b.fetch(with_job_costs=True), "A", "A", what="after the timed runs")
    eng.close()


def _submit_device(eng, cs, copt):
    """rawdtw_batch_submit_device on device copies of the case's anchors, ref_base and read_base: (status, handle, the copies)"""
    cb = cs.candidate_batch(eng)
    host = [np.ascontiguousarray(cb.chain_off, np.uint64), np.ascontiguousarray(cb.anchor_off, np.uint64)]
    dev = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to("cuda:0") for x in (cb.anchors, cb.ref_base, cb.read_base)]
    torch.cuda.synchronize()
    h = C.c_void_p()
    st = eng.lib.rawdtw_batch_submit_device(eng._ctx, C.byref(copt), cb.n_reads, vp(host[0]), vp(host[1]), *(C.c_void_p(d.data_ptr()) for d in dev), C.byref(h))
    return st, h, (host, dev)


def _fetch(eng, cs, h):
    nc = int(cs.chain_off[-1])
    n_jobs = int(np.maximum(np.diff(cs.anchor_off.astype(np.int64)) - 1, 0).sum())  # (align_chain: n_anchors - 1 parts a chain, rmap.cpp:248)
    score, keep, jc = np.zeros(nc, np.float32), np.zeros(nc, np.uint8), np.zeros(n_jobs, np.float32)
    eng._check(eng.lib.rawdtw_batch_fetch(eng._ctx, h, vp(score), vp(keep), vp(jc)))
    return score, keep, jc


@pytest.mark.parametrize("which", ["tiny", "medium"])
def test_submit_device_leaves_the_context_unchanged(oracle, which):
    cs = case(which)
    eng = cs.engine(time_plan=1)
    assert eng.get_option("resident_arrays") == 0 and eng.get_option("wide_at_create") == 0
    st, h, alive = _submit_device(eng, cs, cs.opt.c_struct())
    assert st == 0 and h.value, eng.lib.rawdtw_last_error(eng._ctx)
    cs.check(oracle, _fetch(eng, cs, h), "A", "A", what="rawdtw_batch_submit_device")
    eng.lib.rawdtw_batch_destroy(h)
    assert eng.get_option("resident_arrays") == 0
    b = cs.batch(eng, submit=True)  # host arrays: a context left with device arrays switched on would read them as device memory
    cs.check(oracle, b.fetch(with_job_costs=True), "A", "A", what="rawdtw_batch_submit behind rawdtw_batch_submit_device")
    assert b.verify_plan() is True and eng.get_option("resident_arrays") == 0
    b.close()
    # the same where the first call fails
    bad = cs.opt.c_struct()
    bad.border_constraint = 2
    st, h, alive = _submit_device(eng, cs, bad)
    assert st == 1 and not h.value  # RAWDTW_ERR_INVALID
    assert eng.get_option("resident_arrays") == 0
    # A plain create behind it: the side list's launch waits for the run.  Other events go up between the create and the run, and the run
    # is held to the oracle on THOSE: a launch that had gone out with the planning launches would have scored the side list's parts on the
    # events of the create.
    b = cs.batch(eng)
    cs.upload(eng, "B")
    b.run()
    cs.check(oracle, b.fetch(with_job_costs=True), "B", "A", what="rawdtw_batch_create behind a failed rawdtw_batch_submit_device, other events before the run")
    assert b.verify_plan() is True and cs.costs_mostly_differ(("A", "A"), ("B", "A"))
    assert which == "tiny" or b.stream_counters()["side_jobs"] > 0  # (medium: the side list has parts, the check above bites)
    print("wide_ms of a plain create behind the failed submit:", b.wide_ms())
    b.close()
    eng.close()


@pytest.mark.parametrize("which", ["tiny", "medium"])
def test_repeated_statistics(oracle, which):
    cs = case(which)
    eng = cs.engine()
    fresh = cs.batch(eng)
    want_info = fresh.info()  # (a batch nobody asked for launch statistics)
    fresh.close()
    b = cs.batch(eng)
    assert b.verify_plan() is True
    stats = [b.launch_stats(with_cells=False), b.launch_stats(with_cells=True), b.launch_stats(with_cells=False)]
    figures = [[(s["kind"], s["param"], s["n_jobs"], s["algorithmic_bytes"]) for s in st] for st in stats]
    assert figures[0] == figures[1] == figures[2], figures
    assert [k for k, _, _, _ in figures[0]] == [KIND_WREG, KIND_MERGED, KIND_FOLD, KIND_SELECT]
    assert figures[0][1][2] > 0 and figures[0][1][3] > 0  # the tiles' launch has jobs and bytes
    info = b.info()
    assert info == want_info, (info, want_info)
    assert sum(s["cells"] for s in stats[1]) == info["cells"] and sum(n for _, _, n, _ in figures[0][:2]) == info["n_jobs"]
    assert sum(s["algorithmic_bytes"] for s in stats[1][:2]) == info["algorithmic_bytes"]
    b.run()
    cs.check(oracle, b.fetch(with_job_costs=True), "A", "A", what="after the statistics")
    eng.close()
