"""Every device path that addresses the two arenas, at offsets past 2^30, 2^31 and 2^32 (tests/high_offset_cases.py; pinned on the CPU by
tests/test_high_offsets_cpu.py).  A 2^32 + 2^27-float reference arena and a 2^31 + 2^27-float event arena are adopted from torch: one
constant, the small segment at four places each, decoys of other content wherever a truncated offset would land.  Every job list and
batch runs at the places; every expected value is the low twin's, from the oracle and the host restatements on arrays of a segment's
size, and every comparison is bit for bit.  One sub-batch of each of the three tracebacks takes its direction workspace past 2^32 bytes."""
import ctypes as C
import gc

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch

    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import rawalign_amd as ra
from rawalign_amd.align import Batch
from rawalign_amd.dtw import ANCHOR_DTYPE
from tests import high_offset_cases as hc
from tests import test_banded_tb_gpu as bt
from tests import test_semiglobal_gpu as sg
from tests.util import assert_bits_equal, oracle_costs, planner_options

pytestmark = pytest.mark.gpu
COPIES = 16   # every job at every pair of places
HOOK = "RAWDTW_LOCAL_JOBS"   # read when a context is created: "host" brings the anchors home instead of k_local_jobs


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def torch_arena(n_floats, seg, decoy, places, decoy_places):
    """the arena on the device; out of memory is the only reason to skip (a stale HIP error left behind by the library would be a bug)"""
    assert torch is not None, "these tests adopt their arenas from torch"
    try:
        arena = torch.full((n_floats,), float(hc.FILL), dtype=torch.float32, device="cuda:0")
    except RuntimeError as err:
        if "out of memory" not in str(err).lower():
            raise
        pytest.skip("not enough device memory for an arena of %.1f GB" % (4e-9 * n_floats))
    s, d = torch.from_numpy(seg.copy()).cuda(), torch.from_numpy(decoy.copy()).cuda()
    for p in places:
        arena[p:p + len(seg)] = s
    for p in decoy_places:
        arena[p:p + len(decoy)] = d
    torch.cuda.synchronize()
    return arena


@pytest.fixture(scope="module")
def arenas():
    ref = torch_arena(hc.REF_FLOATS, hc.ref_segment(), hc.ref_decoy(), hc.REF_PLACES, hc.REF_DECOYS)
    ev = torch_arena(hc.EV_FLOATS, hc.ev_segment(), hc.ev_decoy(), hc.EV_PLACES, hc.EV_DECOYS)
    yield ref, ev
    del ref, ev
    gc.collect()
    torch.cuda.empty_cache()


def engine_on(arenas):
    ref, ev = arenas
    e = ra.Engine(0)
    e.set_reference_device(ref.data_ptr(), hc.REF_FLOATS, keepalive=ref)
    e.set_events_device(ev.data_ptr(), hc.EV_FLOATS, keepalive=ev)
    return e


@pytest.fixture(scope="module")
def eng(arenas):
    e = engine_on(arenas)
    yield e
    e.close()


# ---- 1: job-list bodies ------------------------------------------------------------------------------------------------------------------
def test_job_list_bodies_at_the_places(eng, oracle):
    """Engine.plan, events read from the arena: the 400-job mix (lane, group, wave, full and multi-strip bodies), each job at one pair of
    places, and behind it the banded classes the mix's radii do not reach, each at all sixteen pairs"""
    low, high = hc.spread(hc.score_jobs())
    wide_low, wide_high = hc.spread(hc.class_jobs(), COPIES)
    want = np.concatenate([oracle_costs(oracle, low, hc.ev_segment(), hc.ref_segment()),
                           np.repeat(oracle_costs(oracle, hc.class_jobs(), hc.ev_segment(), hc.ref_segment()), COPIES)])
    pl = eng.plan(np.concatenate([high, wide_high]))
    info = pl.info()
    assert info["n_jobs"] == 400 + 16 * len(hc.CLASS_K) and info["n_lane_jobs"] > 0 and info["n_wave_band_jobs"] > 16 * 5 and info["n_full_jobs"] > 0
    assert info["n_launches"] >= 8
    pl.run()
    got = pl.fetch()
    pl.close()
    assert_bits_equal(got, want, "job list at the places")
    ri, ei = hc.round_robin(400)
    big = low["n"] >= 200
    for r in range(4):   # every pair of places was hit by a banded and by a full job, every place by large ones of both kinds
        for e in range(4):
            sel = (ri == r) & (ei == e)
            assert (low["band_radius"][sel] < 0).any() and (low["band_radius"][sel] > 0).any()
        for at in (ri, ei):
            assert (low["band_radius"][big & (at == r)] < 0).any() and (low["band_radius"][big & (at == r)] > 0).any()


# ---- 2: candidate batches ----------------------------------------------------------------------------------------------------------------
def high_batch():
    rp, ep = hc.batch_places()
    return hc.shifted(hc.candidate_batch(), rp, ep)


def check_batch(got, want, what):
    assert_bits_equal(got[0], want[0], what + ": scores")
    assert np.array_equal(got[1], want[1]), what + ": keeps"
    assert_bits_equal(got[2], want[2], what + ": job costs")


FORMS = {"sparse_banded_device_plan": (dict(), 1), "sparse_banded_host_plan": (dict(), 0),
         "global_full": (dict(dtw_border_constraint=0, dtw_fill_method=0), 1), "global_banded": (dict(dtw_border_constraint=0, dtw_fill_method=1), 1)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_candidate_batches_at_the_places(eng, oracle, form):
    kw, dev = FORMS[form]
    opt = ra.MapOpt(**kw)
    want = hc.batch_expected(oracle, hc.candidate_batch(), opt)
    cb = high_batch()
    assert (cb.ref_base >= 1 << 32).any() and (cb.read_base >= 1 << 30).any() and (cb.read_base >= 1 << 31).any()
    with planner_options(eng, device_plan=dev, device_plan_min_jobs=0):
        b = Batch(eng, opt, cb)
        if not kw:
            assert b.verify_plan() == bool(dev)
        b.run()
        got = b.fetch(with_job_costs=True)
        b.close()
    check_batch(got, want, form)


class OnDevice:
    """device copies of a batch's anchors, ref_base and read_base, alive as long as this is"""

    def __init__(self, cb):
        arrs = (np.ascontiguousarray(cb.anchors, ANCHOR_DTYPE), np.ascontiguousarray(cb.ref_base, np.uint64), np.ascontiguousarray(cb.read_base, np.uint32))
        self.t = [torch.from_numpy(np.concatenate([a.view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])).to("cuda:0") for a in arrs]
        torch.cuda.synchronize()
        self.ptrs = [t.data_ptr() for t in self.t]


@pytest.mark.parametrize("how", ["host_arrays", "device_arrays", "device_arrays_jobs_on_host"])
def test_local_batches_at_the_places(arenas, how, monkeypatch):
    """the local border constraint: one semiglobal job a chain; from host arrays, and from device arrays with k_local_jobs writing the
    records or -- the hook set when the context is created -- the anchors brought home"""
    opt = ra.MapOpt(dtw_border_constraint=2)
    want = hc.local_expected(hc.candidate_batch(), opt)
    if how == "device_arrays_jobs_on_host":
        monkeypatch.setenv(HOOK, "host")
    e = engine_on(arenas)
    monkeypatch.delenv(HOOK, raising=False)
    e.set_border_local(True)
    cb = high_batch()
    if how == "host_arrays":
        b = Batch(e, opt, cb)
        b.run()
    else:
        dev = OnDevice(cb)
        b = Batch(e, opt, cb, device_ptrs=dev.ptrs)
    got = b.fetch(with_job_costs=True)
    assert b.hand_over_stats()["records_on_device"] == (cb.n_chains if how == "device_arrays" else 0)
    b.close()
    check_batch(got, want, how)
    e.close()


# ---- 3: semiglobal cost, span and traceback in the arena form ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def semi_want():
    cases = [(a, b, ex) for a, b, _, ex in hc.windows(hc.semiglobal_jobs())]
    want = sg.host_answers(cases)
    spans = [ra.semiglobal_span_host(a, b, ex) for a, b, ex in cases]
    rep = lambda xs: [x for x in xs for _ in range(COPIES)]  # noqa: E731
    return rep(cases), rep(want), rep(spans)


@pytest.mark.parametrize("full_wg", [1, 0])
def test_semiglobal_cost_span_and_traceback_at_the_places(eng, semi_want, full_wg):
    cases, want, spans = semi_want
    _, high = hc.spread(hc.semiglobal_jobs(), COPIES)
    assert len(high) == len(cases) == 22 * COPIES
    eng.set_option("full_wg", full_wg)
    try:
        cost, end_j = eng.semiglobal_batch(high)
        scost, sj0, send = eng.semiglobal_span(high)
        tb = eng.semiglobal_traceback(high)
        assert eng.get_option("tb_sub_batches") == 1
    finally:
        eng.set_option("full_wg", 1)
    sg.check_batch(cases, want, cost, end_j, "cost, full_wg %d" % full_wg)
    for k, (c, j0, ej) in enumerate(spans):
        assert (int(bits(scost[k])[0]), int(sj0[k]), int(send[k])) == (int(bits(c)[0]), j0, ej), ("span", full_wg, k)
    sg.check_paths(cases, want, tb, "paths, full_wg %d" % full_wg)


# ---- 4: the banded traceback in the arena form ---------------------------------------------------------------------------------------------
def test_banded_traceback_at_the_places(eng):
    """bands of 1, 3 and 17 chunks on planted paths that read a code from every chunk, both orientations"""
    low = hc.banded_jobs()
    cases = hc.windows(low)
    want = bt.host_answers(cases)
    assert all(len(w.i) > 0 and bits(w.cost)[0] == 0 for w in want)   # (the planted paths are inside their bands)
    _, high = hc.spread(low, COPIES)
    tb = eng.banded_traceback(high)
    assert eng.get_option("tb_sub_batches") == 1
    rep = lambda xs: [x for x in xs for _ in range(COPIES)]  # noqa: E731
    bt.check(rep(cases), rep(want), tb, "banded at the places")


# ---- 5: the full-matrix traceback over the arena as it lies ----------------------------------------------------------------------------------
def check_global_paths(jobs_of, want, got, what):
    """got = (cost, off, plen, step, dist); job k must answer want[jobs_of[k]] = the oracle's (cost, i, j, d)"""
    cost, off, plen, step, dist = got
    for k, w in enumerate(jobs_of):
        c, pi, pj, pd = want[w]
        s, n = int(off[k]), int(plen[k])
        assert n == len(pi) and bits(cost[k])[0] == bits(c)[0], (what, k, w)
        st = step[s:s + n]
        assert (n == 0 or st[0] == 0) and np.array_equal(np.cumsum(st & 1), pi) and np.array_equal(np.cumsum(st >> 1), pj), (what, k, w)
        assert np.array_equal(bits(dist[s:s + n]), bits(pd)), (what, k, w)


def test_traceback_arena_steps_at_the_places(eng, oracle):
    low = hc.traceback_jobs()
    want = [oracle.dtw_global_tb(a, b, ex) for a, b, _, ex in hc.windows(low)]
    _, high = hc.spread(low, COPIES)
    got = eng.traceback_arena_steps(high)
    assert eng.get_option("tb_sub_batches") == 1
    check_global_paths(np.repeat(np.arange(len(low)), COPIES), want, got, "arena steps at the places")


# ---- 6: append to, and fetch from, stretches at the event places -----------------------------------------------------------------------------
def test_events_fetch_from_the_places(eng):
    """k_events_gather: planted copies, decoys and the filler between them, as torch wrote them"""
    seg, decoy = hc.ev_segment(), hc.ev_decoy()
    starts = list(hc.EV_PLACES) + list(hc.EV_DECOYS)
    got = eng.events_fetch(starts, [hc.SEG_EV] * len(starts))
    for k, g in enumerate(got):
        assert np.array_equal(bits(g), bits(seg if k < 4 else decoy)), starts[k]
    odd = [(p + 12345, 777) for p in hc.EV_PLACES] + [((1 << 30) - 3, 7), ((1 << 31) - 5, 11), (hc.EV_FLOATS - 1, 1)]
    got = eng.events_fetch([s for s, _ in odd], [n for _, n in odd])
    for (s, n), g in zip(odd, got):
        o = s - max(p for p in hc.EV_PLACES if p <= s)
        assert np.array_equal(bits(g), bits(seg[o:o + n])), s
    between = eng.events_fetch([hc.EV_PLACES[1] - 100, hc.EV_PLACES[3] - 100], [100, 100])
    assert all((bits(g) == bits(hc.FILL)[0]).all() for g in between)


GUARD = 64


def test_append_events_to_the_places():
    """k_events_scatter into a reserved arena of EV_FLOATS: stretches of odd lengths at odd offsets inside every place, the last one
    ending with the arena.  Where a truncated destination would land lies a canary, appended first (all of those lie below 2^30); the
    canaries and a guard band on both sides of every destination are the same bits before and after, and the stretches come back."""
    e = ra.Engine(0)
    try:
        e.reserve_events(hc.EV_FLOATS)
    except ra.RawDTWError as err:
        if err.status != 2:   # RAWDTW_ERR_OOM
            raise
        pytest.skip("not enough device memory for a reserved arena of %.1f GB" % (4e-9 * hc.EV_FLOATS))
    rng = np.random.default_rng(1217)
    lens = [1, 255, 1001, 4097]
    dst, pieces = [], []
    for p in hc.EV_PLACES[1:]:
        at = p + (1 if p % 2 == 0 else 0)   # odd offsets throughout
        for ln in lens:
            dst.append(at)
            pieces.append(rng.normal(size=ln).astype(np.float32))
            at += ln + 2 * GUARD + ln % 2
    # the straddling places: one stretch across the mark itself, beginning 333 floats below it
    for mark in (hc.MARK_30, hc.MARK_31):
        dst.append(mark - 333)
        pieces.append(rng.normal(size=1001).astype(np.float32))
    dst.append(hc.EV_FLOATS - 513)   # ends with the arena
    pieces.append(rng.normal(size=513).astype(np.float32))
    dst, ln = np.array(dst, np.int64), np.array([len(x) for x in pieces], np.int64)
    order = np.argsort(dst)
    assert (dst[order][1:] >= (dst + ln)[order][:-1] + 2 * GUARD).all() and (dst % 2 == 1).all() and (dst + ln).max() == hc.EV_FLOATS
    assert (dst >= hc.MARK_31).sum() >= 5 and ((dst >= hc.MARK_30) & (dst < hc.MARK_31)).sum() >= 5
    # canaries where dst mod 2^30 and dst mod 2^31 lie (all below 2^30), with room for the longest stretch and a guard; overlapping ones
    # are merged, and one that would touch a destination is left out (a truncated write then lands in that destination's own stretch)
    alias = sorted({int(d % w) for d in dst for w in (hc.MARK_30, hc.MARK_31) if d % w != d})
    room = int(ln.max()) + GUARD
    spans = []
    for a in alias:
        lo_a, hi_a = max(a - GUARD, 0), a + room
        if not ((hi_a + GUARD <= dst) | (dst + ln + GUARD <= lo_a)).all():
            continue
        if spans and lo_a <= spans[-1][1]:
            spans[-1][1] = max(spans[-1][1], hi_a)
        else:
            spans.append([lo_a, hi_a])
    assert len(alias) >= 9 and sum(any(lo_a <= a < hi_a for lo_a, hi_a in spans) for a in alias) >= 8 and spans[-1][1] < hc.MARK_30
    lo = np.array([x[0] for x in spans], np.int64)
    canary = [rng.normal(size=x[1] - x[0]).astype(np.float32) for x in spans]
    e.append_events(np.concatenate(canary), np.concatenate([[0], np.cumsum([len(c) for c in canary])]).astype(np.uint64), lo.astype(np.uint32))
    watch_at = np.concatenate([lo, dst - GUARD, np.minimum(dst + ln, hc.EV_FLOATS - GUARD)])
    watch_ln = np.concatenate([np.array([len(c) for c in canary], np.int64), np.full(2 * len(dst), GUARD)])
    before = e.events_fetch(watch_at, watch_ln)
    for k in range(len(lo)):
        assert np.array_equal(bits(before[k]), bits(canary[k])), k
    src = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64)
    e.append_events(np.concatenate(pieces), src, dst.astype(np.uint32))
    back = e.events_fetch(dst, ln)
    for k, x in enumerate(pieces):
        assert np.array_equal(bits(back[k]), bits(x)), (k, int(dst[k]))
    after = e.events_fetch(watch_at, watch_ln)
    last = int(np.argmax(dst))   # (the guard "behind" the stretch that ends with the arena is the stretch's own tail)
    for k, (x, y) in enumerate(zip(before, after)):
        if k == len(lo) + len(dst) + last:
            continue
        assert np.array_equal(bits(x), bits(y)), (k, int(watch_at[k]))
    e.close()


# ---- 8: one sub-batch whose direction workspace passes 2^32 bytes ---------------------------------------------------------------------------
def tb_timing(e):
    f, w, d, n = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
    e._check(e.lib.rawdtw_traceback_timing(e._ctx, C.byref(f), C.byref(w), C.byref(d), C.byref(n)))
    return {"direction_bytes": d.value, "path_elements": n.value}


@pytest.mark.parametrize("kind", ["full", "semiglobal", "banded"])
def test_one_sub_batch_with_directions_past_4_gib(eng, oracle, kind):
    """a few hundred jobs cycling over seven windows, at the places: every job's direction offset is 64-bit arithmetic in the fill and
    in the walk, and the jobs behind the mark answer what their window answers anywhere"""
    low, high, which = hc.direction_jobs(kind)
    win = hc.windows(hc.direction_windows(kind))
    if kind == "full":
        want = [oracle.dtw_global_tb(a, b, ex) for a, b, _, ex in win]
        got = eng.traceback_arena_steps(high)
        written = tb_timing(eng)["direction_bytes"]
    elif kind == "semiglobal":
        want = sg.host_answers([(a, b, ex) for a, b, _, ex in win])
        got = eng.semiglobal_traceback(high)
        written = eng.semiglobal_timing()["direction_bytes"]
    else:
        want = bt.host_answers(win)
        got = eng.banded_traceback(high)
        written = eng.banded_traceback_timing()["direction_bytes"]
    assert eng.get_option("tb_sub_batches") == 1
    assert written == hc.direction_total(kind, low) > hc.DIR_FLOOR > 1 << 32
    if kind == "full":
        check_global_paths(which, want, got, kind)
    elif kind == "semiglobal":
        sg.check_paths([(win[w][0], win[w][1], win[w][3]) for w in which], [want[w] for w in which], got, kind)
    else:
        bt.check([win[w] for w in which], [want[w] for w in which], got, kind)


# ---- 7: the resident pipeline at the event places ------------------------------------------------------------------------------------------
SENTINEL = 0x5EA7BEEF   # no event has these bits (tests/test_signal_round_gpu.py)
SLOT_ROOM, PIPE_READS = 1024, 40


def pipeline_places():
    """(dst of the low twin, dst of the high twin): 1 024-float stretches, ten around 2^30 (one of them across it), ten around 2^31, ten at
    the arena's end (the last ends with it) and ten low; odd starts except at the very end"""
    lo = 1 + np.arange(PIPE_READS, dtype=np.int64) * SLOT_ROOM
    hi = np.zeros(PIPE_READS, np.int64)
    for k in range(PIPE_READS):
        j, where = k // 4, k % 4
        hi[k] = (1 + j * SLOT_ROOM, hc.MARK_30 - 5 * SLOT_ROOM + 1 + j * SLOT_ROOM, hc.MARK_31 - 5 * SLOT_ROOM + 1 + j * SLOT_ROOM,
                 hc.EV_FLOATS - (10 - j) * SLOT_ROOM)[where]
    assert ((hi < hc.MARK_30) & (hi + SLOT_ROOM > hc.MARK_30)).any() and ((hi < hc.MARK_31) & (hi + SLOT_ROOM > hc.MARK_31)).any()
    assert (hi + SLOT_ROOM).max() == hc.EV_FLOATS and len(set(hi.tolist())) == PIPE_READS
    return lo, hi


def sentinel_arena(e, n):
    t = torch.full((int(n),), SENTINEL, dtype=torch.int32, device="cuda:0")
    e.set_events_device(t.data_ptr(), t.numel(), keepalive=t)
    return t


@pytest.mark.parametrize("kind", ["pa", "raw"])
def test_the_resident_pipeline_at_the_places(arenas, kind):
    """detect_resident (dst_start), seed_resident (ev_start), a device chain round on the resident hits (read_base at the places, key_base
    beyond 2^32) and rawdtw_batch_submit_device on its device arrays, on a sentinel-filled arena of EV_FLOATS against the same calls on
    a small one: event counts, the stretches with the sentinel on both sides, hits, chain records, anchors, scores, keeps and job costs
    are the low twin's.  (The chains' ref_base and read_base stay on the device; the scores and job costs answer for them: any other
    window holds other signals or the sentinel.)"""
    from rawalign_amd import mapping as M
    from rawalign_amd.align import CandidateBatch
    from rawalign_amd.dtw import CHAIN_REC_DTYPE, SEED_DTYPE
    from rawalign_amd.rawsig import Channel
    from rawalign_amd.seeding import SeedIndex
    from tests import map_ref_cases as mc

    ref = mc.make_reference()
    six = SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)
    wins = [np.ascontiguousarray(sig[i:i + 1000], np.float32) for sig in mc.make_raw_reads() for i in range(0, len(sig) - 999, 1000)][:PIPE_READS]
    assert len(wins) == PIPE_READS
    chan = None
    if kind == "raw":
        chan = Channel(8192.0, 1450.0, 3.0)
        wins = [np.round(w * (chan.digitisation / chan.range) - chan.offset).astype(np.int16) for w in wins]
    data = np.concatenate(wins)
    off = np.arange(PIPE_READS + 1, dtype=np.uint64) * 1000
    dst_lo, dst_hi = pipeline_places()
    room = np.full(PIPE_READS, SLOT_ROOM - 2, np.uint32)   # (a float of sentinel stays on both sides of every stretch)
    n_keys = 2 * len(ref.forward)
    rel = np.arange(n_keys, dtype=np.int64) * 20000 + 7
    key_place = np.array(hc.REF_PLACES, np.int64)[[2, 3, 1, 3, 0, 2][:n_keys]]
    copt = M.default_chain_opt(mc.E)
    opt = ra.MapOpt()
    results = {}
    for twin, dst in (("low", dst_lo), ("high", dst_hi)):
        e = ra.Engine(0)
        try:
            if twin == "low":
                e.upload_reference([hc.ref_segment()], [hc.ref_segment()])
                key_base = (rel + e.reference_offset(0, 1)).astype(np.uint64)
                arena = sentinel_arena(e, PIPE_READS * SLOT_ROOM + 8)
            else:
                e.set_reference_device(arenas[0].data_ptr(), hc.REF_FLOATS, keepalive=arenas[0])
                key_base = (rel + key_place).astype(np.uint64)
                assert (key_base >= 1 << 32).sum() >= 2
                try:
                    arena = sentinel_arena(e, hc.EV_FLOATS)
                except RuntimeError as err:
                    if "out of memory" not in str(err).lower():
                        raise
                    pytest.skip("not enough device memory for a second event arena")
            e.upload_seed_index(six)
            ev_len, s_len, total = e.detect_resident(data, off, dst.astype(np.uint64), room, chan=chan)
            assert total == int(ev_len.sum()) > 40 * PIPE_READS and ev_len.max() <= SLOT_ROOM - 2
            stretches = e.events_fetch(dst - 1, ev_len.astype(np.int64) + 2)
            rs = e.seed_resident(dst.astype(np.uint64), ev_len)
            hits = rs.fetch()
            hoff = rs.hit_off.astype(np.uint64)
            n = PIPE_READS
            cap = n * 32
            chain_off, anchor_off = np.zeros(n + 1, np.uint64), np.zeros(cap + 1, np.uint64)
            recs, anchors = np.zeros(cap, CHAIN_REC_DTYPE), np.zeros(int(hoff[-1]) + 1, ANCHOR_DTYPE)
            prev_off, prev_all = np.zeros(n + 1, np.uint64), np.zeros(1, SEED_DTYPE)
            chunk_start, sits = np.zeros(n, np.uint32), (ev_len < 6).astype(np.uint8)
            assert not sits.any()
            read_base = dst.astype(np.uint32)
            vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
            e._check(e.lib.rawdtw_chain_round_begin_resident(e._ctx, C.byref(copt), n, vp(hoff), vp(prev_off), vp(prev_all), vp(chunk_start), vp(sits),
                                                             vp(read_base), n_keys, vp(key_base), vp(chain_off), vp(anchor_off), vp(recs), cap, vp(anchors)))
            d = [C.c_void_p() for _ in range(3)]
            e._check(e.lib.rawdtw_chain_round_end(e._ctx, *[C.byref(x) for x in d]))
            nc = int(chain_off[-1])
            na = int(anchor_off[nc])
            assert nc >= n // 2 and na > 4 * nc
            read_of = np.repeat(np.arange(n), np.diff(chain_off.astype(np.int64)))
            cb = CandidateBatch(None, chain_off, anchor_off[:nc + 1], anchors[:na], key_base[recs["key"][:nc]], read_base[read_of])
            b = Batch(e, opt, cb, device_ptrs=[x.value for x in d])
            got = b.fetch(with_job_costs=True)
            b.close()
            results[twin] = dict(ev_len=ev_len, s_len=s_len, stretches=[bits(x) for x in stretches], hit_off=hoff, hits=hits.tobytes(), chain_off=chain_off,
                                 anchor_off=anchor_off[:nc + 1], recs=recs[:nc].tobytes(), anchors=anchors[:na].tobytes(), score=bits(got[0]), keep=got[1],
                                 costs=bits(got[2]), ref_rel=cb.ref_base.astype(np.int64), read_base=cb.read_base.astype(np.int64))
            del arena
        finally:
            e.close()
    lo, hi = results["low"], results["high"]
    for k, (x, y) in enumerate(zip(lo["stretches"], hi["stretches"])):
        assert x[0] == SENTINEL == x[-1] and (x[1:-1] != SENTINEL).all() and np.array_equal(x, y), (kind, k)
    for key in ("ev_len", "s_len", "hit_off", "chain_off", "anchor_off", "score", "keep", "costs"):
        assert np.array_equal(lo[key], hi[key]), (kind, key)
    for key in ("hits", "recs", "anchors"):
        assert lo[key] == hi[key], (kind, key)
    # (chains and their jobs; the key bases point into random signals, so most scores are the early exit's -1e10: the job costs carry the check)
    assert len(lo["costs"]) >= len(lo["score"]) >= PIPE_READS // 2
    read_of = np.repeat(np.arange(PIPE_READS), np.diff(lo["chain_off"].astype(np.int64)))
    assert np.array_equal(hi["read_base"] - lo["read_base"], (dst_hi - dst_lo)[read_of])
    assert (hi["ref_rel"] >= 1 << 32).any() and (hi["read_base"] >= 1 << 31).any()
