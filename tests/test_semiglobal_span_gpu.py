"""The semiglobal span on the device (include/rawdtw.h, "span": rawdtw_semiglobal_span_batch, rawdtw_dtw_semiglobal_span; kernel:
k_semi_span_wave in rawdtw_semiglobal_kernels.hip), bit for bit: (cost, j0, end_j) against the reference's recorded answers
(tests/golden/semiglobal_ref.npz) where there is one, against rawdtw_semiglobal_span_host elsewhere (tests/test_semiglobal_span_cpu.py
holds it to the fixture, the live reference and the O(n m) host path), and against out_j0 of rawdtw_semiglobal_traceback_steps on the same
jobs in the same context.  The largest matrix is 2561 x 1000 cells."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import synth
from rawalign_amd.dtw import JOB_DTYPE
from tests import semiglobal_cases as sc
from tests import semiglobal_span_cases as sp
from tests import value_cases as vc
from tests.util import make_arena_jobs

pytestmark = pytest.mark.gpu
INVALID, RANGE = 1, 4


def engine_for(cases, **options):
    """-> (engine, jobs, events): every b in the engine's reference arena, every a in `events`, FULL jobs over them"""
    jobs, ev, rf = make_arena_jobs([(a, b, -1, ex) for a, b, ex in cases])
    eng = ra.Engine(0)
    for name, value in options.items():
        eng.set_option(name, value)
    eng.upload_reference([rf], [rf])
    jobs["ref_off"] += eng.reference_offset(0, 1)
    return eng, jobs, ev


def host_spans(cases):
    return [ra.semiglobal_span_host(a, b, ex) for a, b, ex in cases]


def check_spans(cases, want, got, what, tb_j0=None):
    cost, j0, end_j = got
    for k, ((a, b, ex), (wc, wj0, wej)) in enumerate(zip(cases, want)):
        assert sc.bits(cost[k])[0] == sc.bits(wc)[0] and j0[k] == wj0 and end_j[k] == wej, \
            (what, k, len(a), len(b), ex, (cost[k], j0[k], end_j[k]), (wc, wj0, wej))
    if tb_j0 is not None:
        assert np.array_equal(j0, tb_j0), (what, np.nonzero(j0 != tb_j0)[0][:8])


@pytest.fixture(scope="module")
def sweep():
    cases = sp.sweep_cases()
    return cases, host_spans(cases)


def test_fixture_spans():
    """the 173 recorded cases in one call, exclude_last 0 and 1: _slow's cost bits, end_j, and element 0 of DTW_semiglobal_tb's path"""
    fx = sc.Fixture()
    cases = [fx.inputs(k) + (ex,) for k in range(len(fx)) for ex in (0, 1)]
    eng, jobs, ev = engine_for(cases)
    cost, j0, end_j = eng.semiglobal_span(jobs, ev)
    tb_j0 = eng.semiglobal_traceback(jobs, ev)[1]
    moved = 0
    for q, (a, b, ex) in enumerate(cases):
        k = q // 2
        want_j0 = int(fx.path(k, 0)[1][0])  # (the flag does not change j0; with it the path of a one-row job is empty)
        assert sc.bits(cost[q])[0] == fx.z["slow"][k, ex] and end_j[q] == fx.z["end_j"][k] and j0[q] == want_j0, (fx.tag(k), k, ex)
        assert tb_j0[q] == want_j0 or (ex and len(a) == 1), (fx.tag(k), k, ex)
        moved += want_j0 != 0
    assert moved >= 200


def test_sweep_in_job_order_and_shuffled(sweep):
    """n at every class and strip edge (1, 2; 64/65, 128/129, 256/257; 512/513; 1024/1025; 1537; 2561: six strips, the four-slot ring
    of boundary rows reuses slots 0 and 1) x m on both sides of the 64-column chunk; shuffled, the classes lie scattered through the
    outputs"""
    cases, want = sweep
    assert max(len(a) for a, _, _ in cases) == 2561
    eng, jobs, ev = engine_for(cases)
    tb_j0 = eng.semiglobal_traceback(jobs, ev)[1]
    check_spans(cases, want, eng.semiglobal_span(jobs, ev), "sweep", tb_j0)
    perm = np.random.default_rng(7).permutation(len(cases))
    check_spans([cases[k] for k in perm], [want[k] for k in perm], eng.semiglobal_span(jobs[perm], ev), "shuffled", tb_j0[perm])
    for (a, b, ex), (c, s, e) in zip(cases, want):
        assert len(a) > 1 or s == e
        assert len(b) > 1 or s == 0


def test_many_strips_on_one_wave(sweep):
    """the shapes of the pipelined class with "full_wg" off: one wave carries the starts through up to six strips, in place in one row"""
    cases, want = sweep
    pick = [k for k, (a, _, _) in enumerate(cases) if len(a) in sp.PIPELINED_N]
    assert len(pick) == 2 * len(sp.PIPELINED_N) * len(sc.SWEEP_M)
    sub = [cases[k] for k in pick]
    eng, jobs, ev = engine_for(sub, full_wg=0)
    check_spans(sub, [want[k] for k in pick], eng.semiglobal_span(jobs, ev), "one wave", eng.semiglobal_traceback(jobs, ev)[1])


def test_planted_starts():
    """a copy of a planted so that the path starts in column 0, 63, 64, 65 and six chunks or more before its end; j0 against the
    constructed number.  Two equal minima: the first end and its own start.  n > m: column 0 all the way"""
    cases, starts = [], []
    for n in sp.PLANT_N:
        for at, j0 in sp.planted_starts(n):
            a, b = sc.planted(n, sp.PLANT_M, (at,))
            cases.append((a, b, at & 1))
            starts.append((0, j0, at))
    for n, m, ats in ((20, 200, (63, 128)), (130, 700, (200, 650)), (600, 1300, (620, 1299))):
        a, b = sc.planted(n, m, ats)
        cases.append((a, b, 0))
        starts.append((0, ats[0] - n + 1, ats[0]))
    eng, jobs, ev = engine_for(cases)
    cost, j0, end_j = eng.semiglobal_span(jobs, ev)
    assert [(int(sc.bits(c)[0]), int(s), int(e)) for c, s, e in zip(cost, j0, end_j)] == starts
    assert np.array_equal(j0, eng.semiglobal_traceback(jobs, ev)[1])
    rng = np.random.default_rng(31)
    tall = [(rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32), q & 1) for q, (n, m) in enumerate(sc.TALL)]
    for n, m in sc.TALL + ((1100, 3),):  # every column but the first forty away: the path runs up column 0
        b = np.full(m, 40.0, np.float32)
        b[0] = 0.0
        tall.append((rng.normal(size=n).astype(np.float32), b, 0))
    eng, jobs, ev = engine_for(tall)
    got = eng.semiglobal_span(jobs, ev)
    check_spans(tall, host_spans(tall), got, "tall")
    assert not got[1][len(sc.TALL):].any() and not got[2][len(sc.TALL):].any() and got[1][1] == 0  # (and m == 1)
    assert np.array_equal(got[1], eng.semiglobal_traceback(jobs, ev)[1])


def test_value_domains():
    """every value domain (costs below, around and far above 1e10, subnormals, zeros, spikes, integers) over DOMAIN_SHAPES: the
    predicates are the traceback fill's, so j0 is the traceback's whatever the values"""
    cases = []
    for name in vc.DOMAIN_NAMES:
        rng = vc.domain_rng(name, salt=47)
        for n, m in sc.DOMAIN_SHAPES:
            cases.append((vc.DOMAINS[name](rng, n), vc.DOMAINS[name](rng, m), len(cases) & 1))
    eng, jobs, ev = engine_for(cases)
    tb = eng.semiglobal_traceback(jobs, ev)
    got = eng.semiglobal_span(jobs, ev)
    one_row = np.array([len(a) == 1 and ex == 1 for a, _, ex in cases])  # (the traceback's path is empty there)
    assert np.array_equal(got[1][~one_row], tb[1][~one_row]) and np.array_equal(sc.bits(got[0]), sc.bits(tb[0]))
    check_spans(cases, host_spans(cases), got, "domains")


def raw_span(eng, jobs, ev, pad=16):
    """the C call with canaries behind the three outputs -> (status, cost, j0, end_j) as they lie, pad included"""
    jobs = np.ascontiguousarray(jobs, JOB_DTYPE)
    cost = np.full(len(jobs) + pad, -7.5, np.float32)
    j0 = np.full(len(jobs) + pad, 0xABCD1234, np.uint32)
    end_j = np.full(len(jobs) + pad, 0x1234ABCD, np.uint32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    st = eng.lib.rawdtw_semiglobal_span_batch(eng._ctx, ptr(jobs), len(jobs), None if ev is None else ptr(ev), 0 if ev is None else len(ev),
                                              ptr(cost), ptr(j0), ptr(end_j))
    return st, cost, j0, end_j


def untouched(cost, j0, end_j, frm=0):
    return bool(np.all(cost[frm:] == np.float32(-7.5)) and np.all(j0[frm:] == 0xABCD1234) and np.all(end_j[frm:] == 0x1234ABCD))


def test_arena_form_and_canaries():
    """500 jobs of every class over shared arenas, windows flush against both ends of both arenas; h_events given and h_events == NULL
    (the event arena as it lies); nothing is written behind the jobs' results"""
    rng = np.random.default_rng(626)
    ev = rng.normal(size=6000).astype(np.float32)
    rf = (np.round(rng.normal(size=9000) * 2) / 2).astype(np.float32)
    eng = ra.Engine(0)
    eng.upload_reference([rf], [rf])
    base = eng.reference_offset(0, 1)
    jobs = np.zeros(500, JOB_DTYPE)
    tops = (64, 128, 256, 700, 1300)
    for k in range(len(jobs)):
        c = k % 5 if k % 40 else 4
        n = int(rng.integers(1 if c == 0 else tops[c - 1] + 1, tops[c] + 1))
        m = int(rng.integers(1, 40 if c == 4 else 300))
        jobs[k] = (base + int(rng.integers(0, len(rf) - m + 1)), int(rng.integers(0, len(ev) - n + 1)), n, m, -1, k & 1, 0)
    jobs[0]["read_off"], jobs[0]["ref_off"] = 0, base
    jobs[1]["read_off"], jobs[1]["ref_off"] = len(ev) - int(jobs[1]["n"]), base + len(rf) - int(jobs[1]["m"])
    jobs[7]["read_off"], jobs[7]["ref_off"] = len(ev) - int(jobs[7]["n"]), base
    assert len(set(np.searchsorted(tops, jobs["n"]))) == 5
    cases = [(ev[j["read_off"]:j["read_off"] + j["n"]], rf[int(j["ref_off"]) - base:int(j["ref_off"]) - base + j["m"]], int(j["exclude_last"])) for j in jobs]
    want = host_spans(cases)
    st, cost, j0, end_j = raw_span(eng, jobs, ev)
    assert st == 0 and untouched(cost, j0, end_j, len(jobs))
    check_spans(cases, want, (cost, j0, end_j), "h_events form")
    eng2 = ra.Engine(0)
    eng2.upload_reference([rf], [rf])
    eng2.upload_events(ev)
    for again in range(2):
        st, cost, j0, end_j = raw_span(eng2, jobs, None)
        assert st == 0 and untouched(cost, j0, end_j, len(jobs))
        check_spans(cases, want, (cost, j0, end_j), "arena form %d" % again)
    check_spans(cases, want, eng2.semiglobal_span(jobs), "Engine.semiglobal_span")


def test_refusals_leave_outputs_and_context_alone():
    rng = np.random.default_rng(828)
    cases = [(rng.normal(size=30).astype(np.float32), rng.normal(size=50).astype(np.float32), 0),
             (rng.normal(size=70).astype(np.float32), rng.normal(size=20).astype(np.float32), 1)]
    want = host_spans(cases)
    eng, jobs, ev = engine_for(cases)

    def refused(status, events=ev, **change):
        bad = jobs.copy()
        for name, value in change.items():
            bad[name][1] = value
        st, cost, j0, end_j = raw_span(eng, bad, events)
        assert st == status and untouched(cost, j0, end_j), (change, st)
        with pytest.raises(ra.RawDTWError) as e:  # the cost form refuses the same list with the same status
            eng.semiglobal_batch(bad, events)
        assert e.value.status == status, change
        check_spans(cases, want, eng.semiglobal_span(jobs, ev), "after %r" % (change,))  # a good call on the same context

    refused(INVALID, n=0)
    refused(INVALID, m=0)
    refused(INVALID, band_radius=0)
    refused(INVALID, band_radius=5)
    refused(RANGE, read_off=len(ev) - 69)
    refused(RANGE, ref_off=2 ** 33)
    refused(RANGE, ref_off=2 ** 40)
    eng.upload_events(ev)  # the arena form reads the arena as it lies: 100 events there, the window would end at 101
    refused(RANGE, events=None, read_off=31)
    check_spans(cases, want, eng.semiglobal_span(jobs), "the arena form after its refusal")
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.zeros(4, np.float32), np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    for k in range(3):  # a null output
        args = [ptr(x) for x in out]
        args[k] = None
        assert eng.lib.rawdtw_semiglobal_span_batch(eng._ctx, ptr(jobs), len(jobs), ptr(ev), len(ev), *args) == INVALID
    assert eng.lib.rawdtw_semiglobal_span_batch(eng._ctx, None, 2, ptr(ev), len(ev), *[ptr(x) for x in out]) == INVALID
    st, cost, j0, end_j = raw_span(eng, jobs[:0], ev[:0])  # no job: RAWDTW_OK, nothing touched
    assert st == 0 and untouched(cost, j0, end_j)
    fresh = ra.Engine(0)  # a context without the arenas it needs
    st, cost, j0, end_j = raw_span(fresh, jobs, ev)
    assert st == INVALID and untouched(cost, j0, end_j)
    z = np.zeros(5, np.float32)
    for n, m in ((0, 5), (5, 0)):
        with pytest.raises(ra.RawDTWError) as e:
            eng.DTW_semiglobal_span(z[:n], z[:m])
        assert e.value.status == INVALID
    check_spans(cases, want, eng.semiglobal_span(jobs, ev), "after the refusals")
    for (a, b, ex), (wc, wj0, wej) in zip(cases, want):  # the drop-in, on the context's own arenas afterwards
        c, s, e = eng.DTW_semiglobal_span(a, b, ex)
        assert (sc.bits(c)[0], s, e) == (sc.bits(wc)[0], wj0, wej)
    check_spans(cases, want, eng.semiglobal_span(jobs, ev), "after the drop-in")


def test_span_between_a_cost_call_and_a_traceback_call():
    """one context: cost, span, traceback, span, cost -- every call's results are what it gives alone; the timing record after a span
    call is the span launches' and nothing else; "tb_sub_batches" keeps what the traceback left"""
    rng = np.random.default_rng(727)
    cases = [(rng.normal(size=n).astype(np.float32), (np.round(rng.normal(size=m) * 2) / 2).astype(np.float32), k & 1)
             for k, (n, m) in enumerate(((400, 3000),) * 6 + ((1100, 900), (60, 200), (1, 50), (513, 64)))]
    alone, jobs, ev = engine_for(cases, tb_workspace_mb=1)
    cost_alone = alone.semiglobal_batch(jobs, ev)
    tb_alone = alone.semiglobal_traceback(jobs, ev)
    eng, jobs, ev = engine_for(cases, tb_workspace_mb=1)
    before = eng.get_option("tb_sub_batches")
    c1 = eng.semiglobal_batch(jobs, ev)
    s1 = eng.semiglobal_span(jobs, ev)
    assert eng.get_option("tb_sub_batches") == before
    t = eng.semiglobal_timing()
    assert t["fill_ms"] > 0 and t["walk_ms"] == 0 and t["direction_bytes"] == 0 and t["path_elements"] == 0
    tb = eng.semiglobal_traceback(jobs, ev)
    subs = eng.get_option("tb_sub_batches")
    assert subs >= 2 and eng.semiglobal_timing()["direction_bytes"] > 0
    s2 = eng.semiglobal_span(jobs, ev)
    assert eng.get_option("tb_sub_batches") == subs
    t = eng.semiglobal_timing()
    assert t["fill_ms"] > 0 and t["walk_ms"] == 0 and t["direction_bytes"] == 0 and t["path_elements"] == 0
    c2 = eng.semiglobal_batch(jobs, ev)
    for x, y in zip(c1 + c2 + tb, cost_alone + cost_alone + tb_alone):
        assert x.tobytes() == y.tobytes()
    for s in (s1, s2):
        check_spans(cases, host_spans(cases), s, "in sequence", tb[1])
        assert s[0].tobytes() == c1[0].tobytes() and s[2].tobytes() == c1[1].tobytes()


def test_placement_on_a_synthetic_reference():
    """64 chunks of 150 events cut from known positions of a two-sequence, two-strand reference, a little noise added: every read's
    target is the strand it was cut from, [j0, end_j] holds the middle of the stretch it was cut from and lies within 8 events of its
    ends, and the whole tuple is the one built from rawdtw_semiglobal_span_host"""
    n = 150
    sref = synth.make_reference([2600, 1900], seed=21)
    eng = ra.Engine(0)
    eng.upload_reference(sref.forward, sref.reverse)
    signals = [sref.forward[0], sref.reverse[0], sref.forward[1], sref.reverse[1]]
    targets = [(eng.reference_offset(q // 2, 1 - (q & 1)), len(sig)) for q, sig in enumerate(signals)]  # (strand 1: forward_signals)
    rng = np.random.default_rng(22)
    truth = [(int(rng.integers(0, 4)), 0) for _ in range(64)]
    truth = [(t, int(rng.integers(0, len(signals[t]) - n + 1))) for t, _ in truth]
    truth[0], truth[1] = (0, 0), (3, len(signals[3]) - n)  # flush against a target's ends
    ev = np.concatenate([signals[t][p:p + n] + rng.normal(0, 0.02, n).astype(np.float32) for t, p in truth]).astype(np.float32)
    reads = [(k * n, n) for k in range(len(truth))]
    eng.upload_events(ev)
    got = eng.semiglobal_place(reads, targets)
    assert got["target"].dtype == np.int32 and all(len(got[key]) == 64 for key in ("target", "cost", "j0", "end_j", "second"))
    for k, (t, p) in enumerate(truth):
        assert got["target"][k] == t and got["j0"][k] <= p + n // 2 <= got["end_j"][k], (k, t, p, got["target"][k], got["j0"][k], got["end_j"][k])
        assert abs(int(got["j0"][k]) - p) <= 8 and abs(int(got["end_j"][k]) - (p + n - 1)) <= 8 and got["cost"][k] < got["second"][k]
    table = [[ra.semiglobal_span_host(ev[k * n:(k + 1) * n], sig) for sig in signals] for k in range(len(truth))]
    want = ra.semiglobal_place_reduce(*[np.array([[cell[q] for cell in row] for row in table]) for q in range(3)])
    for key in ("target", "cost", "j0", "end_j", "second"):
        assert got[key].tobytes() == want[key].tobytes(), key
    got_ex = eng.semiglobal_place(reads[:4], targets, exclude_last=True)
    assert np.array_equal(got_ex["j0"], got["j0"][:4]) and np.array_equal(got_ex["target"], got["target"][:4])
