"""Semiglobal DTW on the device (include/rawdtw.h: rawdtw_semiglobal_batch, rawdtw_semiglobal_traceback_steps, rawdtw_dtw_semiglobal,
rawdtw_dtw_semiglobal_tb; kernels: rawdtw_semiglobal_kernels.hip), bit for bit throughout: costs, end_j, j0, step bytes, distances.

The yardsticks: the answers recorded from the compiled reference (tests/golden/semiglobal_ref.npz) for the value domains, and the
library's host restatement (rawdtw_semiglobal_tb_host: tests/test_semiglobal_cpu.py holds it to the fixture and to the live reference)
for shapes too large for a fixture.  The largest matrix is 1537 x 1000 cells.

DTW_semiglobal itself (its 1e10 sentinel, tests/semiglobal_cases.py) is compared on every case of the domains s9, cross, spike, sub38,
sub41, sub44, zeros and ints that `sentinel_free` admits -- the condition of the arithmetic contract in include/rawdtw.h, decided from
the inputs in numpy -- and each of those domains has at least three such cases; s3e9, s10, s12 and s30 are compared with _slow and
_tb only."""

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd.dtw import JOB_DTYPE
from tests import semiglobal_cases as sc
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


def host_answers(cases):
    return [ra.semiglobal_host(a, b, ex, traceback=True) for a, b, ex in cases]


def check_batch(cases, want, cost, end_j, what):
    for k, ((a, b, ex), (r, ej)) in enumerate(zip(cases, want)):
        assert sc.bits(cost[k])[0] == sc.bits(r.cost)[0] and end_j[k] == ej, (what, k, len(a), len(b), ex, cost[k], r.cost, end_j[k], ej)


def check_paths(cases, want, tb, what):
    cost, j0, off, plen, step, pd = tb
    for k, ((a, b, ex), (r, ej)) in enumerate(zip(cases, want)):
        s = int(off[k])
        assert sc.bits(cost[k])[0] == sc.bits(r.cost)[0] and plen[k] == len(r.i), (what, k, len(a), len(b), ex)
        if len(r.i) == 0:
            continue
        assert j0[k] == r.j[0] and step[s] == 0, (what, k)
        i, j = ra.expand_steps(step[s:s + int(plen[k])], int(j0[k]))
        assert np.array_equal(i, r.i) and np.array_equal(j, r.j), (what, k, len(a), len(b), ex)
        assert np.array_equal(sc.bits(pd[s:s + int(plen[k])]), sc.bits(r.difference)), (what, k)


@pytest.fixture(scope="module")
def sweep():
    """n at every class and strip edge x m around the 64-column chunk, n > m, n == 1; normal and integer-valued signals (ties in the
    walk's rule and in the last row); exclude_last 0 and 1"""
    rng = np.random.default_rng(515)
    shapes = [(n, m) for n in sc.SWEEP_N for m in sc.SWEEP_M] + list(sc.TALL)
    cases = []
    for q, (n, m) in enumerate(shapes):
        cases.append((rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32), q & 1))
        cases.append((rng.integers(-2, 3, n).astype(np.float32), rng.integers(-2, 3, m).astype(np.float32), 1 - (q & 1)))
    return cases, host_answers(cases)


def test_sweep_costs_and_end_columns(sweep):
    cases, want = sweep
    eng, jobs, ev = engine_for(cases)
    cost, end_j = eng.semiglobal_batch(jobs, ev)
    check_batch(cases, want, cost, end_j, "sweep")
    for (a, b, ex), c in zip(cases, cost):  # n == 1: the smallest |a0 - b_j|, less itself when the last element is excluded
        if len(a) == 1:
            d = np.abs(a[0] - b).astype(np.float32)
            assert sc.bits(c)[0] == sc.bits(np.float32(0.0) if ex else d.min())[0]


def test_sweep_paths(sweep):
    cases, want = sweep
    eng, jobs, ev = engine_for(cases)
    tb = eng.semiglobal_traceback(jobs, ev)
    check_paths(cases, want, tb, "sweep")
    assert eng.get_option("tb_sub_batches") == 1
    for (a, b, ex), (r, ej) in zip(cases, want):
        if len(a) == 1:
            assert len(r.i) == 1 - ex
        if len(b) == 1 and not ex:
            assert np.array_equal(r.j, np.zeros(len(a), np.uint32))  # a run along j == 0


def test_planted_end_columns():
    """the minimum of the last row planted at end_j = 0, 63, 64, 65 and m - 1 (and the like further right for taller jobs), and two
    equal minima: the first wins"""
    cases, ends = [], []
    for n, m, ats in ((20, 130, (0, 63, 64, 65, 129)), (130, 700, (0, 191, 192, 193, 699)), (600, 900, (0, 639, 640, 641, 899))):
        for at in ats:
            a, b = sc.planted(n, m, (at,))
            cases.append((a, b, at & 1))
            ends.append(at)
    for n, m, ats in ((20, 130, (40, 100)), (20, 200, (63, 128)), (130, 700, (200, 650)), (600, 1300, (620, 1299))):
        a, b = sc.planted(n, m, ats)
        cases.append((a, b, 0))
        ends.append(ats[0])
    want = host_answers(cases)
    assert [ej for _, ej in want] == ends  # (the construction did what it says)
    eng, jobs, ev = engine_for(cases)
    check_batch(cases, want, *eng.semiglobal_batch(jobs, ev), "planted")
    check_paths(cases, want, eng.semiglobal_traceback(jobs, ev), "planted")


def test_value_domains_against_the_recorded_reference():
    fx = sc.Fixture()
    cases = [fx.inputs(k) + (ex,) for k in range(len(fx)) for ex in (0, 1)]
    eng, jobs, ev = engine_for(cases)
    cost, end_j = eng.semiglobal_batch(jobs, ev)
    tcost, j0, off, plen, step, pd = eng.semiglobal_traceback(jobs, ev)
    free = {}
    for q, (a, b, ex) in enumerate(cases):
        k = q // 2
        what = (fx.tag(k), k, len(a), len(b), ex)
        assert sc.bits(cost[q])[0] == sc.bits(tcost[q])[0] == fx.z["slow"][k, ex] == fx.z["tb_cost"][k, ex], what
        assert end_j[q] == fx.z["end_j"][k], what
        wi, wj, wd = fx.path(k, ex)
        s, ln = int(off[q]), int(plen[q])
        assert ln == len(wi), what
        if ln:
            i, j = ra.expand_steps(step[s:s + ln], int(j0[q]))
            assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(sc.bits(pd[s:s + ln]), sc.bits(wd)), what
        if ex == 0 and fx.tag(k) not in vc.SENTINEL_DOMAINS and sc.sentinel_free(a, b):
            # DTW_semiglobal itself: the batch's cost, and the drop-in (which ignores the flag, as its namesake does)
            assert sc.bits(cost[q])[0] == fx.z["fast"][k, 0], what
            if free.get(fx.tag(k), 0) < 3:
                assert sc.bits(eng.DTW_semiglobal(a, b, True).cost)[0] == fx.z["fast"][k, 1], what
            free[fx.tag(k)] = free.get(fx.tag(k), 0) + 1
    assert all(free.get(d, 0) >= 3 for d in sc.ALL_THREE), free


def test_value_domains_at_larger_shapes():
    """every domain past one strip and on the pipelined form, against the host restatement; sums stay finite even at 1e30"""
    cases = []
    for name in vc.DOMAIN_NAMES:
        rng = vc.domain_rng(name, salt=43)
        for n, m in ((513, 600), (1025, 200), (257, 65)):
            a, b = vc.DOMAINS[name](rng, n), vc.DOMAINS[name](rng, m)
            assert n + m <= 2600 and vc.sums_stay_finite((a, b), n, m)
            cases.append((a, b, len(cases) & 1))
    want = host_answers(cases)
    eng, jobs, ev = engine_for(cases)
    check_batch(cases, want, *eng.semiglobal_batch(jobs, ev), "domains")
    check_paths(cases, want, eng.semiglobal_traceback(jobs, ev), "domains")


def test_batch_of_mixed_classes_over_the_arenas():
    """2 000 jobs of every class over shared arenas, windows flush against both ends of both arenas; the h_events form and the arena form"""
    rng = np.random.default_rng(616)
    ev = rng.normal(size=6000).astype(np.float32)
    rf = (np.round(rng.normal(size=9000) * 2) / 2).astype(np.float32)
    eng = ra.Engine(0)
    eng.upload_reference([rf], [rf])
    base = eng.reference_offset(0, 1)
    jobs = np.zeros(2000, JOB_DTYPE)
    tops = (64, 128, 256, 700, 1300)
    for k in range(len(jobs)):
        c = k % 5 if k % 40 else 4
        n = int(rng.integers(1 if c == 0 else tops[c - 1] + 1, tops[c] + 1))
        m = int(rng.integers(1, 40 if c == 4 else 300))
        jobs[k] = (base + int(rng.integers(0, len(rf) - m + 1)), int(rng.integers(0, len(ev) - n + 1)), n, m, -1, k & 1, 0)
    jobs[0]["read_off"], jobs[0]["ref_off"] = 0, base
    jobs[1]["read_off"], jobs[1]["ref_off"] = len(ev) - int(jobs[1]["n"]), base + len(rf) - int(jobs[1]["m"])
    jobs[7]["read_off"], jobs[7]["ref_off"] = len(ev) - int(jobs[7]["n"]), base
    assert len(set(np.searchsorted(tops, jobs["n"]))) == 5 and (jobs["n"] > 1024).sum() >= 40
    cases = [(ev[j["read_off"]:j["read_off"] + j["n"]], rf[int(j["ref_off"]) - base:int(j["ref_off"]) - base + j["m"]], int(j["exclude_last"])) for j in jobs]
    want = host_answers(cases)
    check_batch(cases, want, *eng.semiglobal_batch(jobs, ev), "h_events form")
    eng2 = ra.Engine(0)
    eng2.upload_reference([rf], [rf])
    eng2.upload_events(ev)
    check_batch(cases, want, *eng2.semiglobal_batch(jobs), "arena form")
    check_batch(cases, want, *eng2.semiglobal_batch(jobs), "arena form, again")
    sub = np.arange(0, 2000, 9)
    check_paths([cases[k] for k in sub], [want[k] for k in sub], eng2.semiglobal_traceback(jobs[sub]), "arena form, paths")


def test_traceback_in_sub_batches():
    """forty 400 x 3 000 jobs under a 1 MiB direction budget: several sub-batches; the same paths as in one, and the host's"""
    rng = np.random.default_rng(717)
    cases = [(rng.normal(size=400).astype(np.float32), (np.round(rng.normal(size=3000) * 2) / 2).astype(np.float32), k & 1) for k in range(40)]
    want = host_answers(cases)
    small, jobs, ev = engine_for(cases, tb_workspace_mb=1)
    one, jobs1, _ = engine_for(cases)
    tb_small = small.semiglobal_traceback(jobs, ev)
    tb_one = one.semiglobal_traceback(jobs1, ev)
    assert small.get_option("tb_sub_batches") >= 10 and one.get_option("tb_sub_batches") == 1
    for x, y in zip(tb_small, tb_one):
        assert x.tobytes() == y.tobytes()
    check_paths(cases, want, tb_small, "sub-batches")
    t = small.semiglobal_timing()
    assert t["path_elements"] == int(tb_small[3].sum()) and t["direction_bytes"] > 40 * 400 * 3000 // 4


def test_refusals_leave_the_context_usable():
    rng = np.random.default_rng(818)
    cases = [(rng.normal(size=30).astype(np.float32), rng.normal(size=50).astype(np.float32), 0),
             (rng.normal(size=70).astype(np.float32), rng.normal(size=20).astype(np.float32), 1)]
    want = host_answers(cases)
    eng, jobs, ev = engine_for(cases)

    def refused(status, **change):
        bad = jobs.copy()
        for name, value in change.items():
            bad[name][1] = value
        for call in (eng.semiglobal_batch, eng.semiglobal_traceback):
            with pytest.raises(ra.RawDTWError) as e:
                call(bad, ev)
            assert e.value.status == status, (change, e.value)
        check_batch(cases, want, *eng.semiglobal_batch(jobs, ev), "after %r" % (change,))  # a good call on the same context

    refused(INVALID, n=0)
    refused(INVALID, m=0)
    refused(INVALID, band_radius=0)
    refused(INVALID, band_radius=5)
    refused(RANGE, read_off=len(ev) - 69)
    refused(RANGE, ref_off=2 ** 33)
    refused(RANGE, ref_off=2 ** 40)
    eng.upload_events(ev)  # the arena form reads the arena as it lies: 100 events there, the window would end at 101
    bad = jobs.copy()
    bad["read_off"][1] = 31
    with pytest.raises(ra.RawDTWError) as e:
        eng.semiglobal_batch(bad)
    assert e.value.status == RANGE
    check_batch(cases, want, *eng.semiglobal_batch(jobs), "the arena form after its refusal")
    for call in (eng.semiglobal_batch, eng.semiglobal_traceback):  # no job: RAWDTW_OK, nothing touched
        out = call(jobs[:0], ev[:0])
        assert len(out[0]) == 0
    for n, m in ((0, 5), (5, 0)):
        z = np.zeros(5, np.float32)
        for call in (eng.DTW_semiglobal, eng.DTW_semiglobal_tb):
            with pytest.raises(ra.RawDTWError) as e:
                call(z[:n], z[:m])
            assert e.value.status == INVALID
    check_paths(cases, want, eng.semiglobal_traceback(jobs, ev), "after the refusals")


def test_steps_and_j0_expand_to_the_drop_in_s_path():
    rng = np.random.default_rng(919)
    cases = [(rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32), ex)
             for n, m, ex in ((90, 400, 0), (90, 400, 1), (300, 5, 0), (1, 9, 0), (1, 9, 1), (1100, 300, 1), (257, 129, 0))]
    eng, jobs, ev = engine_for(cases)
    cost, j0, off, plen, step, pd = eng.semiglobal_traceback(jobs, ev)
    for k, (a, b, ex) in enumerate(cases):
        r = eng.DTW_semiglobal_tb(a, b, ex)
        s, ln = int(off[k]), int(plen[k])
        i, j = ra.expand_steps(step[s:s + ln], int(j0[k]))
        assert sc.bits(r.cost)[0] == sc.bits(cost[k])[0] and len(r) == ln
        assert np.array_equal(r.i, i) and np.array_equal(r.j, j) and np.array_equal(sc.bits(r.difference), sc.bits(pd[s:s + ln]))
        if ln:
            assert r.i[0] == 0 and (ex or r.i[-1] == len(a) - 1) and len(r) <= len(a) + len(b) - 1
