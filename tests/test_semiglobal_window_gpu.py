"""The semiglobal traceback in windows on the device (include/rawdtw.h, "semiglobal, in windows": rawdtw_set_semiglobal_window; kernels
k_semi_ckpt_wave and k_semi_window in rawdtw_semiglobal_kernels.hip).

The yardstick is the n x m form on the SAME context with the setter off (tests/test_semiglobal_gpu.py holds that one to the recorded
reference and to the host restatement): cost bits, j0, path_len, step bytes and distances, byte for byte; on the fixture's cases also the
reference's recorded paths.  Window counts, direction bytes and sub-batch counts are derived here from n, m, C and the class
(tests/semiglobal_window_cases.py), the windows from the setter-off paths.  The largest matrix is 1537 x 1000 cells."""
import ctypes as C

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from rawalign_amd import mapper
from rawalign_amd.mapping import StopOpt
from tests import map_ref_cases as mc
from tests import semiglobal_cases as sc
from tests import semiglobal_window_cases as wc
from tests import value_cases as vc
from tests.util import make_arena_jobs

pytestmark = pytest.mark.gpu
INVALID, RANGE = 1, 4
WINDOW_M = (1, 63, 64, 65, 129, 200, 1000)


def engine_for(cases, **options):
    """-> (engine, jobs, events): every b in the engine's reference arena, every a in `events`, FULL jobs over them"""
    jobs, ev, rf = make_arena_jobs([(a, b, -1, ex) for a, b, ex in cases])
    eng = ra.Engine(0)
    for name, value in options.items():
        eng.set_option(name, value)
    eng.upload_reference([rf], [rf])
    jobs["ref_off"] += eng.reference_offset(0, 1)
    return eng, jobs, ev


def off_and_on(eng, jobs, ev, cols):
    """the same call with the setter off and on, on one context -> (off, on, the on call's timing, its window stats)"""
    eng.set_semiglobal_window(0)
    off = eng.semiglobal_traceback(jobs, ev)
    assert eng.semiglobal_window_stats() == dict(jobs_windowed=0, windows=0, max_windows_a_job=0, checkpoint_bytes=0)
    eng.set_semiglobal_window(cols)
    assert eng.get_semiglobal_window() == cols
    on = eng.semiglobal_traceback(jobs, ev)
    return off, on, eng.semiglobal_timing(), eng.semiglobal_window_stats()


def identical(off, on, what):
    for name, x, y in zip(("cost", "j0", "path_off", "path_len", "step", "distance"), off, on):
        assert x.tobytes() == y.tobytes(), (what, name, np.flatnonzero(x.view(np.uint8).reshape(-1) != y.view(np.uint8).reshape(-1))[:4])


def model_counts(cases, off, cols):
    """windows a job from the setter-off path (the full path: with exclude_last the end cell is put back), and the layout's bytes"""
    cost, j0, poff, plen, step, pd = off
    windows = []
    for k, (a, b, ex) in enumerate(cases):
        s, ln = int(poff[k]), int(plen[k])
        i, j = ra.expand_steps(step[s:s + ln], int(j0[k]))
        if ex:
            end_j = ra.semiglobal_host(a, b)[1]
            i, j = np.append(i, len(a) - 1), np.append(j, end_j)
        windows.append(wc.windows_of(i, j, len(b), cols))
    w = [wc.windowed(len(b), cols) for _, b, _ in cases]
    return dict(jobs_windowed=sum(w), windows=sum(windows), max_windows_a_job=max(windows, default=0),
                checkpoint_bytes=sum(wc.ckpt_bytes(len(a), len(b), cols) for (a, b, _), x in zip(cases, w) if x)), \
        sum(wc.workspace_bytes(len(a), len(b), cols) for a, b, _ in cases)


def check(cases, cols, what, **options):
    eng, jobs, ev = engine_for(cases, **options)
    off, on, timing, stats = off_and_on(eng, jobs, ev, cols)
    identical(off, on, what)
    want_stats, want_bytes = model_counts(cases, off, cols)
    assert stats == want_stats, (what, stats, want_stats)
    assert timing["direction_bytes"] == want_bytes and timing["path_elements"] == int(on[3].sum()), (what, timing, want_bytes)
    # bar (a): what is not checkpoints is one window of n x C directions a windowed job, by the layout formula
    assert timing["direction_bytes"] - stats["checkpoint_bytes"] == sum(
        wc.al256(wc.semi_dir_bytes(len(a), min(cols, len(b)))) if wc.windowed(len(b), cols) else wc.al256(wc.semi_dir_bytes(len(a), len(b))) for a, b, _ in cases)
    return eng, jobs, ev, off, on


@pytest.fixture(scope="module")
def sweep():
    """n at every class and strip edge (1 025 and 1 537 rows: three and four strips) x m around the window and the 64-column chunk;
    normal and integer-valued signals (ties in the walk's rule); exclude_last 0 and 1"""
    rng = np.random.default_rng(2525)
    cases = []
    for q, (n, m) in enumerate([(n, m) for n in sc.SWEEP_N for m in WINDOW_M] + list(sc.TALL)):
        cases.append((rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32), q & 1))
        cases.append((rng.integers(-2, 3, n).astype(np.float32), rng.integers(-2, 3, m).astype(np.float32), 1 - (q & 1)))
    return cases


def test_sweep_at_64_columns(sweep):
    eng, jobs, ev, off, on = check(sweep, 64, "sweep")
    assert eng.get_option("tb_sub_batches") == 1
    t = eng.semiglobal_timing()
    assert t["fill_ms"] > 0 and t["walk_ms"] > 0


def test_128_columns_with_mixed_classes_in_one_call(sweep):
    cases = sweep[::3]
    assert len({wc.rpl_of(len(a)) for a, _, _ in cases}) == 4 and sum(len(a) > 1024 for a, _, _ in cases) >= 4
    assert {len(b) <= 128 for _, b, _ in cases} == {True, False}   # windowed jobs and others in one call
    check(cases, 128, "mixed at 128")
    check(cases, 128, "mixed at 128, one wave a job", full_wg=0)


def test_planted_multi_window_paths_and_the_window_s_own_width():
    cases = [(a, b, k & 1) for k, (_, a, b) in enumerate(wc.planted_cases())]   # (m == C and m == C + 1 among them)
    eng, jobs, ev, off, on = check(cases, 64, "planted")
    for sig_n, m, at in ((257, 400, 63), (257, 400, 64), (600, 900, 640), (600, 900, 0), (1100, 700, 699)):
        a, b = sc.planted(sig_n, m, (at,))
        cases.append((a, b, at & 1))
    check(cases, 64, "planted, taller")
    check(cases, 256, "planted, 256 columns")


def test_value_domains_and_the_recorded_reference():
    fx = sc.Fixture()
    cases = [fx.inputs(k) + (ex,) for k in range(len(fx)) for ex in (0, 1)]
    n_fx = len(cases)
    for name in vc.DOMAIN_NAMES:
        rng = vc.domain_rng(name, salt=53)
        for n, m in ((513, 600), (1025, 200), (257, 65), (70, 300)):
            a, b = vc.DOMAINS[name](rng, n), vc.DOMAINS[name](rng, m)
            assert vc.sums_stay_finite((a, b), n, m)
            cases.append((a, b, len(cases) & 1))
    eng, jobs, ev, off, on = check(cases, 64, "domains")
    cost, j0, poff, plen, step, pd = on
    for q in range(n_fx):
        k, ex = q // 2, q & 1
        wi, wj, wd = fx.path(k, ex)
        s, ln = int(poff[q]), int(plen[q])
        what = (fx.tag(k), k, ex)
        assert sc.bits(cost[q])[0] == fx.z["tb_cost"][k, ex] and ln == len(wi), what
        if ln:
            i, j = ra.expand_steps(step[s:s + ln], int(j0[q]))
            assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(sc.bits(pd[s:s + ln]), sc.bits(wd)), what


def test_arena_form_and_the_drop_in():
    rng = np.random.default_rng(626)
    cases = [(rng.normal(size=n).astype(np.float32), (np.round(rng.normal(size=m) * 2) / 2).astype(np.float32), ex)
             for n, m, ex in ((90, 400, 0), (90, 400, 1), (300, 5, 0), (1, 90, 0), (1, 90, 1), (1100, 300, 1), (257, 129, 0), (40, 64, 1), (40, 65, 0))]
    eng, jobs, ev = engine_for(cases)
    eng.upload_events(ev)
    off, on, _, stats = off_and_on(eng, jobs, None, 64)   # h_events == NULL
    identical(off, on, "arena form")
    assert stats["jobs_windowed"] == sum(len(b) > 64 for _, b, _ in cases)
    cost, j0, poff, plen, step, pd = on
    for k, (a, b, ex) in enumerate(cases):
        eng.set_semiglobal_window(64)
        r = eng.DTW_semiglobal_tb(a, b, ex)
        want_windows = eng.semiglobal_window_stats()
        eng.set_semiglobal_window(0)
        w = eng.DTW_semiglobal_tb(a, b, ex)
        s, ln = int(poff[k]), int(plen[k])
        i, j = ra.expand_steps(step[s:s + ln], int(j0[k]))
        assert sc.bits(r.cost)[0] == sc.bits(w.cost)[0] == sc.bits(cost[k])[0] and len(r) == len(w) == ln, k
        assert np.array_equal(r.i, w.i) and np.array_equal(r.j, w.j) and np.array_equal(sc.bits(r.difference), sc.bits(w.difference)), k
        assert np.array_equal(r.i, i) and np.array_equal(r.j, j), k
        assert want_windows["jobs_windowed"] == int(len(b) > 64) and (want_windows["windows"] > 0) == (len(b) > 64 and len(a) > 1), k


def test_refusals_are_unchanged_with_the_setter_on():
    rng = np.random.default_rng(828)
    cases = [(rng.normal(size=30).astype(np.float32), rng.normal(size=150).astype(np.float32), 0),
             (rng.normal(size=70).astype(np.float32), rng.normal(size=220).astype(np.float32), 1)]
    eng, jobs, ev = engine_for(cases)
    good_off, good_on, _, _ = off_and_on(eng, jobs, ev, 64)
    identical(good_off, good_on, "before the refusals")
    ptr = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731

    def refused(status, **change):
        bad = jobs.copy()
        for name, value in change.items():
            bad[name][1] = value
        got = []
        for cols in (0, 64):
            eng.set_semiglobal_window(cols)
            out = [np.full(2, 7, np.float32), np.full(2, 7, np.uint32), np.zeros(3, np.uint64), np.full(2, 7, np.uint32), np.full(700, 7, np.uint8), np.full(700, 7, np.float32)]
            out[2][1:] = np.cumsum([30 + 150 - 1, 70 + 220 - 1])
            st = eng.lib.rawdtw_semiglobal_traceback_steps(eng._ctx, ptr(bad), len(bad), ptr(ev), len(ev), *[ptr(x) for x in out])
            assert st == status, (change, cols, st)
            for x in (out[0], out[1], out[3], out[4], out[5]):
                assert (x == 7).all(), (change, cols)   # the out arrays are untouched
            got.append(eng.lib.rawdtw_last_error(eng._ctx))
        assert got[0] == got[1], change                 # ... and the message is the same
        eng.set_semiglobal_window(64)
        identical(good_off, eng.semiglobal_traceback(jobs, ev), "after %r" % (change,))

    refused(INVALID, band_radius=5)
    refused(INVALID, n=0)
    refused(INVALID, m=0)
    refused(RANGE, read_off=len(ev) - 69)
    refused(RANGE, ref_off=2 ** 40)


def test_invalid_setter_values_are_refused_and_nothing_is_stored():
    eng = ra.Engine(0)
    assert eng.get_semiglobal_window() == 0
    eng.set_semiglobal_window(512)
    for bad in (1, 32, 63, 65, 100, 4097, (1 << 20) + 64, 1 << 21, (1 << 32) - 64):
        with pytest.raises(ra.RawDTWError) as e:
            eng.set_semiglobal_window(bad)
        assert e.value.status == INVALID and eng.get_semiglobal_window() == 512, bad
    for good in (64, 128, 4096, 1 << 20, 0):
        eng.set_semiglobal_window(good)
        assert eng.get_semiglobal_window() == good


def test_sub_batches():
    """eight 257 x 4 096 jobs under a 1 MiB budget: eight sub-batches as n x m directions, one in windows of 64 columns -- both from
    the split's formula --, and the same paths"""
    rng = np.random.default_rng(929)
    cases = [(rng.normal(size=257).astype(np.float32), (np.round(rng.normal(size=4096) * 2) / 2).astype(np.float32), k & 1) for k in range(8)]
    mib = 1 << 20
    want_off = wc.split([wc.job_bytes(257, 4096, 0)] * 8, mib)
    want_on = wc.split([wc.job_bytes(257, 4096, 64)] * 8, mib)
    assert len(want_off) > 1 and len(want_on) == 1
    eng, jobs, ev = engine_for(cases, tb_workspace_mb=1)
    eng.set_semiglobal_window(0)
    off = eng.semiglobal_traceback(jobs, ev)
    assert eng.get_option("tb_sub_batches") == len(want_off)
    eng.set_semiglobal_window(64)
    on = eng.semiglobal_traceback(jobs, ev)
    assert eng.get_option("tb_sub_batches") == 1
    identical(off, on, "sub-batches")
    want_stats, want_bytes = model_counts(cases, off, 64)
    assert eng.semiglobal_window_stats() == want_stats and eng.semiglobal_timing()["direction_bytes"] == want_bytes == 8 * wc.job_bytes(257, 4096, 64)
    # ... and windowed jobs in several sub-batches: twenty of them, twelve fit the budget
    cases = cases + cases + cases[:4]
    eng, jobs, ev = engine_for(cases, tb_workspace_mb=1)
    off, on, timing, stats = off_and_on(eng, jobs, ev, 64)
    assert eng.get_option("tb_sub_batches") == len(wc.split([wc.job_bytes(257, 4096, 64)] * 20, mib)) == 2
    identical(off, on, "windowed sub-batches")
    assert stats == model_counts(cases, off, 64)[0]


def test_local_border_mapper_cigar_lines():
    """a local-border --dtw-output-cigar mapper, one read group: the lines with the setter on the context are the lines with it off"""
    ref = mc.make_reference()
    wr = mc.WholeReads(0, ref=ref)
    lines = {}
    for cols in (0, 64):
        e = ra.Engine(0)
        e.upload_reference(ref.forward, ref.reverse)
        e.set_border_local(True)
        e.set_semiglobal_window(cols)
        opt, copt = mc.whole_project_opts("cigar", 0)
        opt.dtw_border_constraint = 2
        cm = mapper.CMapper(e, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096, max_reads=wr.n_reads,
                            chain_opt=copt, output_chains=True, threads=3, carry=False, groups=1)
        lines[cols] = mapper.map_reads_c(wr, list(range(wr.n_reads)), cm)
        windowed = e.semiglobal_window_stats()["jobs_windowed"]
        cm.close()
        e.close()
        assert (windowed > 0) == (cols > 0), (cols, windowed)   # the finish's chains are wider than 64 columns: it did go through windows
    assert lines[0] == lines[64] and sum("\taln:s:(" in ln for ln in lines[64][0]) >= 3


def test_place_with_paths():
    """8 reads x 4 targets: the winners' (cost, j0, end_j) from the span are the traceback's cost, first and last column, bit for bit,
    with the window off and on; paths=False is today's dict"""
    rng = np.random.default_rng(1030)
    signals = [(np.round(rng.normal(size=m) * 4) / 4).astype(np.float32) for m in (700, 900, 640, 1000)]
    truth = [(k % 4, int(rng.integers(0, len(signals[k % 4]) - 130))) for k in range(8)]
    n = 120
    ev = np.concatenate([signals[t][s:s + n] + 0.05 * rng.normal(size=n).astype(np.float32) for t, s in truth]).astype(np.float32)
    eng = ra.Engine(0)
    eng.upload_reference(signals, signals)
    eng.upload_events(ev)
    reads = [(k * n, n) for k in range(8)]
    targets = [(eng.reference_offset(s, 1), len(signals[s])) for s in range(4)]
    plain = eng.semiglobal_place(reads, targets)
    again = eng.semiglobal_place(reads, targets, paths=False)
    assert sorted(plain) == sorted(again) == ["cost", "end_j", "j0", "second", "target"]
    assert all(plain[k].tobytes() == again[k].tobytes() for k in plain)
    assert [int(t) for t in plain["target"]] == [t for t, _ in truth]
    got = {}
    for cols in (0, 64):
        eng.set_semiglobal_window(cols)
        p = got[cols] = eng.semiglobal_place(reads, targets, paths=True)
        assert all(p[k].tobytes() == plain[k].tobytes() for k in plain)
        for r in range(8):
            s, ln = int(p["path_off"][r]), int(p["path_len"][r])
            i, j = ra.expand_steps(p["step"][s:s + ln], int(p["tb_j0"][r]))
            assert sc.bits(p["tb_cost"][r])[0] == sc.bits(p["cost"][r])[0] and j[0] == p["j0"][r] and j[-1] == p["end_j"][r], (cols, r)
            assert i[0] == 0 and i[-1] == n - 1
        assert (eng.semiglobal_window_stats()["jobs_windowed"] == 8) == (cols == 64)
    for key in ("path_off", "path_len", "step", "distance", "tb_cost", "tb_j0"):
        assert got[0][key].tobytes() == got[64][key].tobytes(), key
