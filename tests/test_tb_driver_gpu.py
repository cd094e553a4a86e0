"""The one traceback driver (rawalign_amd/csrc/rawdtw_tb_driver.cpp) on the device: slot reuse on the banded and the semiglobal path,
which ran one sub-batch at a time before it; one context through all three paths and the text form, whose grow-only buffers they now
share; and refusals.  Bit for bit throughout.  Expected values come from the library's host restatements (rawdtw_banded_tb_host,
rawdtw_semiglobal_tb_host) and the oracle; the lists and the CPU models of the split are tests/tb_driver_cases.py's.

The four routes of the full-matrix path at 1 MiB over the `pipe` list (dense and direct, dense through the landing zone, steps at
offsets with gaps, (i, j)) are tests/test_traceback_pipeline_gpu.py's: test_pipe_steps_form_in_every_layout and
test_pipe_in_thirteen_sub_batches_equals_oracle_and_the_unsplit_call."""
import ctypes as C

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from rawalign_amd.dtw import ALN_REC_DTYPE
from tests import tb_driver_cases as dc
from tests import traceback_cases as tc
from tests.util import make_arena_jobs

pytestmark = pytest.mark.gpu
INVALID, RANGE = 1, 4
CANARY = 0xEE
PATHS = ("full", "banded", "semiglobal")


def vp(x):
    return C.c_void_p(x.ctypes.data)


def bits(x):
    return np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32)


def canaries(n, dtype):
    a = np.empty(max(n, 1), dtype)
    a.view(np.uint8)[:] = CANARY
    return a


def untouched(*arrays):
    return all(np.all(a.view(np.uint8) == CANARY) for a in arrays)


def timings(eng):
    """{path: (fill_ms, walk_ms, direction_bytes, path_elements)} of the three getters"""
    out = {}
    for path, fn in zip(PATHS, (eng.lib.rawdtw_traceback_timing, eng.lib.rawdtw_banded_traceback_timing, eng.lib.rawdtw_semiglobal_timing)):
        f, w, d, e = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
        assert fn(eng._ctx, C.byref(f), C.byref(w), C.byref(d), C.byref(e)) == 0
        out[path] = (f.value, w.value, d.value, e.value)
    return out


def engine_for(cases, **options):
    """cases: [(a, b, R, exclude_last)] -> (engine, jobs, events): every b in the engine's reference arena, every a in `events`"""
    jobs, ev, rf = make_arena_jobs(cases)
    eng = ra.Engine(0)
    for name, value in options.items():
        eng.set_option(name, value)
    eng.upload_reference([rf], [rf])
    jobs["ref_off"] += eng.reference_offset(0, 1)
    return eng, jobs, ev


def steps_call(eng, path, jobs, ev, gap=0, page_locked=False):
    """one steps-form call of `path` into arrays of canaries, job k's room `gap` elements behind job k - 1's -> (status, arrays): cost,
    path_len, step, distance and, semiglobal, j0; the offsets"""
    caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
    off = np.zeros(len(jobs) + 1, np.uint64)
    np.cumsum(caps + np.uint64(gap), out=off[1:])
    total = int(off[-1]) + 8
    cost, plen, j0 = canaries(len(jobs), np.float32), canaries(len(jobs), np.uint32), canaries(len(jobs), np.uint32)
    if page_locked:
        ptrs = [C.c_void_p(), C.c_void_p()]
        assert eng.lib.rawdtw_host_alloc(total, C.byref(ptrs[0])) == 0 and eng.lib.rawdtw_host_alloc(4 * total, C.byref(ptrs[1])) == 0
        step = np.frombuffer((C.c_char * total).from_address(ptrs[0].value), np.uint8, total)
        dist = np.frombuffer((C.c_char * (4 * total)).from_address(ptrs[1].value), np.float32, total)
        step[:] = CANARY
        dist.view(np.uint8)[:] = CANARY
    else:
        step, dist = canaries(total, np.uint8), canaries(total, np.float32)
    head = (eng._ctx, vp(jobs), len(jobs), vp(ev), len(ev), vp(cost))
    tail = (vp(off), vp(plen), vp(step), vp(dist))
    if path == "full":
        st = eng.lib.rawdtw_traceback_batch_steps(*head, *tail)
    elif path == "banded":
        st = eng.lib.rawdtw_banded_traceback_steps(*head, *tail)
    else:
        st = eng.lib.rawdtw_semiglobal_traceback_steps(*head, vp(j0), *tail)
    out = [cost, plen, step.copy(), dist.copy()] + ([j0] if path == "semiglobal" else [])
    if page_locked:
        del step, dist
        for p in ptrs:
            eng.lib.rawdtw_host_free(p)
    return st, out, off


def check_paths(what, cases, want, out, off):
    """want: [(cost, i, j, difference)], exclude_last's pop included; the cells behind every path keep their canaries"""
    cost, plen, step, dist = out[:4]
    for k, (c, wi, wj, wd) in enumerate(want):
        s, ln, e = int(off[k]), int(plen[k]), int(off[k + 1])
        key = (what, k, len(cases[k][0]), len(cases[k][1]))
        assert bits(cost[k])[0] == bits(c)[0] and ln == len(wi), key + (cost[k], c, ln, len(wi))
        assert np.all(step[s + ln:e] == CANARY) and untouched(dist[s + ln:e]), key
        if ln == 0:
            continue
        j0 = int(out[4][k]) if len(out) > 4 else 0
        assert step[s] == 0 and j0 == wj[0], key
        i, j = ra.expand_steps(step[s:s + ln], j0)
        assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(bits(dist[s:s + ln]), bits(wd)), key
    assert np.all(step[int(off[-1]):] == CANARY) and untouched(dist[int(off[-1]):]), what


@pytest.fixture(scope="module")
def banded():
    cases = dc.banded_cases()
    want = []
    for a, b, R, ex in cases:
        r = ra.banded_tb_host(a, b, R, ex)
        want.append((r.cost, r.i, r.j, r.difference))
    return cases, want


@pytest.fixture(scope="module")
def semiglobal():
    cases = [(a, b, -1, ex) for a, b, ex in dc.semiglobal_cases()]
    want = []
    for a, b, _, ex in cases:
        r, _ = ra.semiglobal_host(a, b, ex, traceback=True)
        want.append((r.cost, r.i, r.j, r.difference))
    return cases, want


def slot_reuse(path, cases, want, split, job_bytes, drop_in):
    """the list at 1 MiB and unsplit: the host's answers, identical arrays, the split and the timing getters as modelled"""
    small, jobs, ev = engine_for(cases, tb_workspace_mb=dc.BUDGET_MB)
    one, jobs1, _ = engine_for(cases)
    before = timings(small)
    st, got, off = steps_call(small, path, jobs, ev, gap=3)
    assert st == 0 and small.get_option("tb_sub_batches") == len(split) >= 5
    check_paths(path + " at 1 MiB", cases, want, got, off)
    st, whole, off1 = steps_call(one, path, jobs1, ev, gap=3)
    assert st == 0 and one.get_option("tb_sub_batches") == 1 and np.array_equal(off, off1)
    for x, y in zip(got, whole):
        assert x.tobytes() == y.tobytes()
    after = timings(small)
    for other in PATHS:
        if other != path:
            assert after[other] == before[other] == (0.0, 0.0, 0, 0), other
    fill_ms, walk_ms, dir_bytes, elems = after[path]
    assert fill_ms > 0 and walk_ms > 0 and dir_bytes == sum(job_bytes) and elems == int(got[1].sum()) == sum(len(w[1]) for w in want)
    assert timings(one)[path][2:] == (dir_bytes, elems)
    # the (i, j) drop-ins on the context with the lowered budget: a job a call, the job over the budget among them
    for k in (0, 1, dc.NO_PATH_AT, dc.BIG_AT, len(cases) - 1):
        a, b, R, ex = cases[k]
        r = drop_in(small, a, b, R, ex)
        c, wi, wj, wd = want[k]
        assert small.get_option("tb_sub_batches") == 1
        assert bits(r.cost)[0] == bits(c)[0] and np.array_equal(r.i, wi) and np.array_equal(r.j, wj) and np.array_equal(bits(r.difference), bits(wd)), (path, k)
    st, again, _ = steps_call(small, path, jobs, ev, gap=3)   # ... and the split call once more behind them
    assert st == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(again, got))
    small.close()
    one.close()


def test_banded_slot_reuse(banded):
    cases, want = banded
    assert len(want[dc.NO_PATH_AT][1]) == 0 and all(len(w[1]) for k, w in enumerate(want) if k != dc.NO_PATH_AT)
    slot_reuse("banded", cases, want, dc.banded_split(cases), dc.banded_job_bytes(cases), lambda e, a, b, R, ex: e.DTW_global_banded_tb(a, b, R, ex))


def test_semiglobal_slot_reuse(semiglobal):
    cases, want = semiglobal
    assert min(int(w[2][0]) for w in want if len(w[2])) >= 30   # every path starts at a column j0 > 0
    slot_reuse("semiglobal", cases, want, dc.semiglobal_split(dc.semiglobal_cases()), dc.semiglobal_job_bytes(dc.semiglobal_cases()),
               lambda e, a, b, R, ex: e.DTW_semiglobal_tb(a, b, ex))


# ---- one context, three paths, shared grow-only buffers --------------------------------------------------------------------------------
def test_one_context_through_every_path_equals_fresh_contexts(banded, semiglobal):
    """a small full-matrix steps call, the banded list at 1 MiB, a small semiglobal call, a text-form call, a full-matrix call into
    page-locked arrays (dense: the paths come home in place) and the first call again, on ONE context: each result is what a fresh
    context gives for that call alone"""
    full = tc.edge_cases()[:24]
    pipe = tc.pipe_cases()[1:40]
    recs = np.zeros(len(full), ALN_REC_DTYPE)
    recs["off_i"], recs["off_j"], recs["mode"] = 11, 7, np.arange(len(full)) & 1
    arenas = {"full": make_arena_jobs(full), "pipe": make_arena_jobs(pipe), "banded": make_arena_jobs(banded[0]),
              "semiglobal": make_arena_jobs(semiglobal[0][:12])}

    def run(eng, which):
        name, path, mb, kw = which
        jobs, ev, rf = arenas[name]
        eng.upload_reference([rf], [rf])
        jobs = jobs.copy()
        jobs["ref_off"] += eng.reference_offset(0, 1)
        eng.set_option("tb_workspace_mb", mb)
        if path == "text":
            return [np.asarray(x) for x in eng.traceback_text(jobs, recs, ev)], eng.get_option("tb_sub_batches")
        st, out, off = steps_call(eng, path, jobs, ev, **kw)
        assert st == 0, which
        if path == "full":   # a dense stretch comes home whole: what lies behind a path's last element inside its room is not specified
            cost, plen, step, dist = out
            keep = np.zeros(len(step), bool)
            for k in range(len(jobs)):
                keep[int(off[k]):int(off[k]) + int(plen[k])] = True
            keep[int(off[-1]):] = True
            out = [cost, plen, step[keep], dist[keep]]
        return out, eng.get_option("tb_sub_batches")

    sequence = [("full", "full", 0, {}), ("banded", "banded", 1, {}), ("semiglobal", "semiglobal", 0, {}), ("full", "text", 0, {}),
                ("pipe", "full", 1, dict(page_locked=True)), ("full", "full", 0, {})]
    shared = ra.Engine(0)
    got = [run(shared, which) for which in sequence]
    shared.close()
    assert got[1][1] == len(dc.banded_split(banded[0])) and got[4][1] == len(tc.split(tc.shapes_of(pipe), tc.MIB)) >= 3
    for which, (out, subs) in zip(sequence, got):
        fresh = ra.Engine(0)
        alone, subs_alone = run(fresh, which)
        fresh.close()
        assert subs == subs_alone and len(out) == len(alone), which
        for x, y in zip(out, alone):
            assert x.tobytes() == y.tobytes(), which
    assert got[0][0][2].size > 1000 and all(x.tobytes() == y.tobytes() for x, y in zip(got[0][0], got[5][0]))


# ---- refusals write nothing and enqueue nothing ----------------------------------------------------------------------------------------
def refusal(path, cases, want, spoil, status, resets):
    """a good call, a refused one (`spoil` changes the job list), a good call: the refused call writes nothing; it leaves the timing
    getters and "tb_sub_batches" as they were -- but for the getter named in `resets`, which the entry has cleared by then"""
    eng, jobs, ev = engine_for(cases, tb_workspace_mb=dc.BUDGET_MB)
    st, good, off = steps_call(eng, path, jobs, ev, gap=1)
    assert st == 0
    check_paths(path, cases, want, good, off)
    before, subs = timings(eng), eng.get_option("tb_sub_batches")
    bad = jobs.copy()
    spoil(bad, ev)
    st, out, _ = steps_call(eng, path, bad, ev, gap=1)
    assert st == status and untouched(*out), (path, st)
    after = timings(eng)
    for p in PATHS:
        assert after[p] == ((0.0, 0.0, 0, 0) if p in resets else before[p]), (path, p)
    assert eng.get_option("tb_sub_batches") == (0 if resets else subs)
    st, again, _ = steps_call(eng, path, jobs, ev, gap=1)
    assert st == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(again, good))
    eng.close()


def beyond_events(jobs, ev):
    jobs["read_off"][len(jobs) - 2] = len(ev) - int(jobs["n"][len(jobs) - 2]) + 1


def zero_length(jobs, ev):
    jobs["n"][len(jobs) - 2] = 0


def test_banded_refusal(banded):
    cases, want = banded[0][:20], banded[1][:20]
    refusal("banded", cases, want, beyond_events, RANGE, ())
    refusal("banded", cases, want, zero_length, INVALID, ())


def test_semiglobal_refusal(semiglobal):
    cases, want = semiglobal[0][:12], semiglobal[1][:12]
    refusal("semiglobal", cases, want, beyond_events, RANGE, ())
    refusal("semiglobal", cases, want, zero_length, INVALID, ())


def test_full_matrix_refusal(oracle):
    """The full-matrix entries clear their getter and "tb_sub_batches" before they look at the jobs' lengths: a zero-length job is refused
    with both at zero.  A null argument is refused before that."""
    cases = tc.edge_cases()[:24]
    want = tc.oracle_paths(oracle, "edge")[:24]
    refusal("full", cases, want, zero_length, INVALID, ("full",))
    eng, jobs, ev = engine_for(cases)
    st, good, off = steps_call(eng, "full", jobs, ev, gap=1)
    before = timings(eng)
    cost, plen, dist = canaries(len(jobs), np.float32), canaries(len(jobs), np.uint32), canaries(int(off[-1]), np.float32)
    assert eng.lib.rawdtw_traceback_batch_steps(eng._ctx, vp(jobs), len(jobs), vp(ev), len(ev), vp(cost), vp(off), vp(plen), None, vp(dist)) == INVALID
    assert untouched(cost, plen, dist) and timings(eng) == before and eng.get_option("tb_sub_batches") == 1
    st, again, _ = steps_call(eng, "full", jobs, ev, gap=1)
    assert st == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(again, good))
    eng.close()
