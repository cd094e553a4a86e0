"""rawdtw_traceback_arena_steps: the traceback over the context's event arena as it lies.  The read pieces are appended into a reserved
arena at permuted odd offsets with gaps; the same jobs over the same pieces laid densely go through rawdtw_traceback_batch_steps on a
second context -- costs, lengths, step bytes and distances must be the same bits, in one sub-batch and in several --, a subset is checked
against the oracle's dtw_global_tb, and afterwards the arena is what it was."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd.dtw import JOB_DTYPE
from tests.util import make_arena_jobs

pytestmark = pytest.mark.gpu
INVALID = 1
# tests/test_gpu_parity.py's traceback shapes (shorter sides in every rows-per-lane class: <= 64, <= 128, <= 256, above; one, two and
# three strips), and two dozen small ones
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (30, 20), (64, 64), (65, 100), (130, 129), (260, 300), (513, 600), (600, 513), (900, 1100),
          (1500, 1300), (1100, 2600)]
ORACLE_SUBSET = (0, 2, 4, 5, 6, 7, 8, 9, 14, 20, 37)


def vp(a):
    return C.c_void_p(a.ctypes.data)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(606)
    shapes = SHAPES + [(int(rng.integers(1, 90)), int(rng.integers(1, 90))) for _ in range(24)]
    return [(rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32), -1, k % 3 == 1) for k, (n, m) in enumerate(shapes)]


def scattered(cases):
    """the pieces' places in the arena: a permuted order, odd starts, gaps; the last one placed ends exactly at n_ev -> (dst, n_ev)"""
    rng = np.random.default_rng(607)
    dst = np.zeros(len(cases), np.uint32)
    pos = 3
    for k in rng.permutation(len(cases)):
        pos += 1 - pos % 2
        dst[k] = pos
        pos += len(cases[k][0]) + int(rng.integers(0, 50))
        last = k
    n_ev = int(dst[last]) + len(cases[last][0])
    assert np.all(dst % 2 == 1) and not np.array_equal(np.argsort(dst), np.arange(len(cases)))
    return dst, n_ev


@pytest.fixture(scope="module")
def setup(cases):
    """engine A: the reserved arena with the pieces appended where `scattered` puts them, and the jobs over it; engine B: nothing but the
    reference.  -> (A, B, arena jobs, dense jobs, dense events, dst, lens, n_ev)"""
    jobs, ev, rf = make_arena_jobs(cases)
    dst, n_ev = scattered(cases)
    lens = jobs["n"].astype(np.uint32)
    a, b = ra.Engine(0), ra.Engine(0)
    for e in (a, b):
        e.upload_reference([rf], [rf])
    jobs["ref_off"] += a.reference_offset(0, 1)
    assert a.reference_offset(0, 1) == b.reference_offset(0, 1)
    a.reserve_events(n_ev)
    src = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.uint64)
    a.append_events(ev, src, dst)
    arena_jobs = jobs.copy()
    arena_jobs["read_off"] = dst
    yield a, b, arena_jobs, jobs, ev, dst, lens, n_ev
    a.close()
    b.close()


def dense_steps(e, jobs, ev):
    caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
    off = np.concatenate([[0], np.cumsum(caps)]).astype(np.uint64)
    cost, plen = np.zeros(len(jobs), np.float32), np.zeros(len(jobs), np.uint32)
    step, dist = np.full(int(off[-1]) + 1, 0xEE, np.uint8), np.zeros(int(off[-1]) + 1, np.float32)
    e._check(e.lib.rawdtw_traceback_batch_steps(e._ctx, vp(jobs), len(jobs), vp(ev), len(ev), vp(cost), vp(off), vp(plen), vp(step), vp(dist)))
    return cost, off, plen, step, dist


def same_paths(got, want, what):
    gc, goff, glen, gstep, gd = got
    wc, woff, wlen, wstep, wd = want
    assert np.array_equal(goff, woff) and np.array_equal(glen, wlen), what
    assert np.array_equal(bits(gc), bits(wc)), what
    for k in range(len(glen)):
        s, n = int(goff[k]), int(glen[k])
        assert np.array_equal(gstep[s:s + n], wstep[s:s + n]), (what, k)
        assert np.array_equal(bits(gd[s:s + n]), bits(wd[s:s + n])), (what, k)


@pytest.fixture(scope="module")
def want(setup):
    """rawdtw_traceback_batch_steps on the second context, the pieces dense: computed once, never changed"""
    _, b, _, jobs, ev, _, _, _ = setup
    out = dense_steps(b, jobs, ev)
    for x in out:
        x.setflags(write=False)
    return out


def whole_arena(a, n_ev):
    return a.events_fetch([0], [n_ev])[0]


def test_the_arena_form_equals_the_steps_form_and_the_oracle(setup, want, cases, oracle):
    a, _, arena_jobs, _, _, _, _, n_ev = setup
    before = whole_arena(a, n_ev)
    got = a.traceback_arena_steps(arena_jobs)
    assert a.get_option("tb_sub_batches") == 1
    same_paths(got, want, "one sub-batch")
    cost, off, plen, step, dist = got
    for k in ORACLE_SUBSET:
        x, y, _, ex = cases[k]
        c, pi, pj, pd = oracle.dtw_global_tb(x, y, ex)
        s, n = int(off[k]), int(plen[k])
        assert n == len(pi) and bits(cost[k]) == bits(c), k
        st = step[s:s + n]
        assert st[0] == 0 and np.array_equal(np.cumsum(st & 1), pi) and np.array_equal(np.cumsum(st >> 1), pj), k
        assert np.array_equal(bits(dist[s:s + n]), bits(pd)), k
    assert np.array_equal(bits(whole_arena(a, n_ev)), bits(before))


def test_several_sub_batches_give_the_same(setup, want):
    a, b, arena_jobs, jobs, ev, _, _, _ = setup
    try:
        for e in (a, b):
            e.set_option("tb_workspace_mb", 1)
        got = a.traceback_arena_steps(arena_jobs)
        n_sub = a.get_option("tb_sub_batches")
        assert n_sub >= 3
        same_paths(got, want, "several sub-batches")
        same_paths(dense_steps(b, jobs, ev), want, "the steps form, several sub-batches")
        assert b.get_option("tb_sub_batches") == n_sub
    finally:
        for e in (a, b):
            e.set_option("tb_workspace_mb", 0)


def test_the_arena_is_intact_afterwards(setup, cases):
    a, b, arena_jobs, jobs, ev, dst, lens, n_ev = setup
    before = whole_arena(a, n_ev)
    cost_before = b.score_batch(jobs, ev)          # (the second context: the pieces dense)
    a.traceback_arena_steps(arena_jobs)
    pieces = a.events_fetch(dst, lens)
    for k, (x, _, _, _) in enumerate(cases):
        assert np.array_equal(bits(pieces[k]), bits(x)), k
    after = whole_arena(a, n_ev)
    assert np.array_equal(bits(after), bits(before))
    # scoring on the arena as it lies (a plan uploads no event) ...
    pl = a.plan(arena_jobs)
    pl.run()
    assert np.array_equal(bits(pl.fetch()), bits(cost_before))
    pl.close()
    # ... and rawdtw_score_batch given what the fetch brought home
    assert np.array_equal(bits(a.score_batch(arena_jobs, after)), bits(cost_before))


def test_refusals(setup):
    a, b, arena_jobs, _, _, dst, lens, n_ev = setup
    lib = a.lib
    caps = arena_jobs["n"].astype(np.uint64) + arena_jobs["m"].astype(np.uint64) - 1
    off = np.concatenate([[0], np.cumsum(caps)]).astype(np.uint64)
    cost, plen = np.zeros(len(arena_jobs), np.float32), np.zeros(len(arena_jobs), np.uint32)
    step, dist = np.full(int(off[-1]) + 2, 0xEE, np.uint8), np.zeros(int(off[-1]) + 2, np.float32)
    # a job reaching one float past n_ev
    k = int(np.argmax(dst.astype(np.int64) + lens))
    assert int(dst[k]) + int(lens[k]) == n_ev
    far = np.ascontiguousarray(arena_jobs.copy(), JOB_DTYPE)
    far["read_off"][k] += 1
    before = whole_arena(a, n_ev)
    assert lib.rawdtw_traceback_arena_steps(a._ctx, vp(far), len(far), vp(cost), vp(off), vp(plen), vp(step), vp(dist)) == INVALID
    assert "arena" in lib.rawdtw_last_error(a._ctx).decode()
    assert np.all(step == 0xEE) and np.array_equal(bits(whole_arena(a, n_ev)), bits(before))
    # null arguments
    assert lib.rawdtw_traceback_arena_steps(None, vp(far), len(far), vp(cost), vp(off), vp(plen), vp(step), vp(dist)) == INVALID
    assert lib.rawdtw_traceback_arena_steps(a._ctx, vp(far), len(far), vp(cost), vp(off), vp(plen), None, vp(dist)) == INVALID
    # a context with no arena (the second engine never had events before this module's dense calls: a fresh one)
    bare = ra.Engine(0)
    try:
        one = np.ascontiguousarray(arena_jobs[:1].copy(), JOB_DTYPE)
        assert lib.rawdtw_traceback_arena_steps(bare._ctx, vp(one), 1, vp(cost), vp(off), vp(plen), vp(step), vp(dist)) == INVALID
        assert "arena" in lib.rawdtw_last_error(bare._ctx).decode()
    finally:
        bare.close()
    assert np.all(step == 0xEE)
