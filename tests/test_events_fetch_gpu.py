"""rawdtw_events_fetch (k_events_gather, rawdtw_runs.hip): stretches of the context's event arena to the host, densely and in order,
against numpy slices of what was uploaded -- bit for bit, into page-locked memory (the device writes it) and pageable memory (staging
and one copy), with the sentinel behind the total untouched; and its refusals, which enqueue nothing."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra

pytestmark = pytest.mark.gpu
INVALID, RANGE = 1, 4
N_EV = 70_001                     # odd: the segment that ends at n_ev starts at an odd offset too
LENS = [0, 1, 3, 63, 64, 65, 255, 256, 257, 1025, 40_000]
SENTINEL = np.uint32(0x5EA7BEEF)
COUNTS = [0, 1, 64, 65]
TAIL = 16                         # sentinel floats behind the total


def vp(a):
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def arena():
    """70 001 distinct floats"""
    rng = np.random.default_rng(77)
    vals = (np.arange(N_EV, dtype=np.float32) * np.float32(0.5) + np.float32(3.0))
    vals = vals[rng.permutation(N_EV)].copy()
    assert len(np.unique(vals.view(np.uint32))) == N_EV
    return vals


@pytest.fixture(scope="module")
def engine(arena):
    e = ra.Engine(0)
    e.upload_events(arena)
    e.sync()
    yield e
    e.close()


def segments():
    """65 segments: LENS first -- the 40 000 one ends exactly at n_ev, the 257 one starts inside the 1 025 one, the others at permuted odd
    offsets with gaps below 30 000 -- then 54 more of the small lengths, a dozen of them empty, anywhere at odd offsets"""
    rng = np.random.default_rng(78)
    start = np.zeros(len(LENS), np.uint32)
    pos = 1
    for k in rng.permutation(len(LENS) - 1):      # (every length but the last)
        start[k] = pos
        pos += LENS[k] + 2 + int(rng.integers(0, 40))
        pos += 1 - pos % 2
    assert pos < N_EV - LENS[-1]
    start[-1] = N_EV - LENS[-1]
    i257, i1025 = LENS.index(257), LENS.index(1025)
    start[i257] = start[i1025] + 500 + 1 - (int(start[i1025]) + 500) % 2   # odd, and 257 floats of the 1 025 one's
    lens = list(LENS)
    starts = [int(s) for s in start]
    for k in range(65 - len(LENS)):
        ln = 0 if k % 4 == 0 else int(rng.choice(LENS[1:-1]))
        lens.append(ln)
        starts.append(int(rng.integers(0, (N_EV - ln) // 2)) * 2 + 1 if ln else int(rng.integers(0, N_EV // 2)) * 2 + 1)
    order = rng.permutation(len(LENS))             # (the long one and the empty one not at fixed places)
    starts[:len(LENS)] = [starts[k] for k in order]
    lens[:len(LENS)] = [lens[k] for k in order]
    return np.array(starts, np.uint32), np.array(lens, np.uint32)


def test_the_segment_list_has_the_properties_it_is_there_for():
    st, ln = segments()
    assert len(st) == 65 and sorted(ln[:11].tolist()) == LENS and np.all(st % 2 == 1)
    assert np.all(st.astype(np.int64) + ln <= N_EV)
    assert any(int(s) + int(l) == N_EV and l == 40_000 for s, l in zip(st, ln))
    a = [(int(s), int(s) + int(l)) for s, l in zip(st[:11], ln[:11]) if l in (257, 1025)]
    assert max(a[0][0], a[1][0]) < min(a[0][1], a[1][1])          # the two overlap
    assert not np.array_equal(np.argsort(st[:11], kind="stable"), np.arange(11)) and (ln == 0).sum() >= 10


class Pinned:
    """float32 array in rawdtw_host_alloc's memory"""

    def __init__(self, lib, n):
        self.lib, self.p = lib, C.c_void_p()
        assert lib.rawdtw_host_alloc(4 * max(n, 1), C.byref(self.p)) == 0 and self.p.value
        self.array = np.frombuffer((C.c_char * (4 * max(n, 1))).from_address(self.p.value), np.float32, max(n, 1))

    def free(self):
        self.array = None
        self.lib.rawdtw_host_free(self.p)


@pytest.mark.parametrize("pinned", [True, False], ids=["page-locked", "pageable"])
@pytest.mark.parametrize("count", COUNTS)
def test_segments_come_home_densely_in_order(engine, arena, count, pinned):
    lib = engine.lib
    st, ln = segments()
    st, ln = st[:count].copy(), ln[:count].copy()
    total = int(ln.astype(np.int64).sum())
    cap = total + TAIL
    buf = Pinned(lib, cap) if pinned else None
    out = buf.array if pinned else np.empty(cap, np.float32)
    try:
        assert lib.rawdtw_host_is_page_locked(vp(out)) == int(pinned)
        out.view(np.uint32)[:] = SENTINEL
        off = np.full(count + 1, 0xAAAAAAAA, np.uint64)
        engine._check(lib.rawdtw_events_fetch(engine._ctx, count, vp(st), vp(ln), vp(off), vp(out), cap))
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(ln.astype(np.uint64))]).astype(np.uint64))
        want = np.concatenate([arena[int(s):int(s) + int(l)] for s, l in zip(st, ln)] + [np.zeros(0, np.float32)])
        got = out.view(np.uint32)
        bad = np.nonzero(got[:total] != want.view(np.uint32))[0]
        assert len(bad) == 0, (count, pinned, bad[:8])
        assert np.all(got[total:] == SENTINEL)
        # the exact room, too
        out.view(np.uint32)[:] = SENTINEL
        engine._check(lib.rawdtw_events_fetch(engine._ctx, count, vp(st), vp(ln), vp(off), vp(out), total))
        assert np.array_equal(got[:total], want.view(np.uint32)) and np.all(got[total:] == SENTINEL)
    finally:
        if buf:
            buf.free()


def test_the_engines_form_returns_one_array_a_segment(engine, arena):
    st, ln = segments()
    got = engine.events_fetch(st, ln)
    assert len(got) == 65
    for g, s, l in zip(got, st, ln):
        assert np.array_equal(g.view(np.uint32), arena[int(s):int(s) + int(l)].view(np.uint32))
    assert engine.events_fetch([], []) == []


def test_refusals_enqueue_nothing(engine, arena):
    lib, c = engine.lib, engine._ctx
    st, ln = segments()
    st, ln = st[:11].copy(), ln[:11].copy()
    total = int(ln.sum())
    out = np.empty(total + TAIL, np.float32)
    out.view(np.uint32)[:] = SENTINEL
    off = np.zeros(12, np.uint64)
    # a segment one float past n_ev
    far_s, far_l = st.copy(), ln.copy()
    k = int(np.argmax(ln))
    far_l[k] += 1
    assert int(far_s[k]) + int(far_l[k]) == N_EV + 1
    assert lib.rawdtw_events_fetch(c, 11, vp(far_s), vp(far_l), vp(off), vp(out), len(out)) == INVALID
    assert "arena" in lib.rawdtw_last_error(c).decode()
    far_s, far_l = st.copy(), ln.copy()
    far_s[0], far_l[0] = N_EV, 1
    assert lib.rawdtw_events_fetch(c, 11, vp(far_s), vp(far_l), vp(off), vp(out), len(out)) == INVALID
    # out_cap one short: the offsets are filled, out is not touched
    off[:] = 0
    assert lib.rawdtw_events_fetch(c, 11, vp(st), vp(ln), vp(off), vp(out), total - 1) == RANGE
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(ln.astype(np.uint64))]).astype(np.uint64))
    assert np.all(out.view(np.uint32) == SENTINEL)
    # null arguments
    assert lib.rawdtw_events_fetch(None, 11, vp(st), vp(ln), vp(off), vp(out), len(out)) == INVALID
    assert lib.rawdtw_events_fetch(c, 11, None, vp(ln), vp(off), vp(out), len(out)) == INVALID
    assert lib.rawdtw_events_fetch(c, 11, vp(st), None, vp(off), vp(out), len(out)) == INVALID
    assert lib.rawdtw_events_fetch(c, 11, vp(st), vp(ln), None, vp(out), len(out)) == INVALID
    assert lib.rawdtw_events_fetch(c, 11, vp(st), vp(ln), vp(off), None, len(out)) == INVALID
    # a context with no arena
    bare = ra.Engine(0)
    try:
        one_s, one_l = np.array([0], np.uint32), np.array([0], np.uint32)
        assert lib.rawdtw_events_fetch(bare._ctx, 1, vp(one_s), vp(one_l), vp(off), vp(out), len(out)) == INVALID
        assert "arena" in lib.rawdtw_last_error(bare._ctx).decode()
    finally:
        bare.close()
    # a page-locked out whose allocation is smaller than out_cap: from its start, and from inside it
    small_s, small_l = np.array([1, 101], np.uint32), np.array([63, 65], np.uint32)
    buf = Pinned(lib, 2048)
    try:
        buf.array.view(np.uint32)[:] = SENTINEL
        beyond = 2048 + (16 << 20)   # (far beyond any rounding of the allocation)
        assert lib.rawdtw_events_fetch(c, 2, vp(small_s), vp(small_l), vp(off), vp(buf.array), beyond) == INVALID
        assert "page-locked" in lib.rawdtw_last_error(c).decode()
        assert lib.rawdtw_events_fetch(c, 2, vp(small_s), vp(small_l), vp(off), vp(buf.array[1024:]), beyond) == INVALID
        assert np.all(buf.array.view(np.uint32) == SENTINEL)
        # ... and one that holds them, from inside the allocation at an odd float: served in place
        engine._check(lib.rawdtw_events_fetch(c, 2, vp(small_s), vp(small_l), vp(off), vp(buf.array[1025:]), 1023))
        want = np.concatenate([arena[1:64], arena[101:166]]).view(np.uint32)
        got = buf.array.view(np.uint32)
        assert np.array_equal(got[1025:1025 + 128], want) and np.all(got[:1025] == SENTINEL) and np.all(got[1025 + 128:] == SENTINEL)
    finally:
        buf.free()
    assert np.all(out.view(np.uint32) == SENTINEL)
