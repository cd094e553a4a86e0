"""The index build's entry points beside one another on one context (include/rawdtw.h: rawdtw_seed_index_build_device, _build_device_min,
_build_resident, rawdtw_seed_table_from_entries and the three _stats readers): every entry in alternation, each table against the host's
from the same arrays and each statistic written by the entry that owns it and by no other; refused calls, which leave every statistic and
the context's table; and a reference that yields no entry.  Integers, bytes and status codes only: a time is finite and not negative.
Inputs: tests/seed_build_min_cases.py, tests/seed_resident_cases.py, tests/seed_cases.py.  Nothing here reads the reference itself."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import seeding
from rawalign_amd._lib import RawDTWError
from rawalign_amd.seeding import SeedIndex, SeedParams
from tests import seed_build_min_cases as bc
from tests import seed_cases as sc
from tests import seed_resident_cases as rc
from tests.test_refsig_scale_gpu import same_header, same_lists

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 5
ABSENT = [0, 1, 0xFFFFFFFF, 12345]


@pytest.fixture()
def eng():
    e = ra.Engine(0)
    e.set_option("seed_minimizer", 1)
    yield e
    e.close()


def stats(eng):
    """(rawdtw_seed_index_build_stats, _build_min_stats, _build_resident_stats), every time finite and not negative"""
    out = (eng.seed_build_stats(), eng.seed_build_min_stats(), eng.seed_build_resident_stats())
    for d in out:
        for k, v in d.items():
            if k.endswith("_ms"):
                assert math.isfinite(v) and v >= 0, (k, v)
    return out


def same_index(got, want, what):
    same_header(got, want, what)
    same_lists(got, want, want.keys().tolist() + ABSENT, what)


def refused(status, fn, *a, **kw):
    with pytest.raises(RawDTWError) as err:
        fn(*a, **kw)
    assert err.value.status == status, err.value


def resident_numbers(st, fwd, rev, p, want, what):
    """what tests/test_seed_resident_gpu.py's same_table holds a resident build's statistics to"""
    kept, entries = rc.kept_and_entries(fwd, rev, p)
    assert st["tile"] == rc.TILE and st["tiles"] == 2 * sum((len(x) + rc.TILE - 1) // rc.TILE for x in fwd), what
    assert st["kept"] == kept and entries in (None, st["entries"]), what
    assert st["entries"] == want.n_positions and st["keys"] == want.n_keys and st["log2_slots"] == rc.log2_slots(want.n_keys), what


def test_every_entry_in_alternation_on_one_context(eng):
    """device, device_min, resident at w = 0 and w = 5, from_entries, device again: each table equals the host's, and each statistic is
    written by the entries that own it alone"""
    fwd, rev, Ms = bc.edge_reference(5, 6)
    assert len(fwd[1]) == 0 and sum(0 < len(x) < 6 for x in fwd) >= 2
    p0, p5 = SeedParams(w=0, e=6), SeedParams(w=5, e=6)
    want = {0: SeedIndex.from_signals(fwd, rev, p0, threads=4), 5: SeedIndex.from_signals(fwd, rev, p5, threads=4)}
    assert want[5].n_positions < want[0].n_positions == 2 * sum(Ms)
    name, hs, ys = [c for c in rc.table_cases() if c[0] == "wraps"][0]
    want_entries = SeedIndex.from_entries(SeedParams(), 3, hs, ys)
    eng.upload_reference(fwd, rev)
    build, mins, res = stats(eng)

    # 1. rawdtw_seed_index_build_device, w = 0
    got = SeedIndex.from_device(eng, p0)
    same_index(got, want[0], "device w0")
    got.close()
    assert stats(eng)[1:] == (mins, res)

    # 2. rawdtw_seed_index_build_device_min, w = 5
    got = SeedIndex.from_device(eng, p5, minimizer=True)
    same_index(got, want[5], "device_min w5")
    got.close()
    build, mins, now_res = stats(eng)
    assert (mins["entries"], mins["emers"]) == (want[5].n_positions, 2 * sum(Ms)) and now_res == res

    # 3. rawdtw_seed_index_build_resident, w = 0
    got = SeedIndex.from_device(eng, p0, resident=True)
    assert got.resident
    build, now_mins, res = stats(eng)
    got.fetch(eng)
    same_index(got, want[0], "resident w0")
    got.close()
    assert now_mins == mins
    resident_numbers(res, fwd, rev, p0, want[0], "resident w0")

    # 4. rawdtw_seed_index_build_resident, w = 5
    got = SeedIndex.from_device(eng, p5, resident=True)
    assert got.resident
    build, mins, res = stats(eng)
    got.fetch(eng)
    same_index(got, want[5], "resident w5")
    got.close()
    assert (mins["entries"], mins["emers"]) == (want[5].n_positions, 2 * sum(Ms))
    resident_numbers(res, fwd, rev, p5, want[5], "resident w5")

    # 5. rawdtw_seed_table_from_entries
    got = SeedIndex.from_entries(SeedParams(), 3, hs, ys, engine=eng)
    assert got.resident
    now_build, now_mins, res = stats(eng)
    got.fetch(eng)
    same_header(got, want_entries, name)
    same_lists(got, want_entries, np.unique(hs).tolist() + ABSENT, name)
    got.close()
    assert now_build == build and now_mins == mins
    assert (res["tiles"], res["kept"], res["entries"]) == (0, 0, len(hs))
    assert res["keys"] == want_entries.n_keys == len(np.unique(hs)) and res["log2_slots"] == rc.log2_slots(want_entries.n_keys)

    # 6. rawdtw_seed_index_build_device, w = 0, again
    got = SeedIndex.from_device(eng, p0)
    same_index(got, want[0], "device w0 again")
    got.close()
    assert stats(eng)[1:] == (mins, res)


def test_refused_calls_leave_every_statistic_and_the_table(eng):
    fwd, rev, p, chunks = sc.build_case("e6")
    ev, off = sc.flat(chunks)
    p5 = dataclasses.replace(p, w=5)
    eng.upload_reference(fwd, rev)
    si = SeedIndex.from_device(eng, p5, resident=True)
    before = stats(eng)
    assert before[1]["entries"] == before[2]["entries"] > 0
    want_off, want_hits = eng.seed_hits(ev, off)
    assert len(want_hits) > 0
    for kw in ({}, {"minimizer": True}, {"resident": True}):
        for bad in (SeedParams(w=256), SeedParams(e=1), SeedParams(w=5, e=1)):
            refused(INVALID, SeedIndex.from_device, eng, bad, **kw)
    refused(UNSUPPORTED, SeedIndex.from_device, eng, SeedParams(w=5))   # (rawdtw_seed_index_build_device itself refuses w > 0)
    refused(INVALID, SeedIndex.from_entries, SeedParams(), 1, [7, 5], [1, 2], engine=eng)   # unsorted
    fresh = ra.Engine(0)
    try:
        fresh_before = stats(fresh)
        for kw in ({}, {"minimizer": True}, {"resident": True}):
            refused(INVALID, SeedIndex.from_device, fresh, p5 if kw else p, **kw)   # no reference on the context
        assert stats(fresh) == fresh_before
    finally:
        fresh.close()
    hoff, hits = np.zeros(len(off), np.uint64), np.zeros(max(len(want_hits), 1), seeding.HIT_DTYPE)
    eng._check(eng.lib.rawdtw_seed_begin(eng._ctx, len(off) - 1, off.ctypes.data, ev.ctypes.data, hoff.ctypes.data, hits.ctypes.data, len(hits)))
    try:   # a seeding begun and not ended: the context's table is in use
        refused(INVALID, SeedIndex.from_device, eng, p5, resident=True)
        refused(INVALID, SeedIndex.from_entries, SeedParams(), 1, [5, 7], [1, 2], engine=eng)
    finally:
        eng._check(eng.lib.rawdtw_seed_end(eng._ctx, C.byref(C.c_float())))
    assert np.array_equal(hoff, want_off) and hits[:len(want_hits)].tobytes() == want_hits.tobytes()
    assert stats(eng) == before
    got_off, got_hits = eng.seed_hits(ev, off)
    assert np.array_equal(got_off, want_off) and got_hits.tobytes() == want_hits.tobytes() and si.resident
    si.close()


@pytest.mark.parametrize("w", [0, 5])
def test_a_reference_that_yields_no_entry(eng, w):
    """sequences of 0 and 3 events at e = 6: events on the device, no e-mer, a table of 16 empty slots from all three builds"""
    rng = np.random.default_rng(7)
    fwd, rev = [np.zeros(0, np.float32), bc.all_kept(3, rng)], [np.zeros(0, np.float32), bc.all_kept(3, rng)]
    p = SeedParams(w=w, e=6)
    want = SeedIndex.from_signals(fwd, rev, p)
    assert want.n_keys == 0 and want.n_positions == 0
    eng.upload_reference(fwd, rev)
    for kw in ({}, {"minimizer": True}, {"resident": True}):
        if w and not kw:
            continue   # (rawdtw_seed_index_build_device takes w = 0 alone)
        got = SeedIndex.from_device(eng, p, **kw)   # (any status but RAWDTW_OK raises)
        build, mins, res = stats(eng)
        if kw.get("resident"):
            assert got.resident and (res["entries"], res["keys"], res["log2_slots"]) == (0, 0, rc.log2_slots(0))
            assert (res["tiles"], res["kept"]) == (2, 6)
            chunk = bc.all_kept(200, rng)
            hoff, hits = eng.seed_hits(chunk, np.array([0, len(chunk)], np.uint64))
            assert hoff.tolist() == [0, 0] and len(hits) == 0
            got.fetch(eng)
        if w:
            assert (mins["emers"], mins["entries"]) == (0, 0)
        same_header(got, want, (w, kw))
        for h in ABSENT + [7, 0x80000000]:
            assert len(got.get(h)) == 0, (w, kw, h)
        got.close()
