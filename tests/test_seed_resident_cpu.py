"""The resident seed index's two constructions on the host (rawalign_amd/csrc/rawdtw_seed_tile.h): the kept-event filter cut into tiles
against a copy of the serial loop, and the insertion of keys in any order against a copy of fill_table's loop -- each a stand-alone C++
program, plain and under AddressSanitizer + UndefinedBehaviorSanitizer; then rawdtw_seed_index_from_entries against
rawdtw_seed_index_build on the existing fixtures' entries, the refusals of the new entry points, and the cases module's own restatement
of the recurrence against the one the minimizer tests use.  Exact equality of integers.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rawalign_amd._lib import RawDTWError, SeedPars, SeedResidentStats, load_library
from rawalign_amd.seeding import SeedIndex, SeedParams
from tests import seed_build_min_cases as bc
from tests import seed_cases as sc
from tests import seed_resident_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")
INVALID, UNSUPPORTED = 1, 5
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")


def stand_alone(tmp_path, name, flags, arg):
    exe = os.path.join(str(tmp_path), name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "abi", name + ".cpp"), "-o", exe], check=True)
    run = subprocess.run([exe, arg], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout.split()


# ---- the two headers, stand-alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [(), SANITIZE], ids=["plain", "asan_ubsan"])
def test_tiled_filter_equals_the_serial_loop_stand_alone(tmp_path, flags):
    """tests/abi/seed_tile.cpp: both rules at tile sizes 1, 2, 3, 64 and the real one, on the edge strands and 3 000 random ones"""
    word, n, tile = stand_alone(tmp_path, "seed_tile", flags, "3000")
    assert word == "ok" and int(n) > 1_000_000 and int(tile) == rc.TILE


@pytest.mark.parametrize("flags", [(), SANITIZE], ids=["plain", "asan_ubsan"])
def test_insertion_in_any_order_equals_sequential_insertion_stand_alone(tmp_path, flags):
    """tests/abi/seed_insert.cpp: ascending, descending, random and interleaved schedules; the descending one is seen to displace"""
    word, n, displaced = stand_alone(tmp_path, "seed_insert", flags, "3000")
    assert word == "ok" and int(n) > 500_000 and int(displaced) > 0


# ---- the cases module's restatement -------------------------------------------------------------------------------------------------------
def test_the_restatement_of_the_recurrence_is_the_minimizer_tests_one():
    """kept_events(masked=False) is tests/seed_build_min_cases.py's float32 loop on strands with differences at, just below and just above
    0.3; masked=True differs from it exactly by the mask rule"""
    rng = np.random.default_rng(rc.SEED + 9)
    near = np.array([0, 0.3, 0.30000004, 0.29999998, 0.6, -0.3, 1.5, 0.1], np.float32)
    n = 0
    for it in range(60):
        x = near[rng.integers(0, len(near), 300)].copy()
        if it % 3 == 0:
            x[rng.integers(0, 300, 12)] = [np.nan, np.inf, -np.inf, rc.MASK] * 3
        if it % 6 == 0:
            x[0] = rc.MASK
        with np.errstate(invalid="ignore"):
            want = bc.kept_events(x)
        assert np.array_equal(rc.kept_events(x, False), want), it
        got = rc.kept_events(x, True)
        assert not np.any(x[got] == rc.MASK)
        n += len(want)
    assert n > 5000
    x = np.array([rc.MASK, 1.0, 1.1, rc.MASK, 1.2, 2.0], np.float32)   # event 0 masked: `last` stays the mask, the next event is kept
    assert rc.kept_events(x, True).tolist() == [1, 5] and rc.kept_events(x, False).tolist() == [0, 1, 3, 4, 5]


def test_the_crafted_tables_have_their_properties():
    names = [c[0] for c in rc.table_cases()]
    assert names == ["empty", "one", "keys_8", "keys_9", "all_single", "one_key", "list_of_2", "one_home", "wraps"]
    for name, hs, ys in rc.table_cases():
        assert hs.dtype == np.uint32 and ys.dtype == np.uint64 and len(hs) == len(ys)
        order = np.lexsort((ys, hs))
        assert np.array_equal(order, np.arange(len(hs))), name
    _, hs, _ = [c for c in rc.table_cases() if c[0] == "wraps"][0]
    keys = np.unique(hs)
    lg = rc.log2_slots(len(keys))
    homes = [rc.first_slot(h, lg) for h in keys]
    assert homes.count((1 << lg) - 1) == 12 and min(homes) == 0   # more keys on the last slot than it and its neighbours hold


# ---- through the library ------------------------------------------------------------------------------------------------------------------
def entries_of(six):
    keys = np.sort(six.keys())
    lists = [six.get(int(k)) for k in keys]
    return np.repeat(keys, [len(y) for y in lists]).astype(np.uint32), np.concatenate(lists + [np.zeros(0, np.uint64)])


@pytest.mark.parametrize("name", ["e6", "e2", "motif", "w5"])
def test_from_entries_equals_the_host_build_on_the_fixtures_entries(name):
    fwd, rev, p, _ = sc.build_case(name)
    want = SeedIndex.from_signals(fwd, rev, p, threads=4)
    hs, ys = entries_of(want)
    got = SeedIndex.from_entries(p, want.n_seq, hs, ys)
    assert not got.resident and len(hs) == want.n_positions > 400   # (the smallest, e2, has 492)
    assert (got.n_seq, got.n_keys, got.n_positions, got.table_bytes, got.pars) == (want.n_seq, want.n_keys, want.n_positions, want.table_bytes, want.pars)
    assert np.array_equal(got.keys(), want.keys())   # (table order: the slots' layout)
    for h in want.keys().tolist() + [0, 1, 0xFFFFFFFF]:
        assert np.array_equal(got.get(h), want.get(h)), (name, h)


@pytest.mark.parametrize("case", rc.table_cases(), ids=lambda c: c[0])
def test_from_entries_on_the_crafted_tables(case):
    name, hs, ys = case
    six = SeedIndex.from_entries(SeedParams(), 3, hs, ys)
    keys = np.unique(hs)
    assert six.n_keys == len(keys) and six.n_positions == len(hs)
    lg = rc.log2_slots(len(keys))
    assert six.table_bytes == (1 << lg) * 16 + 8 * sum(int(c) for c in np.unique(hs, return_counts=True)[1] if c > 1)
    assert sorted(six.keys().tolist()) == keys.tolist()
    for h in keys.tolist():
        assert np.array_equal(six.get(h), ys[hs == h])


def test_unsorted_entries_and_null_contexts_are_refused():
    lib = load_library()
    p, h = SeedPars(0, 6, 0, 9, 3, 6), C.c_void_p()
    hs, ys = np.array([5, 5, 7], np.uint32), np.array([8, 9, 1], np.uint64)
    assert lib.rawdtw_seed_index_from_entries(C.byref(p), 1, 3, hs.ctypes.data, ys.ctypes.data, C.byref(h)) == 0 and h.value
    assert lib.rawdtw_seed_index_is_resident(h) == 0 and lib.rawdtw_seed_index_is_resident(None) == 0
    lib.rawdtw_seed_index_destroy(h)
    for bad_h, bad_y in (([7, 5, 5], [1, 8, 9]), ([5, 5, 7], [9, 8, 1])):   # hashes that descend; a group's positions that descend
        with pytest.raises(RawDTWError) as err:
            SeedIndex.from_entries(SeedParams(), 1, bad_h, bad_y)
        assert err.value.status == INVALID
    h = C.c_void_p(1)
    assert lib.rawdtw_seed_index_from_entries(C.byref(SeedPars(0, 1, 0, 9, 3, 6)), 1, 3, hs.ctypes.data, ys.ctypes.data, C.byref(h)) == INVALID and not h.value
    assert lib.rawdtw_seed_index_from_entries(C.byref(p), 1, 3, None, ys.ctypes.data, C.byref(h)) == INVALID
    # the device entries without a context
    h = C.c_void_p(1)
    assert lib.rawdtw_seed_index_build_resident(None, C.byref(p), C.byref(h)) == INVALID
    assert lib.rawdtw_seed_table_from_entries(None, C.byref(p), 1, 3, hs.ctypes.data, ys.ctypes.data, C.byref(h)) == INVALID
    assert lib.rawdtw_seed_index_build_resident_stats(None, C.byref(SeedResidentStats())) == INVALID
    six = SeedIndex.from_entries(SeedParams(), 1, hs, ys)
    assert lib.rawdtw_seed_index_fetch(None, six._h) == INVALID
