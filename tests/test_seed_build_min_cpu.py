"""The parallel form of the minimizer sketch on the host (include/rawdtw.h: rawdtw_seed_sketch_windowed -- the kept events, every e-mer's
hash, then rawalign_amd/csrc/rawdtw_seed_min.h's step for every e-mer on its own, as rawdtw_seed_build.hip's kernels run it) against the
serial restatement of ri_sketch_min (rawdtw_seed_sketch) and the reference's recorded sketches (tests/golden/seed_min_ref.npz), element
for element and in order; the step itself against a copy of the serial loop in a stand-alone C++ program, plain and under
AddressSanitizer + UndefinedBehaviorSanitizer.  Exact equality of integers.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rawalign_amd import seeding
from rawalign_amd._lib import RawDTWError, SeedPars, load_library
from rawalign_amd.seeding import SeedParams
from tests import seed_build_min_cases as bc
from tests import seed_cases as sc
from tests import seed_min_cases as smc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")
INVALID, RANGE = 1, 4


def same_sketch(ev, p, what):
    h, pos = seeding.sketch_windowed(ev, p)
    wh, wp = seeding.sketch(ev, p)
    assert h.dtype == wh.dtype == np.uint32 and np.array_equal(h, wh) and np.array_equal(pos, wp), what
    return h, pos


# ---- the recorded cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", smc.CASES)
def test_windowed_equals_the_serial_sketch_and_the_fixture(name):
    """every chunk and every strand of every case of the tie fixture; the chunks' recorded sketches are the reference's own"""
    fx = smc.Fixture()
    fwd, rev, p, chunks = smc.build_case(name)
    assert p.w > 0 and sc.case_sha256(fwd, rev, chunks) == fx.sha(name)
    n = 0
    for c, ev in enumerate(chunks):
        h, pos = same_sketch(ev, p, (name, "chunk", c))
        wh, wp = fx.sketch(name, c)
        assert np.array_equal(h, wh) and np.array_equal(pos, wp), (name, c)
        n += len(h)
    for s, x in enumerate(list(fwd) + list(rev)):
        n += len(same_sketch(x, p, (name, "strand", s))[0])
    assert n > 0


def test_values_chunks_are_what_they_say():
    """the `values` case: a mask first, a mask mid-chunk (kept and coded under this rule), a NaN, the 0.3 threshold's neighbours"""
    fwd, rev, p, chunks = smc.build_case("values")
    first, mid, nan_in, special, threshold = chunks
    assert first[0] == smc.MASK_SIGNAL and mid[smc.mask_mid_chunk(fwd)[1]] == smc.MASK_SIGNAL and np.isnan(nan_in[50])
    assert np.sum(special == smc.MASK_SIGNAL) == 4 and np.isnan(special).sum() == 1
    for ev in chunks:
        h, pos = same_sketch(ev, p, "values")
        assert len(h) > 0
    # the mask is kept: its position is an e-mer's first event somewhere in the windowed sketch's e-mers
    kept = bc.kept_events(mid)
    assert smc.mask_mid_chunk(fwd)[1] in kept.tolist()
    d = np.abs(np.diff(threshold.astype(np.float32)))
    assert np.any(d == sc.DIFF) and np.any(d < sc.DIFF) and np.any(d > sc.DIFF)


# ---- random strands over the tie alphabets ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_strands():
    return [bc.random_strand(it) for it in range(bc.RANDOM_STRANDS)]


def test_windowed_equals_the_serial_sketch_on_random_strands(random_strands):
    seen, elements = set(), 0
    small_M = {w: set() for w in bc.RANDOM_W if w <= 16}
    for it, (ev, a, w, e) in enumerate(random_strands):
        assert len(ev) <= 700
        h, pos = same_sketch(ev, SeedParams(w=w, e=e), (it, a, w, e, len(ev)))
        seen.add((a, w, e))
        elements += len(h)
        if w <= 16 and (it // 108) % 2 == 1:   # (a strand of distinct neighbours: every event kept, M known from the length)
            small_M[w].add(max(len(ev) - e + 1, 0))
    assert seen == {(a, w, e) for a in bc.ALPHABETS for w in bc.RANDOM_W for e in bc.RANDOM_E}
    for w, Ms in small_M.items():
        assert Ms >= set(range(w + 2)), (w, sorted(Ms))
    assert elements > 100_000


def test_the_inputs_discriminate(random_strands):
    """The issue's rules, written again in Python from its text (tests/seed_build_min_cases.py: step_rules over numpy's own e-mer hashes),
    give the library's elements on every sixth random strand with w <= 16 -- and on those strands rule 1 (the first full window's equal
    hashes) and rule 3's tie list (equal hashes of the new minimum) both emit.  A step that left either out would differ here.
    The issue's third clause -- a strand with more elements than e-mers -- is dropped: no input yields one.  Neither these strands, nor the
    stand-alone program's 4 000 hash strings (it counts them), nor the fixture's cases: the serial loop emits an e-mer at most once."""
    by_rule = {1: 0, 2: 0, 3: 0, 30: 0, 5: 0}
    walked = more_than_M = 0
    for it, (ev, a, w, e) in enumerate(random_strands):
        if w > 16 or it % 6:
            continue
        p = SeedParams(w=w, e=e)
        h, first = bc.emer_hashes(ev, p)
        M = len(h)
        model = [x for m in range(M) for x in bc.step_rules(h, m, M, w)]
        got_h, got_pos = seeding.sketch_windowed(ev, p)
        assert [int(h[i]) for i, _ in model] == got_h.tolist() and [int(first[i]) for i, _ in model] == got_pos.tolist(), (it, a, w, e)
        for _, rule in model:
            by_rule[rule] += 1
        walked += 1
        more_than_M += len(model) > M
    print("strands walked:", walked, "elements by rule:", by_rule, "strands with more elements than e-mers:", more_than_M)
    assert walked > 100 and by_rule[1] > 0 and by_rule[30] > 0 and by_rule[2] > 0 and by_rule[3] > 0 and by_rule[5] > 0
    assert more_than_M == 0   # (see the docstring: were this ever to change, the clause comes back)


def test_the_boundary_strand_has_its_property():
    """the device test's strand: every event kept, and at e-mer TILE the minimum leaves the window with the new minimum's hash on both
    sides of TILE - 1 | TILE"""
    for w in bc.BOUNDARY_W:
        x = bc.boundary_strand(w)
        p = SeedParams(w=w, e=2)
        h, first = bc.emer_hashes(x, p)
        assert np.array_equal(first, np.arange(len(h))) and len(h) > bc.TILE + 1
        assert bc.leaves_at(h, bc.TILE, w)
        rules = [r for _, r in bc.step_rules(h, bc.TILE, len(h), w)]
        assert rules[0] == 3 and 30 in rules
        same_sketch(x, p, ("boundary", w))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_null_context_and_small_cap():
    lib = load_library()
    p, h = SeedPars(5, 6, 0, 9, 3, 6), C.c_void_p()
    assert lib.rawdtw_seed_index_build_device_min(None, C.byref(p), C.byref(h)) == INVALID and not h.value
    assert lib.rawdtw_seed_index_build_min_stats(None, None, None, None) == INVALID
    ev = bc.distinct_neighbours(300, 3, np.random.default_rng(3))
    pars = SeedParams(w=5, e=6)
    wh, wp = seeding.sketch(ev, pars)
    assert len(wh) > 40
    n = C.c_uint32(77)
    assert lib.rawdtw_seed_sketch_windowed(C.byref(pars.c()), ev.ctypes.data, len(ev), None, None, 0, C.byref(n)) == RANGE and n.value == len(wh)
    cap = len(wh) - 1
    gh, gp = np.full(len(wh), 0xABABABAB, np.uint32), np.full(len(wh), 0xABABABAB, np.uint32)
    n = C.c_uint32(77)
    assert lib.rawdtw_seed_sketch_windowed(C.byref(pars.c()), ev.ctypes.data, len(ev), gh.ctypes.data, gp.ctypes.data, cap, C.byref(n)) == RANGE
    assert n.value == len(wh) and np.array_equal(gh[:cap], wh[:cap]) and np.array_equal(gp[:cap], wp[:cap])
    assert gh[cap] == gp[cap] == 0xABABABAB   # (nothing behind the cap)
    with pytest.raises(RawDTWError) as err:
        seeding.sketch_windowed(ev, pars, cap=cap)
    assert err.value.status == RANGE and err.value.n == len(wh)
    assert lib.rawdtw_seed_sketch_windowed(C.byref(pars.c()), ev.ctypes.data, len(ev), gh.ctypes.data, gp.ctypes.data, len(wh), C.byref(n)) == 0
    for bad in (SeedParams(w=256), SeedParams(w=5, e=1)):
        assert lib.rawdtw_seed_sketch_windowed(C.byref(bad.c()), ev.ctypes.data, len(ev), gh.ctypes.data, gp.ctypes.data, len(wh), C.byref(n)) == INVALID
    # w = 0 has no window: ri_sketch_reg, as rawdtw_seed_sketch
    h0, p0 = seeding.sketch_windowed(ev, SeedParams())
    w0, q0 = seeding.sketch(ev, SeedParams())
    assert len(h0) == 295 and np.array_equal(h0, w0) and np.array_equal(p0, q0)


# ---- the step alone, stand-alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_step_equals_the_serial_loop_stand_alone(tmp_path, flags):
    """tests/abi/seed_min.cpp: rawdtw_seed_min.h under a plain compiler, every step handed exactly the hashes m - w .. m"""
    exe = os.path.join(str(tmp_path), "seed_min")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "abi", "seed_min.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe, "4000"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    word, n = run.stdout.split()
    assert word == "ok" and int(n) > 100_000, run.stdout + run.stderr
    assert "more elements than e-mers: 0" in run.stderr
