"""The semiglobal traceback in windows without a device (include/rawdtw.h, "semiglobal, in windows").

rawdtw_semiglobal_tb_window_host -- checkpoint columns from a cost-only pass, windows refilled from them, the walk handed from window
to window -- against the n x m forms: rawdtw_semiglobal_tb_host on the device tests' sweep and value domains, the reference's own
recorded paths (tests/golden/semiglobal_ref.npz), and the numpy model on planted paths that cross several windows.  Compared each
time: cost bits, end_j, j0, the length and every element.  The windows a path enters are counted from the numpy model's path
(tests/semiglobal_window_cases.py), not by the code under test.

The layout (rawalign_amd/csrc/rawdtw_semi_window.h) is checked by a stand-alone C++ program, tests/abi/semi_window_layout.cpp, built
plain and with AddressSanitizer + UndefinedBehaviorSanitizer (its own main: nothing is preloaded), against the Python restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rawalign_amd as ra
from tests import semiglobal_cases as sc
from tests import semiglobal_window_cases as wc
from tests import value_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")
COLUMNS = (64, 128)
INVALID = 1


def same(got, want, what):
    """(DtwResult, end_j) twice: cost bits, end_j, j0, lengths and every element"""
    (r, ej), (w, wej) = got, want
    assert sc.bits(r.cost)[0] == sc.bits(w.cost)[0] and ej == wej and len(r.i) == len(w.i), what
    assert np.array_equal(r.i, w.i) and np.array_equal(r.j, w.j) and np.array_equal(sc.bits(r.difference), sc.bits(w.difference)), what
    if len(w.i):
        assert r.j[0] == w.j[0], what


def windowed(a, b, cols, ex):
    r, ej, windows = ra.semiglobal_tb_window_host(a, b, cols, ex)
    return (r, ej), windows


def test_sweep_against_the_matrix_form():
    rng = np.random.default_rng(1515)
    shapes = [(n, m) for n in sc.SWEEP_N for m in sc.SWEEP_M] + list(sc.TALL)
    most = 0
    for q, (n, m) in enumerate(shapes):
        for a, b in ((rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32)),
                     (rng.integers(-2, 3, n).astype(np.float32), rng.integers(-2, 3, m).astype(np.float32))):
            for ex in (0, 1):
                want = ra.semiglobal_host(a, b, ex, traceback=True)
                for cols in COLUMNS:
                    got, windows = windowed(a, b, cols, ex)
                    same(got, want, (n, m, ex, cols))
                    assert (windows == 0) == (m <= cols or n == 1), (n, m, cols, windows)
                    most = max(most, windows)
    assert most >= 3   # (premise: some of the sweep's paths are handed from window to window)


def test_planted_end_columns_against_the_matrix_form():
    for n, m in ((20, 130), (130, 700), (257, 400)):
        for at in sc.PLANT_AT + (127, 128, 129):
            a, b = sc.planted(n, m, (at,))
            for ex in (0, 1):
                want = ra.semiglobal_host(a, b, ex, traceback=True)
                assert want[1] == at % m
                for cols in COLUMNS:
                    same(windowed(a, b, cols, ex)[0], want, (n, m, at, ex, cols))


def test_value_domains_against_the_matrix_form():
    for name in vc.DOMAIN_NAMES:
        rng = vc.domain_rng(name, salt=47)
        for n, m in sc.DOMAIN_SHAPES + ((70, 300), (129, 322)):
            a, b = vc.DOMAINS[name](rng, n), vc.DOMAINS[name](rng, m)
            for ex in (0, 1):
                want = ra.semiglobal_host(a, b, ex, traceback=True)
                for cols in COLUMNS:
                    same(windowed(a, b, cols, ex)[0], want, (name, n, m, ex, cols))


def test_against_the_recorded_reference():
    fx = sc.Fixture()
    multi = 0
    for k in range(len(fx)):
        a, b = fx.inputs(k)
        for ex in (0, 1):
            wi, wj, wd = fx.path(k, ex)
            for cols in COLUMNS:
                (r, ej), windows = windowed(a, b, cols, ex)
                what = (fx.tag(k), k, len(a), len(b), ex, cols)
                assert sc.bits(r.cost)[0] == fx.z["tb_cost"][k, ex] and ej == fx.z["end_j"][k], what
                assert np.array_equal(r.i, wi) and np.array_equal(r.j, wj) and np.array_equal(sc.bits(r.difference), sc.bits(wd)), what
                multi += windows > 1
    assert multi >= 10   # (the fixture's widest cases are 130 and 140 columns: two or three windows at 64)


@pytest.fixture(scope="module")
def planted():
    """[(tag, a, b, pi, pj, end_j)] with the numpy model's full path"""
    return [(tag, a, b) + wc.full_path(a, b) for tag, a, b in wc.planted_cases()]


def test_planted_multi_window_paths(planted):
    cols = wc.C64
    counts, exits, first_column, not_windowed = [], [], 0, 0
    for tag, a, b, pi, pj, end_j in planted:
        n_win = wc.windows_of(pi, pj, len(b), cols)
        counts.append(n_win)
        exits += wc.exits_of(pi, pj, len(b), cols)
        first_column += len(b) > cols and pj[0] % cols == 0 and pj[0] > 0
        not_windowed += len(b) <= cols
        for ex in (0, 1):
            m_cost, m_ej, m_i, m_j, m_d = sc.model(a, b, bool(ex))
            (r, ej), windows = windowed(a, b, cols, ex)
            assert sc.bits(r.cost)[0] == sc.bits(m_cost)[0] and ej == m_ej == end_j, (tag, ex)
            assert np.array_equal(r.i, m_i) and np.array_equal(r.j, m_j) and np.array_equal(sc.bits(r.difference), sc.bits(m_d)), (tag, ex)
            assert windows == n_win, (tag, ex, windows, n_win)
            same((r, ej), ra.semiglobal_host(a, b, ex, traceback=True), (tag, ex))
            for other in (128, 256):   # (and a wider window on the same paths)
                (r2, ej2), w2 = windowed(a, b, other, ex)
                same((r2, ej2), (r, ej), (tag, ex, other))
                assert w2 == wc.windows_of(pi, pj, len(b), other), (tag, ex, other)
    # the conditions the plants are there for, from the numpy paths alone
    ends = {tag.split()[1]: end_j % cols for tag, _, _, _, _, end_j in planted if tag.startswith("end ")}
    assert ends == {"kC-1": cols - 1, "kC": 0, "kC+1": 1}, ends
    assert max(counts) >= 4 and sum(c >= 3 for c in counts) >= 5, counts
    assert "left" in exits and "diag" in exits, exits
    assert first_column >= 1                      # a walk that reaches i == 0 in a window's first column
    assert not_windowed == 1 and counts[[t for t, *_ in planted].index("m == C")] == 0
    assert counts[[t for t, *_ in planted].index("m == C + 1")] >= 1


def test_refusals_and_the_plain_form():
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=20).astype(np.float32), rng.normal(size=90).astype(np.float32)
    for bad in (1, 63, 65, 100, (1 << 20) + 64, 1 << 21):
        with pytest.raises(ra.RawDTWError) as e:
            ra.semiglobal_tb_window_host(a, b, bad)
        assert e.value.status == INVALID
    for x, y in ((a[:0], b), (a, b[:0])):
        with pytest.raises(ra.RawDTWError):
            ra.semiglobal_tb_window_host(x, y, 64)
    want = ra.semiglobal_host(a, b, 0, traceback=True)
    for cols in (0, 128, 1 << 20):   # off, and m <= C: the n x m form, no window
        got, windows = windowed(a, b, cols, 0)
        same(got, want, cols)
        assert windows == 0
    lib = ra.load_library()
    col = C.c_uint32(7)
    assert lib.rawdtw_set_semiglobal_window(None, 64) == INVALID and lib.rawdtw_get_semiglobal_window(None, C.byref(col)) == INVALID and col.value == 7
    assert lib.rawdtw_semiglobal_window_stats(None, None, None, None, None) == INVALID


# ---- the layout ---------------------------------------------------------------------------------------------------------------------
FLAGS = {"plain": (), "asan_ubsan": ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")}
SWEEP_CASES = 14 * 12 * 7   # n x m x C


@pytest.fixture(scope="module", params=sorted(FLAGS))
def program(request, tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("semi_window_layout")), "semi_window_layout")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *FLAGS[request.param], "-I", CSRC,
                    os.path.join(ROOT, "tests", "abi", "semi_window_layout.cpp"), "-o", exe], check=True)
    return exe


def run(program, mode, text):
    """the program's output: the sweep's line, or a tuple of numbers a line"""
    got = subprocess.run([program] + ([mode] if mode else []), input=text, capture_output=True, text=True, timeout=300)
    assert got.returncode == 0, got.stdout + got.stderr
    if not mode:
        return got.stdout
    return [tuple(int(x) for x in line.split()) for line in got.stdout.splitlines()]


def test_layout_sweep(program):
    assert run(program, None, "").strip() == "ok %d" % SWEEP_CASES


def model_rows(shapes, cols):
    rows, off = [], 0
    for n, m in shapes:
        w = wc.windowed(m, cols)
        db = wc.window_dir_bytes(n, m, cols) if w else wc.semi_dir_bytes(n, m)
        row = (int(w), db, wc.al256(db) if w else 0, wc.ckpt_bytes(n, m, cols) if w else 0, wc.workspace_bytes(n, m, cols), off)
        rows.append(row)
        off += row[4]
    return rows


def test_offsets_and_totals_equal_the_python_model(program):
    shapes = [(n, m) for n in sc.SWEEP_N for m in sc.SWEEP_M + (4096, 29903)] + [(400, 29903), (1 << 20, (1 << 21) + 5)]
    for cols in (0, 64, 128, 512, 1024, 4096):
        got = run(program, "jobs", "%d\n" % cols + "".join("%d %d\n" % s for s in shapes))
        assert got == model_rows(shapes, cols), cols
    # job counts that push the offsets of window directions and of checkpoints past 2^32
    shapes = [(1537, 100000)] * 9000 + [(400, 29903)] * 3
    got = run(program, "jobs", "1024\n" + "".join("%d %d\n" % s for s in shapes))
    assert got == model_rows(shapes, 1024) and got[-1][5] > 1 << 32 and got[-4][5] > 1 << 32
    one = model_rows([(1 << 20, (1 << 21) + 5)], 64)[0]
    assert one[3] > 1 << 32   # (one job's checkpoints alone)


def test_split_under_a_small_budget(program):
    mib = 1 << 20
    lists = [[(257, 4096)] * 8, [(400, 3000)] * 40, [(70, 300), (30, 278), (129, 322), (1537, 1000), (40, 64)] * 5,
             [(300, 400)] * 4 + [(3000, 200000)] + [(300, 400)] * 5]
    for shapes in lists:
        for cols in (0, 64, 512):
            got = run(program, "split", "%d %d\n" % (mib, cols) + "".join("%d %d\n" % s for s in shapes))
            want = wc.split([wc.job_bytes(n, m, cols) for n, m in shapes], mib)
            assert [c for _, c in got] == want and [b for b, _ in got] == [0] + list(np.cumsum(want)[:-1]), (shapes[0], cols)
    # the device test's eight 257 x 4 096 jobs: eight sub-batches as n x m directions, one in windows of 64 columns
    assert wc.split([wc.job_bytes(257, 4096, 0)] * 8, mib) == [1] * 8 and wc.split([wc.job_bytes(257, 4096, 64)] * 8, mib) == [8]
    assert wc.job_bytes(3000, 200000, 512) > mib   # (a windowed job over the budget goes alone)
