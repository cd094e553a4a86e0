"""Planted paths without a device (tests/planted_path_cases.py): the construction does what it says -- the cells of distance 0 are the
planted path, and the host restatements, the numpy models and the oracle return exactly that path -- and the banded case list reaches
what it was written to reach: by the model of k_band_tb_walk's window, a code is read from every chunk of a 3-, 5-, 17- and 65-chunk
band, from slot 0 and slot K - 1, through window loads at the band's first and last chunk and after a low-side drift reload.

These are conditions on the INPUTS of tests/test_planted_paths_gpu.py; the window model is compared with no device result."""
import numpy as np
import pytest

import rawalign_amd as ra
from oracle.loader import Oracle
from tests import banded_tb_cases as bc
from tests import planted_path_cases as pc
from tests import semiglobal_cases as sc
from tests import semiglobal_span_cases as sp


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def windows():
    """[(name, n, m, window model of the planted path)] in banded_list's order"""
    out = []
    for name, mv, R, holds, ex in pc.banded_list():
        i, j = pc.path_of(mv)
        out.append((name, int(i[-1]) + 1, int(j[-1]) + 1, pc.walk_window(int(i[-1]) + 1, int(j[-1]) + 1, R, i, j)))
    return out


def zero_cells(a, b):
    """the number of cells (i, j) with a[i] == b[j]"""
    la, ca = np.unique(a, return_counts=True)
    lb, cb = np.unique(b, return_counts=True)
    _, ia, ib = np.intersect1d(la, lb, return_indices=True)
    return int((ca[ia].astype(np.int64) * cb[ib]).sum())


def test_generator():
    assert pc.moves("D2 V3 D H2") == "DDVVVDHH" and pc.transposed("DVDH") == "DHDV"
    a, b = pc.planted("DVVDHD")
    assert a.tolist() == [0, 3, 3, 3, 6, 9] and b.tolist() == [0, 3, 6, 6, 9] and a.dtype == b.dtype == np.float32
    i, j = pc.path_of("DVVDHD")
    assert i.tolist() == [0, 1, 2, 3, 4, 4, 5] and j.tolist() == [0, 1, 1, 1, 2, 3, 4]
    assert np.array_equal(np.argwhere(a[:, None] == b[None, :]), np.stack([i, j], 1))   # the cells of distance 0 ARE the path
    with pytest.raises(AssertionError):
        pc.planted("DVHD")
    every = [mv for _, mv, _, _, _ in pc.banded_list()] + list(pc.GLOBAL.values()) + list(pc.SEMI.values())
    for mv in every:
        a, b = pc.planted(mv)
        i, j = pc.path_of(mv)
        assert pc.separated(mv) and len(a) == i[-1] + 1 and len(b) == j[-1] + 1
        assert not np.any(a[i] != b[j]) and zero_cells(a, b) == len(i) == len(mv) + 1


def test_shapes_and_slots_of_the_banded_list(windows):
    """(n, m, K, chunks, first slot, last slot) of every case as given, (a, b); the transpose of a square job mirrors the slots"""
    want = {"three_chunks": (561, 561, 151, 3, 5, 145), "five_chunks": (861, 861, 301, 5, 5, 295), "slot_0": (919, 919, 151, 3, 0, 149),
            "slot_k_1": (920, 920, 151, 3, 0, 150), "both_edges": (921, 921, 151, 3, 0, 150), "one_chunk": (401, 401, 64, 1, 2, 62),
            "two_chunks": (401, 401, 65, 2, 2, 62), "two_chunks_high": (405, 405, 65, 2, 2, 64), "past_1024": (2721, 2721, 1031, 17, 15, 1025),
            "past_4096": (8795, 8795, 4101, 65, 50, 4097), "slant": (1205, 405, 501, 8, 250, 326)}
    for (name, n, m, w), (_, _, _, holds, _) in list(zip(windows, pc.banded_list()))[::2]:
        assert w["inside"] == holds, name
        if holds:
            assert (n, m, w["K"], w["chunks"], w["slot_min"], w["slot_max"]) == want[name], (name, w)
    assert max(w["K"] for _, _, _, w in windows) <= bc.MAX_K
    assert len(windows) == 2 * len(pc.BANDED) and [ex for *_, ex in pc.banded_list()] == [0, 1] * len(pc.BANDED)


def test_the_list_reaches_every_branch_of_the_window(windows):
    by = {}
    for name, n, m, w in windows:
        by.setdefault(name, []).append(w)
    for name in pc.EVERY_CHUNK:   # a code is read from every chunk of the band
        assert by[name][0]["chunks_read"] == set(range(by[name][0]["chunks"])), (name, by[name][0]["chunks_read"])
    assert {by[name][0]["chunks"] for name in pc.EVERY_CHUNK} == {3, 5, 17, 65}
    assert by["two_chunks_high"][0]["slot_max"] >= 64 and by["two_chunks_high"][0]["chunks_read"] == {0, 1}
    inside = [w for _, _, _, w in windows if w["inside"]]
    wide = [w for w in inside if w["chunks"] >= 3]
    assert sum(w["loads_first"] for w in wide) >= 1     # x < 32 -> row_c = 0, on a band of several chunks
    assert sum(w["loads_last"] for w in wide) >= 1      # row_c + 1 == chunks: the second chunk is read as zeros
    assert sum(w["second"] for w in wide) >= 1000       # codes out of the window's second chunk
    assert sum(w["drift_low"] for w in by["slant"]) == 2 and all(w["loads"] >= 3 for w in inside)
    assert sum(w["drift_high"] for _, _, _, w in windows) == 0   # (cannot happen: see planted_path_cases)
    assert any(w["slot_min"] == 0 for w in wide) and any(w["slot_max"] == w["K"] - 1 for w in wide)
    for w in by["both_edges"]:
        assert (w["slot_min"], w["slot_max"]) == (0, w["K"] - 1)
    for w in by["outside"]:
        assert not w["inside"]


def test_host_restatement_returns_the_planted_path(orc):
    cases, paths = pc.banded_jobs()
    held = 0
    for (name, mv, R, holds, ex), (a, b, _, _), path, r in zip(pc.banded_list(), cases, paths, pc.banded_host_answers()):
        key = (name, len(a), len(b), R, ex)
        assert bc.bits(r.cost)[0] == bc.bits(orc.dtw_banded(a, b, R, ex))[0], key
        if holds:
            wi, wj = pc.expected(path, ex)
            assert bc.bits(r.cost)[0] == 0 and np.array_equal(r.i, wi) and np.array_equal(r.j, wj), key
            assert not r.difference.any(), key
        else:   # the band cuts the planted path: another path, through cells of distance 3 and more
            assert r.cost >= pc.STEP and len(r.i) >= max(len(a), len(b)) - ex, key
            assert not (np.array_equal(r.i, pc.expected(path, ex)[0]) and np.array_equal(r.j, pc.expected(path, ex)[1])), key
            w = pc.walk_window(len(a), len(b), R, *((r.i, r.j) if not ex else (np.append(r.i, len(a) - 1), np.append(r.j, len(b) - 1))))
            assert w["inside"] and {w["slot_min"], w["slot_max"]} & {0, w["K"] - 1}, key   # (it runs along the band's edge)
        if len(a) * len(b) <= pc.MODEL_CELLS:
            held += 1
            w = bc.model(orc, a, b, R, ex)
            assert bc.bits(r.cost)[0] == bc.bits(w["cost"])[0] and np.array_equal(r.i, w["i"]) and np.array_equal(r.j, w["j"]), key
            assert np.array_equal(bc.bits(r.difference), bc.bits(w["d"])) and not w["tie"], key
    assert held == len(cases) - 4


def test_global_planted_paths(orc):
    cases, paths = pc.global_jobs()
    assert sorted((len(a), len(b)) for a, b, _ in cases) == [(513, 913), (913, 513), (1025, 1425), (1425, 1025)]
    for (a, b, ex), path in zip(cases, paths):
        c, pi, pj, pd = orc.dtw_global_tb(a, b, ex)
        wi, wj = pc.expected(path, ex)
        assert bc.bits(c)[0] == 0 and np.array_equal(pi, wi) and np.array_equal(pj, wj) and not pd.any(), (len(a), len(b), ex)
    for mv in pc.GLOBAL.values():   # (the runs lie where the comments say)
        for mvo in (mv, pc.transposed(mv)):
            i, j = pc.path_of(mvo)
            rows_of_v_runs = i[1:][np.frombuffer(mvo.encode(), np.uint8) == ord("V")]
            assert len(rows_of_v_runs) in (300, 700) and (len(rows_of_v_runs) == 300 or rows_of_v_runs[0] < 512 < rows_of_v_runs[-1])


def test_semiglobal_planted_paths():
    """the host restatements give the constructed answers on every job: the planted path shifted by the offset, span (0, offset,
    offset + len(planted b) - 1).  The numpy models (a Python loop over every cell, seconds a job of this size) are held on one."""
    cases, plants = pc.semiglobal_jobs()
    assert len(cases) == 2 * len(pc.SEMI_OFFSETS) and all(len(b) == pc.SEMI_M and len(a) > 1024 for a, b, _ in cases)
    for k, ((a, b, ex), (off, path)) in enumerate(zip(cases, plants)):
        r, ej = ra.semiglobal_host(a, b, ex, traceback=True)
        wi, wj = pc.expected(path, ex)
        assert sc.bits(r.cost)[0] == 0 and ej == off + int(path[1][-1]), (k, off)
        assert np.array_equal(r.i, wi) and np.array_equal(r.j, wj + np.uint32(off)) and not r.difference.any(), (k, off)
        c, j0, ej = ra.semiglobal_span_host(a, b, ex)
        assert (int(sc.bits(c)[0]), j0, ej) == (0, off, off + int(path[1][-1])), (k, off)
    k = pc.SEMI_OFFSETS.index(65)
    (a, b, ex), (off, path) = cases[k], plants[k]
    c, ej, pi, pj, pd = sc.model(a, b, ex)
    wi, wj = pc.expected(path, ex)
    assert sc.bits(c)[0] == 0 and ej == off + int(path[1][-1]) and np.array_equal(pi, wi) and np.array_equal(pj, wj + np.uint32(off))
    c, j0, ej = sp.forward_model(a, b, ex)
    assert (int(sc.bits(c)[0]), j0, ej) == (0, off, off + int(path[1][-1]))
    for mv in pc.SEMI.values():   # V runs over rows 512 and 1024, an H run of 200 in a row of the middle strip; D first and last
        i, j = pc.path_of(mv)
        code = np.frombuffer(mv.encode(), np.uint8)
        runs = [(int(i[s]), int(i[e])) for s, e in _runs(code, ord("V"))]
        assert any(lo < 512 < hi for lo, hi in runs) and any(lo < 1024 < hi for lo, hi in runs), runs
        assert [e - s for s, e in _runs(code, ord("H"))] == [200] and all(512 <= i[s] < 1024 for s, e in _runs(code, ord("H")))
        assert mv[0] == mv[-1] == "D"


def _runs(code, letter):
    """[(s, e)]: the path elements s .. e span a maximal run of `letter` moves (element k + 1 follows move k)"""
    hit = np.concatenate([[False], code == letter, [False]])
    edge = np.flatnonzero(hit[1:] != hit[:-1])
    return list(zip(edge[::2].tolist(), edge[1::2].tolist()))
