"""Planted paths on the device (tests/planted_path_cases.py): every path producer on inputs whose optimal path is known by construction
and runs where random and near-diagonal inputs never go.

The banded traceback (rawdtw_band_tb.hip) on paths that read a direction code from every chunk of bands of 3, 5, 17 and 65 chunks, run
along slot 0 and slot K - 1, load the walk's window at the band's first and last chunk and reload it after the slot drifted out
(tests/test_planted_paths_cpu.py shows that the list does) -- bit for bit against rawdtw_banded_tb_host, costs against the oracle, and
(i, j) against the planted path itself; unsplit, in sub-batches at "tb_workspace_mb" = 1, and through the single-call drop-in.  The
global, semiglobal and span walkers on long V and H runs across their strip edges."""
import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from oracle.loader import Oracle
from tests import banded_tb_cases as bc
from tests import planted_path_cases as pc
from tests import semiglobal_cases as sc
from tests import test_semiglobal_gpu as sg
from tests.test_banded_tb_gpu import D_CANARY, STEP_CANARY, canaried, check, engine_for
from tests.util import make_arena_jobs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def banded():
    """(cases, planted paths, host answers, the unsplit call's result)"""
    cases, paths = pc.banded_jobs()
    want = pc.banded_host_answers()
    eng, jobs, ev = engine_for(cases)
    out = canaried(jobs)
    tb = eng.banded_traceback(jobs, ev, out=out)
    assert eng.get_option("tb_sub_batches") == 1
    eng.close()
    return cases, paths, want, tb


def canaries_intact(off, plen, step, pd, count):
    for k in range(count):
        s, e = int(off[k]) + int(plen[k]), (int(off[k + 1]) if k + 1 < len(off) else len(step))
        assert (step[s:e] == STEP_CANARY).all() and (bc.bits(pd[s:e]) == bc.bits(D_CANARY)[0]).all(), k


def test_banded_list_is_the_hosts_the_oracles_and_the_planted(orc, banded):
    cases, paths, want, tb = banded
    check(cases, want, tb, "planted")
    cost, off, plen, step, pd = tb
    canaries_intact(off, plen, step, pd, len(cases))
    planted = 0
    for k, ((name, mv, R, holds, ex), (a, b, _, _), path) in enumerate(zip(pc.banded_list(), cases, paths)):
        assert bc.bits(cost[k])[0] == bc.bits(orc.dtw_banded(a, b, R, ex))[0], (name, k)
        if holds:   # the planted path itself: no yardstick in between
            planted += 1
            s = int(off[k])
            i, j = ra.expand_steps(step[s:s + int(plen[k])])
            wi, wj = pc.expected(path, ex)
            assert bc.bits(cost[k])[0] == 0 and np.array_equal(i, wi) and np.array_equal(j, wj), (name, k, len(a), len(b), R, ex)
            assert not pd[s:s + int(plen[k])].any(), (name, k)
        else:
            assert cost[k] >= pc.STEP and plen[k] > 0, (name, k)
    assert planted == len(cases) - 2


def test_banded_list_in_sub_batches_at_1_mib(banded):
    """the same list under a 1 MiB direction budget: the small jobs share sub-batches, every large one goes alone over the budget; the
    caller's layout leaves a gap behind every job"""
    cases, paths, want, whole = banded
    small, jobs, ev = engine_for(cases, tb_workspace_mb=1)
    caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
    off = np.zeros(len(jobs), np.uint64)
    off[1:] = np.cumsum(caps + (np.arange(len(jobs)) % 7).astype(np.uint64))[:-1]
    out = canaried(jobs, off)
    cost, _, plen, step, pd = small.banded_traceback(jobs, ev, path_off=off, out=out)
    cut = bc.sub_batches(jobs, 1)
    alone = sum(bc.dir_bytes(int(j["n"]), int(j["m"]), int(j["band_radius"])) > 1 << 20 for j in jobs)
    assert small.get_option("tb_sub_batches") == len(cut) >= 3 and alone >= 4 and max(cut) >= 2, (cut, alone)
    check(cases, want, (cost, off, plen, step, pd), "1 MiB")
    assert np.array_equal(bc.bits(cost), bc.bits(whole[0])) and np.array_equal(plen, whole[2])
    for k in range(len(jobs)):
        s, ln, s0 = int(off[k]), int(plen[k]), int(whole[1][k])
        assert np.array_equal(step[s:s + ln], whole[3][s0:s0 + ln]) and np.array_equal(bc.bits(pd[s:s + ln]), bc.bits(whole[4][s0:s0 + ln])), k
    canaries_intact(off, plen, step, pd, len(jobs))
    small.close()


def test_banded_single_call_drop_in():
    """the three-chunk case and the slanted one with its drift reload, both orientations, through DTW_global_banded_tb"""
    entries = [e for e in pc.banded_list() if e[0] in ("three_chunks", "slant")]
    cases, paths = pc.banded_jobs(entries)
    assert len(cases) == 4
    eng = ra.Engine(0)
    for (a, b, R, ex), path in zip(cases, paths):
        r, w = eng.DTW_global_banded_tb(a, b, R, ex), ra.banded_tb_host(a, b, R, ex)
        wi, wj = pc.expected(path, ex)
        assert bc.bits(r.cost)[0] == bc.bits(w.cost)[0] == 0 and np.array_equal(r.i, wi) and np.array_equal(r.j, wj), (len(a), len(b), R, ex)
        assert np.array_equal(r.i, w.i) and np.array_equal(r.j, w.j) and np.array_equal(bc.bits(r.difference), bc.bits(w.difference))
    eng.close()


def test_global_full_matrix(orc):
    """a V run of 700 rows over the 512-row strip edge and an H run of 300 columns, both in mid-matrix; the shorter side 513 and 1025;
    both orientations"""
    cases, paths = pc.global_jobs()
    jobs, ev, rf = make_arena_jobs([(a, b, -1, ex) for a, b, ex in cases])
    eng = ra.Engine(0)
    eng.upload_reference([rf], [rf])
    jobs["ref_off"] += eng.reference_offset(0, 1)
    res = eng.traceback_batch(jobs, ev)
    for (a, b, ex), path, r in zip(cases, paths, res):
        key = (len(a), len(b), ex)
        c, pi, pj, pdd = orc.dtw_global_tb(a, b, ex)
        wi, wj = pc.expected(path, ex)
        assert bc.bits(r.cost)[0] == bc.bits(c)[0] == 0 and np.array_equal(r.i, wi) and np.array_equal(r.j, wj), key
        assert np.array_equal(r.i, pi) and np.array_equal(r.j, pj) and np.array_equal(bc.bits(r.difference), bc.bits(pdd)), key
        one = eng.DTW_global_tb(a, b, ex)
        assert bc.bits(one.cost)[0] == 0 and np.array_equal(one.i, wi) and np.array_equal(one.j, wj), key
    eng.close()


def test_semiglobal_traceback_and_span():
    """the planted b inside noise at column 0, 63, 64, 65 and 1000 of 3 000; V runs over rows 512 and 1024 of the pipelined class, an
    H run of 200 columns in the middle strip: the path is the planted one shifted by the offset, the span (0, offset, offset +
    len(planted b) - 1); both bit for bit the host restatements' (which tests/test_planted_paths_cpu.py holds to the numpy models)"""
    cases, plants = pc.semiglobal_jobs()
    eng, jobs, ev = sg.engine_for(cases)
    tb = eng.semiglobal_traceback(jobs, ev)
    sg.check_paths(cases, sg.host_answers(cases), tb, "planted")
    cost, j0, off, plen, step, pd = tb
    scost, sj0, send = eng.semiglobal_span(jobs, ev)
    bcost, bend = eng.semiglobal_batch(jobs, ev)
    for k, ((a, b, ex), (at, path)) in enumerate(zip(cases, plants)):
        s, ln = int(off[k]), int(plen[k])
        i, j = ra.expand_steps(step[s:s + ln], int(j0[k]))
        wi, wj = pc.expected(path, ex)
        end = at + int(path[1][-1])
        assert sc.bits(cost[k])[0] == 0 and j0[k] == at and np.array_equal(i, wi) and np.array_equal(j, wj + np.uint32(at)), (k, at, ex)
        assert not pd[s:s + ln].any(), (k, at)
        assert (int(sc.bits(scost[k])[0]), int(sj0[k]), int(send[k])) == (0, at, end), (k, at, ex, scost[k], sj0[k], send[k])
        assert (int(sc.bits(bcost[k])[0]), int(bend[k])) == (0, end), (k, at, ex)
        hc, hj0, hend = ra.semiglobal_span_host(a, b, ex)
        assert (int(sc.bits(hc)[0]), hj0, hend) == (0, at, end), (k, at, ex)
