"""The traceback's sub-batch pipeline (rawdtw_tb_driver.cpp: tb_run) with more than one sub-batch, and the walk
kernel's edges, against oracle.dtw_global_tb bit for bit: the cost bits, i, j, the distance bits and the length, with
exclude_last's pop.  The budget is lowered with the context option "tb_workspace_mb"; "tb_sub_batches" must then equal what the
plain-Python model of the split (tests/traceback_cases.py) says.  The lists and what they are there for: traceback_cases.py."""
import ctypes as C

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch

    torch.cuda.is_available()
except Exception:  # pragma: no cover - torch is optional for these tests
    torch = None

import rawalign_amd as ra
from tests import traceback_cases as tc
from tests.golden_util import bits
from tests.util import OracleScorer, assert_bits_equal, make_arena_jobs, oracle_costs

pytestmark = pytest.mark.gpu

CANARY = 0xEE
_arenas = {}


@pytest.fixture(scope="module")
def engine():
    eng = ra.Engine(0)
    yield eng
    eng.close()


def vp(x):
    return C.c_void_p(x.ctypes.data)


def load(engine, name):
    """the list's arenas on the context; its jobs with the reference's offset"""
    if name not in _arenas:
        _arenas[name] = make_arena_jobs(tc.CASES[name]())
    jobs, ev, rf = _arenas[name]
    engine.upload_reference([rf], [rf])
    jobs = jobs.copy()
    jobs["ref_off"] += engine.reference_offset(0, 1)
    return jobs, ev


def n_subs(name, mb):
    return len(tc.split(tc.shapes_of(tc.CASES[name]()), mb * tc.MIB if mb else tc.DEFAULT_BUDGET))


def canaries(n, dtype):
    a = np.empty(max(n, 1), dtype)
    a.view(np.uint8)[:] = CANARY
    return a


def untouched(*arrays):
    return all(np.all(a.view(np.uint8) == CANARY) for a in arrays)


def call_ij(engine, jobs, ev):
    """rawdtw_traceback_batch into arrays of canaries: (status, cost, off, plen, pi, pj, pd)"""
    caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
    off = np.zeros(len(jobs) + 1, np.uint64)
    np.cumsum(caps, out=off[1:])
    total = int(off[-1])
    cost, plen = canaries(len(jobs), np.float32), canaries(len(jobs), np.uint32)
    pi, pj, pd = canaries(total, np.uint32), canaries(total, np.uint32), canaries(total, np.float32)
    st = engine.lib.rawdtw_traceback_batch(engine._ctx, vp(jobs), len(jobs), vp(ev), len(ev), vp(cost), vp(off), vp(plen), vp(pi), vp(pj), vp(pd))
    return st, cost, off, plen, pi, pj, pd


def assert_ij_equal_oracle(res, want, what):
    st, cost, off, plen, pi, pj, pd = res
    assert st == 0, what
    for k, (c, wi, wj, wd) in enumerate(want):
        s, n = int(off[k]), int(plen[k])
        assert n == len(wi), (what, k, n, len(wi))
        assert bits(cost[k]) == bits(c), (what, k)
        assert np.array_equal(pi[s:s + n], wi) and np.array_equal(pj[s:s + n], wj), (what, k)
        assert np.array_equal(pd[s:s + n].view(np.uint32), wd.view(np.uint32)), (what, k)


def traceback_equals_oracle(engine, oracle, name, mb):
    """one rawdtw_traceback_batch of the list at a budget of mb MiB (0: the default): right, and split as modelled"""
    engine.set_option("tb_workspace_mb", mb)
    jobs, ev = load(engine, name)
    res = call_ij(engine, jobs, ev)
    assert_ij_equal_oracle(res, tc.oracle_paths(oracle, name), f"{name} at {mb} MiB")
    assert engine.get_option("tb_sub_batches") == n_subs(name, mb), (name, mb)
    return res


def test_the_options_read_back_and_start_at_zero():
    eng = ra.Engine(0)
    assert eng.get_option("tb_workspace_mb") == 0 and eng.get_option("tb_sub_batches") == 0
    eng.set_option("tb_workspace_mb", 3)
    assert eng.get_option("tb_workspace_mb") == 3 and eng.get_option("tb_sub_batches") == 0
    with pytest.raises(ra.RawDTWError):
        eng.set_option("tb_sub_batches", 1)  # read-only
    eng.close()


def test_pipe_in_thirteen_sub_batches_equals_oracle_and_the_unsplit_call(engine, oracle):
    """Both slots of the path buffers and of the landing zone, finish(subs[k - 2]) before a slot is reused, sb.begin:
    everything a batch of one sub-batch never runs."""
    assert n_subs("pipe", 1) >= 6
    split = traceback_equals_oracle(engine, oracle, "pipe", 1)
    whole = traceback_equals_oracle(engine, oracle, "pipe", 0)
    assert engine.get_option("tb_sub_batches") == 1
    for a, b in zip(split[1:], whole[1:]):
        assert a.tobytes() == b.tobytes()   # (identical arrays, the cells behind a popped element included)


def test_variable_lowers_the_budget_and_the_option_goes_first(engine, oracle, monkeypatch):
    """RAWDTW_TB_WORKSPACE_MB is read at every call; a non-zero option takes precedence over it."""
    jobs, ev = load(engine, "pipe")
    want = tc.oracle_paths(oracle, "pipe")
    monkeypatch.setenv("RAWDTW_TB_WORKSPACE_MB", "2")
    engine.set_option("tb_workspace_mb", 0)
    assert_ij_equal_oracle(call_ij(engine, jobs, ev), want, "pipe, variable at 2")
    assert engine.get_option("tb_sub_batches") == n_subs("pipe", 2) != n_subs("pipe", 1)
    engine.set_option("tb_workspace_mb", 1)
    assert_ij_equal_oracle(call_ij(engine, jobs, ev), want, "pipe, variable at 2 and option at 1")
    assert engine.get_option("tb_sub_batches") == n_subs("pipe", 1)
    monkeypatch.delenv("RAWDTW_TB_WORKSPACE_MB")
    engine.set_option("tb_workspace_mb", 0)
    assert call_ij(engine, jobs, ev)[0] == 0 and engine.get_option("tb_sub_batches") == 1


def _layouts(jobs, subs):
    """(name, offsets, page-locked) of the steps form's layouts: dense, dense in page-locked arrays, gaps of 7, and dense
    with ONE gap, at a sub-batch boundary -- every sub-batch is then a dense stretch, and the later ones' stretches start
    (sb.lo) beyond the sum of the paths before them -- pageable and page-locked"""
    caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
    dense = np.zeros(len(jobs), np.uint64)
    dense[1:] = np.cumsum(caps)[:-1]
    gaps = np.zeros(len(jobs), np.uint64)
    gaps[1:] = np.cumsum(caps + np.uint64(7))[:-1]
    cut = dense.copy()
    first = subs[len(subs) // 2][0]          # a boundary in the middle of the call
    assert 0 < first < len(jobs)
    cut[first:] += np.uint64(5)
    return caps, (("dense", dense, False), ("dense, page-locked", dense, True), ("gaps of 7", gaps, False),
                  ("gap at a sub-batch boundary", cut, False), ("gap at a sub-batch boundary, page-locked", cut, True))


def test_pipe_steps_form_in_every_layout(engine, oracle):
    """rawdtw_traceback_batch_steps over 13 sub-batches: the dense stretches with their own base sb.lo (through the landing
    zone's two slots, and straight into page-locked arrays at path_step + sb.lo), and job by job where there are gaps.  The
    steps expand to the oracle's (i, j); nothing is written into a gap or behind the last path."""
    lib = engine.lib
    engine.set_option("tb_workspace_mb", 1)
    jobs, ev = load(engine, "pipe")
    want = tc.oracle_paths(oracle, "pipe")
    subs = tc.split(tc.shapes_of(tc.pipe_cases()), tc.MIB)
    caps, layouts = _layouts(jobs, subs)
    for what, off, pinned in layouts:
        total = int(off[-1] + caps[-1]) + 8
        ptrs = []
        if pinned:
            def alloc(nbytes):
                p = C.c_void_p()
                assert lib.rawdtw_host_alloc(nbytes, C.byref(p)) == 0
                ptrs.append(p)
                return p
            step = np.frombuffer((C.c_char * total).from_address(alloc(total).value), np.uint8, total)
            dist = np.frombuffer((C.c_char * (4 * total)).from_address(alloc(4 * total).value), np.float32, total)
        else:
            step, dist = np.zeros(total, np.uint8), np.zeros(total, np.float32)
        step[:] = CANARY
        dist.view(np.uint8)[:] = CANARY
        cost, plen = canaries(len(jobs), np.float32), canaries(len(jobs), np.uint32)
        st = lib.rawdtw_traceback_batch_steps(engine._ctx, vp(jobs), len(jobs), vp(ev), len(ev), vp(cost), vp(off), vp(plen), vp(step), vp(dist))
        assert st == 0, what
        assert engine.get_option("tb_sub_batches") == len(subs), what
        covered = np.zeros(total, bool)
        for k, (c, wi, wj, wd) in enumerate(want):
            s, n = int(off[k]), int(plen[k])
            covered[s:s + int(caps[k])] = True
            assert n == len(wi) and bits(cost[k]) == bits(c), (what, k)
            mv = step[s:s + n]
            assert mv[0] == 0 and np.all(mv <= 3), (what, k)
            assert np.array_equal(np.cumsum(mv & 1), wi) and np.array_equal(np.cumsum(mv >> 1), wj), (what, k)
            assert np.array_equal(dist[s:s + n].view(np.uint32), wd.view(np.uint32)), (what, k)
        assert not covered[-8:].any() and (covered.sum() == total - 8) == (what.startswith("dense"))
        assert np.all(step[~covered] == CANARY), what                                      # every gap, and behind the last path
        assert np.all(dist.view(np.uint8).reshape(-1, 4)[~covered] == CANARY), what
        for p in ptrs:
            lib.rawdtw_host_free(p)


def test_edge_at_the_default_budget_and_at_1_mib(engine, oracle):
    """Rows-per-lane and strip boundaries in both orientations, path lengths of every residue the walk's flushes tell apart,
    long runs along both borders: in one sub-batch, then in seven."""
    traceback_equals_oracle(engine, oracle, "edge", 0)
    assert n_subs("edge", 1) >= 6
    traceback_equals_oracle(engine, oracle, "edge", 1)


def test_big_at_the_default_budget_and_with_the_first_job_over_it(engine, oracle):
    """The benchmark's 8 192 x 8 192 job; at 16 MiB its direction buffer alone is over the budget, so it goes alone."""
    traceback_equals_oracle(engine, oracle, "big", 0)
    assert tc.split(tc.shapes_of(tc.big_cases()), 16 * tc.MIB) == [(0, 1), (1, 3)]
    traceback_equals_oracle(engine, oracle, "big", 16)


def test_refusal_in_the_last_sub_batch_writes_nothing(oracle):
    """A banded job (rmap.cpp:223-225: not implemented) in the last of 13 sub-batches: the call is refused while it plans,
    after twelve plans were built -- status 5, the split already reported, every output array as it was; the context then
    runs the unmodified list correctly."""
    eng = ra.Engine(0)
    eng.set_option("tb_workspace_mb", 1)
    jobs, ev = load(eng, "pipe")
    subs = tc.split(tc.shapes_of(tc.pipe_cases()), tc.MIB)
    bad = jobs.copy()
    k = subs[-1][0] + subs[-1][1] - 1
    bad[k]["band_radius"] = 2
    st, cost, off, plen, pi, pj, pd = call_ij(eng, bad, ev)
    assert st == 5
    assert eng.get_option("tb_sub_batches") == len(subs) >= 6
    assert untouched(cost, plen, pi, pj, pd)
    assert_ij_equal_oracle(call_ij(eng, jobs, ev), tc.oracle_paths(oracle, "pipe"), "pipe after a refusal")
    assert eng.get_option("tb_sub_batches") == len(subs)
    eng.close()


def test_one_context_through_a_sequence_of_budgets_and_sizes(oracle):
    """EDGE at 1 MiB, BIG at the default (every grow-only buffer regrows), PIPE at 1 MiB (the slots' offsets come from the
    regrown sizes), EDGE's jobs as full-matrix costs through rawdtw_score_batch, then PIPE once more with the option back
    at 0."""
    eng = ra.Engine(0)
    traceback_equals_oracle(eng, oracle, "edge", 1)
    traceback_equals_oracle(eng, oracle, "big", 0)
    traceback_equals_oracle(eng, oracle, "pipe", 1)
    jobs, ev = load(eng, "edge")
    _, _, rf = _arenas["edge"]
    assert_bits_equal(eng.score_batch(jobs, ev), oracle_costs(oracle, _arenas["edge"][0], ev, rf), "edge as costs")
    traceback_equals_oracle(eng, oracle, "pipe", 0)
    assert eng.get_option("tb_sub_batches") == 1
    eng.close()


def test_mappers_cigar_flow_at_1_mib(oracle):
    """--dtw-output-cigar at global + full (flag 0x2 | 0x4) with the budget at 1 MiB: the Python flow on the device (a call a
    read) and the library's mapper (rawdtw_mapper_finish: every mapped read's traceback in ONE call, here in several
    sub-batches) write the lines of the same flow on the oracle; the library's mapper also those of its run at the default
    budget."""
    from rawalign_amd import mapper, synth
    from rawalign_amd.mapping import StopOpt

    n = 64
    ref = synth.make_reference([29903], seed=20231005 + 1)
    seeds = mapper.SyntheticSeeds(ref, n, seed=3, max_chunks=4)
    opt = ra.MapOpt(dtw_border_constraint=0, dtw_fill_method=0, flag=0x2 | 0x4)
    want, rounds = mapper.map_reads(seeds, list(range(n)), OracleScorer(oracle, ref), opt)
    assert sum("\taln:s:(" in line for line in want) >= 12
    eng = ra.Engine(0)
    eng.upload_reference(ref.forward, ref.reverse)
    eng.set_option("tb_workspace_mb", 1)
    got, rounds_d = mapper.map_reads(seeds, list(range(n)), mapper.DeviceScorer(eng), opt)
    assert got == want and rounds_d == rounds
    eng.close()
    lines, subs = {}, {}
    for mb in (0, 1):
        eng = ra.Engine(0)
        eng.upload_reference(ref.forward, ref.reverse)
        eng.set_option("tb_workspace_mb", mb)
        cm = mapper.CMapper(eng, opt, StopOpt(), ["seq0"], [len(ref.forward[0])], slot_events=max(rd["n_ev"] for rd in seeds.reads) + 8,
                            max_reads=n, carry=True, threads=4, groups=1)   # (one group: the mapper's only context is eng's)
        lines[mb], _ = mapper.map_reads_c(seeds, list(range(n)), cm)
        subs[mb] = eng.get_option("tb_sub_batches")
        cm.close()
        eng.close()
    print("sub-batches of rawdtw_mapper_finish's traceback:", subs)
    assert subs[0] == 1 and subs[1] >= 3
    assert lines[1] == lines[0]
    assert lines[1] == want
