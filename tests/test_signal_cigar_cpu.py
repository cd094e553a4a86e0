"""rawdtw_traceback_arena_steps, rawdtw_events_fetch and rawdtw_mapper_read_events (include/rawdtw.h) without a device: the symbols and
their signatures, null handles, the header as C99, and a scorer-hook mapper without a context serving a read's events from the host's copy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from rawalign_amd import mapper
from rawalign_amd._lib import SYMBOLS, load_library
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex
from tests import map_ref_cases as mc
from tests.test_mapper_cpu import _oracle_scorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, RANGE = 1, 4
VP, U64, U32, I32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
# the declared signatures, written out from the header's C types
DECLARED = {
    "rawdtw_traceback_arena_steps": (
        "rawdtw_ctx *ctx, const rawdtw_job_t *jobs, uint64_t n_jobs, float *out_cost, const uint64_t *path_off, uint32_t *path_len, "
        "uint8_t *path_step, float *path_d", [VP, VP, U64, VP, VP, VP, VP, VP]),
    "rawdtw_events_fetch": (
        "rawdtw_ctx *ctx, uint32_t n_segments, const uint32_t *seg_start, const uint32_t *seg_len, uint64_t *out_off, float *out, "
        "uint64_t out_cap", [VP, U32, VP, VP, VP, VP, U64]),
    "rawdtw_mapper_read_events": ("rawdtw_mapper *m, uint32_t read_id, float *out, uint32_t cap, uint32_t *n", [VP, U32, VP, U32, VP]),
}


def _norm(s):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", s, flags=re.S)).replace("( ", "(").replace(" )", ")").replace(" ,", ",").strip()


def test_the_three_entries_exist_with_the_declared_signatures():
    lib = load_library()
    header = _norm(open(os.path.join(ROOT, "include", "rawdtw.h")).read())
    for name, (params, argtypes) in DECLARED.items():
        assert hasattr(lib, name), name
        assert "int %s(%s);" % (name, _norm(params)) in header, name
        res, args = SYMBOLS[name]
        assert res is I32 and args == argtypes, name
    assert lib.rawdtw_abi_version() == 2


def test_null_handles_are_refused_not_dereferenced():
    lib = load_library()
    off = np.full(3, 7, np.uint64)
    out = np.full(4, 7.0, np.float32)
    seg = np.zeros(2, np.uint32)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert lib.rawdtw_traceback_arena_steps(None, None, 0, None, None, None, None, None) == INVALID
    assert lib.rawdtw_traceback_arena_steps(None, vp(out), 1, vp(out), vp(off), vp(seg), vp(out), vp(out)) == INVALID
    assert lib.rawdtw_events_fetch(None, 0, None, None, None, None, 0) == INVALID
    assert lib.rawdtw_events_fetch(None, 2, vp(seg), vp(seg), vp(off), vp(out), 4) == INVALID
    assert np.all(off == 7) and np.all(out == 7.0)
    n = C.c_uint32(7)
    assert lib.rawdtw_mapper_read_events(None, 0, vp(out), 4, C.byref(n)) == INVALID and n.value == 7
    assert lib.rawdtw_mapper_read_events(None, 0, None, 0, None) == INVALID
    x = C.c_int64(7)
    assert lib.rawdtw_get_option(None, b"signal_cigar", C.byref(x)) == INVALID and x.value == 7
    assert lib.rawdtw_set_option(None, b"signal_cigar", 1) == INVALID


def test_the_header_still_compiles_as_c99():
    subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "abi", "c99_include.c")], check=True)


def test_a_scorer_hook_mapper_without_a_context_serves_read_events_from_the_hosts_copy(oracle):
    ref = mc.make_reference()
    six = SeedIndex.from_signals(ref.forward, ref.reverse, threads=3)
    fx = mc.Fixture(ref=ref)
    opt, copt = mc.project_opts("default", 0)
    reads = list(range(0, fx.n_reads, 2))
    cm = mapper.CMapper(None, opt, StopOpt(), ["seq%d" % s for s in range(len(fx.lens))], [int(x) for x in fx.lens], slot_events=2048,
                        max_reads=fx.n_reads + 1, chain_opt=copt, output_chains=True, threads=2)
    cm.set_scorer(_oracle_scorer(oracle, ref, opt))
    lib = cm.lib
    ids = [cm.add_read("read_%d" % r, fx.n_chunks(r) * 4000, fx.n_chunks(r)) for r in reads]
    n = C.c_uint32(7)
    assert lib.rawdtw_mapper_read_events(cm._h, ids[0], None, 0, C.byref(n)) == 0 and n.value == 0      # no round yet
    assert all(len(cm.read_events(i)) == 0 for i in ids)
    assert lib.rawdtw_mapper_read_events(cm._h, len(ids), None, 0, C.byref(n)) == INVALID and n.value == 0   # an unknown read
    fed = {r: [] for r in reads}
    for rnd in range(2):
        act = [(i, r) for i, r in zip(ids, reads) if not cm.state(i)[0] and cm.state(i)[1] < fx.n_chunks(r)]
        assert act
        chunks = [fx.chunk(r, cm.state(i)[1]) for i, r in act]
        for (_, r), (ev, _) in zip(act, chunks):
            fed[r].append(np.asarray(ev, np.float32))
        cm.round([i for i, _ in act], chunks, seed_index=six)
    assert sum(len(v) for v in fed.values()) > len(reads)   # (some read was fed two chunks)
    for i, r in zip(ids, reads):
        want = np.concatenate(fed[r])
        got = cm.read_events(i)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), r
        # *n is written whatever the room; too little room: RAWDTW_ERR_RANGE, out untouched
        out = np.full(len(want) + 1, 7.0, np.float32)
        n = C.c_uint32(0)
        assert lib.rawdtw_mapper_read_events(cm._h, i, C.c_void_p(out.ctypes.data), len(want) - 1, C.byref(n)) == RANGE
        assert n.value == len(want) and np.all(out == 7.0)
        assert lib.rawdtw_mapper_read_events(cm._h, i, None, len(want), C.byref(n)) == INVALID and n.value == len(want)
        assert lib.rawdtw_mapper_read_events(cm._h, i, C.c_void_p(out.ctypes.data), len(want), None) == INVALID
    assert cm.signal_stats()["event_bytes_crossed"] == 0
    cm.close()
