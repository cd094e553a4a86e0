#!/usr/bin/env python3
"""A worker of scripts/tb_driver_ab.py: loads the library RAWDTW_LIBRARY names, then runs one timed round of the arm named on each
line of standard input and answers with one JSON line.  The shapes and timed bodies are those of scripts/banded_tb_probe.py (both of
its arms), scripts/semiglobal_probe.py (its traceback and its cost call), scripts/local_probe.py (a), scripts/bench_modes.py --mode
traceback and scripts/aln_text_probe.py (setter off and on; and the same finish of a local and of a global + banded mapper); a probe
runs its arms in one process, and two libraries cannot share one."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: PyTorch bundles its own HIP runtime)

import bench  # noqa: E402
import rawalign_amd as ra  # noqa: E402
from rawalign_amd import mapper, synth  # noqa: E402
from rawalign_amd.dtw import JOB_DTYPE  # noqa: E402
from rawalign_amd.mapping import StopOpt  # noqa: E402

out_stream = os.fdopen(os.dup(1), "w")
os.dup2(2, 1)   # whatever else prints goes to stderr
vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
state = {}


def made(name, setup):
    """a workload, set up when its first arm runs (so an arm's warm-up is the first call on a fresh context)"""
    if name not in state:
        state[name] = setup()
    return state[name]


def getter(eng, name):
    f, w, d, e = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
    assert getattr(eng.lib, name)(eng._ctx, C.byref(f), C.byref(w), C.byref(d), C.byref(e)) == 0
    return {"fill_ms": f.value, "walk_ms": w.value, "direction_bytes": d.value, "path_elements": e.value}


def banded_setup():
    jobs_n, n, m, radius = 1024, 3000, 3000, 300
    rng = np.random.default_rng(3000)
    ref = rng.normal(size=max(60000, 2 * m)).astype(np.float32)
    starts = rng.integers(0, len(ref) - m, jobs_n)
    ev = np.concatenate([np.interp(np.linspace(0, m - 1, n), np.arange(m), ref[s:s + m]) + rng.normal(0, 0.3, n) for s in starts]).astype(np.float32)
    eng = ra.Engine(0)
    eng.upload_reference([ref], [ref[::-1].copy()])
    jobs = np.zeros(jobs_n, JOB_DTYPE)
    jobs["ref_off"] = eng.reference_offset(0, 1) + starts.astype(np.uint64)
    jobs["read_off"] = np.arange(jobs_n, dtype=np.uint32) * n
    jobs["n"], jobs["m"], jobs["band_radius"] = n, m, radius
    full = jobs.copy()
    full["band_radius"] = -1
    off = np.zeros(jobs_n + 1, np.uint64)
    np.cumsum(jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1, out=off[1:])
    total = int(off[-1])
    out = (np.empty(jobs_n, np.float32), np.zeros(jobs_n, np.uint32), np.zeros(total, np.uint8), np.zeros(total, np.float32))
    return dict(eng=eng, jobs=jobs, full=full, ev=ev, off=off, out=out)


def arm_banded():
    s = made("banded", banded_setup)
    t0 = time.perf_counter()
    s["eng"].banded_traceback(s["jobs"], s["ev"], path_off=s["off"], out=s["out"])
    ms = (time.perf_counter() - t0) * 1e3
    return dict(getter(s["eng"], "rawdtw_banded_traceback_timing"), call_ms=ms, check=int(s["out"][1].sum()))


def arm_full_steps():
    s = made("banded", banded_setup)
    eng, full, ev, off, out = s["eng"], s["full"], s["ev"], s["off"], s["out"]
    t0 = time.perf_counter()
    st = eng.lib.rawdtw_traceback_batch_steps(eng._ctx, vp(full), len(full), vp(ev), len(ev), vp(out[0]), vp(off), vp(out[1]), vp(out[2]), vp(out[3]))
    ms = (time.perf_counter() - t0) * 1e3
    assert st == 0, st
    return dict(getter(eng, "rawdtw_traceback_timing"), call_ms=ms, check=int(out[1].sum()))


def semi_setup():
    jobs_n, tb_jobs, n, m = 16384, 1024, 400, 29903
    rng = np.random.default_rng(29903)
    ref = rng.normal(size=m).astype(np.float32)
    starts = rng.integers(0, m - n, jobs_n)
    ev = np.concatenate([ref[s:s + n] + rng.normal(0, 0.3, n).astype(np.float32) for s in starts]).astype(np.float32)
    eng = ra.Engine(0)
    eng.upload_reference([ref], [ref[::-1].copy()])
    jobs = np.zeros(jobs_n, JOB_DTYPE)
    jobs["ref_off"] = eng.reference_offset(0, 1)
    jobs["read_off"] = np.arange(jobs_n, dtype=np.uint32) * n
    jobs["n"], jobs["m"], jobs["band_radius"] = n, m, -1
    eng.upload_events(ev)
    return dict(eng=eng, jobs=jobs, tb=jobs[:tb_jobs].copy())


def arm_semiglobal_tb():
    s = made("semi", semi_setup)
    t0 = time.perf_counter()
    tb = s["eng"].semiglobal_traceback(s["tb"])
    ms = (time.perf_counter() - t0) * 1e3
    return dict(getter(s["eng"], "rawdtw_semiglobal_timing"), call_ms=ms, check=int(tb[3].sum()))


def arm_semiglobal_cost():
    s = made("semi", semi_setup)
    t0 = time.perf_counter()
    cost, end_j = s["eng"].semiglobal_batch(s["jobs"])
    ms = (time.perf_counter() - t0) * 1e3
    return dict(fill_ms=s["eng"].semiglobal_timing()["fill_ms"], call_ms=ms, check=int(end_j.astype(np.uint64).sum()))


def local_setup():
    seed = 20231005 + 2
    ref = synth.make_reference([4_600_000], seed=seed)
    eng = ra.Engine(0)
    eng.upload_reference(ref.forward, ref.reverse)
    eng.set_border_local(True)
    offs = {(0, st): eng.reference_offset(0, st) for st in (0, 1)}
    cb, _ = synth.make_candidate_batch(ref, offs, synth.SynthParams(n_reads=16384), seed=seed)
    eng.upload_events(cb.events)
    return dict(eng=eng, batch=ra.Batch(eng, ra.MapOpt(dtw_border_constraint=2), cb))


def arm_local_scoring():
    s = made("local", local_setup)
    t0 = time.perf_counter()
    s["batch"].run()
    s["eng"].sync()
    return dict(call_ms=(time.perf_counter() - t0) * 1e3)


def bench_tb_setup():
    from rawalign_amd._lib import AlignOpt

    eng = ra.Engine(0)
    ref = synth.make_reference(bench.YEAST, seed=20231005 + 3)
    eng.upload_reference(ref.forward, ref.reverse)
    offs = {(s, st): eng.reference_offset(s, st) for s in range(ref.n_seq) for st in (0, 1)}
    cb, _ = synth.make_candidate_batch(ref, offs, synth.SynthParams(n_reads=1024, max_chunks=6), seed=77)
    eng.upload_events(cb.events)
    copt = AlignOpt(0, 0, 0.10, 0.4, 20.0, 1)
    firsts = [int(cb.chain_off[r]) for r in range(cb.n_reads) if cb.chain_off[r + 1] > cb.chain_off[r]]
    jobs = np.zeros(len(firsts), ra.JOB_DTYPE)
    for k, c in enumerate(firsts):
        a = cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])]
        one = np.zeros(1, ra.JOB_DTYPE)
        eng.lib.rawdtw_chain_build_jobs(C.byref(copt), vp(a), len(a), int(cb.ref_base[c]), int(cb.read_base[c]), 1, vp(one))
        jobs[k] = one[0]
    return dict(eng=eng, jobs=jobs, ev=cb.events)


def arm_bench_traceback():
    s = made("bench_tb", bench_tb_setup)
    t0 = time.perf_counter()
    res = s["eng"].traceback_batch(s["jobs"], s["ev"])
    ms = (time.perf_counter() - t0) * 1e3
    return dict(getter(s["eng"], "rawdtw_traceback_timing"), call_ms=ms, check=int(sum(len(r) for r in res)))


def finish_setup():
    n = 2048
    ref = synth.make_reference(bench.YEAST, seed=20231005 + 3)
    made = mapper.SyntheticSeeds(ref, n, seed=77, max_chunks=6)

    class Seeds:
        reads = made.reads

        def __init__(self):
            self.cache = {}

        def read_job(self, r):
            return made.read_job(r)

        def chunk(self, r, c):
            if (r, c) not in self.cache:
                self.cache[(r, c)] = made.chunk(r, c)
            return self.cache[(r, c)]

    eng = ra.Engine(0)
    eng.upload_reference(ref.forward, ref.reverse)
    eng.set_border_local(True)
    return dict(eng=eng, ref=ref, seeds=Seeds(), n=n, slot=max(rd["n_ev"] for rd in made.reads) + 8)


def finish(kind):
    """a fresh mapper through its rounds and its finish; the finish alone is timed (scripts/aln_text_probe.py's `one`)"""
    import hashlib

    s = made("finish", finish_setup)
    eng, ref, n = s["eng"], s["ref"], s["n"]
    kw = {"off": dict(dtw_border_constraint=0, dtw_fill_method=0), "on": dict(dtw_border_constraint=0, dtw_fill_method=0),
          "local": dict(dtw_border_constraint=2), "banded": dict(dtw_border_constraint=0, dtw_fill_method=1)}[kind]
    opt = ra.MapOpt(flag=ra.MapOpt().flag | 0x4, **kw)
    cm = mapper.CMapper(eng, opt, StopOpt(), [f"seq{q}" for q in range(ref.n_seq)], [len(x) for x in ref.forward], slot_events=s["slot"], max_reads=n,
                        carry=True, threads=16, groups=1)
    took, go = [], cm.finish

    def timed_finish():
        t0 = time.perf_counter()
        st = go()
        took.append((time.perf_counter() - t0) * 1e3)
        return st
    cm.finish = timed_finish
    lines, _ = mapper.map_reads_c(s["seeds"], list(range(n)), cm, device_text=kind == "on", banded_cigar=kind == "banded")
    cm.close()
    name = {"local": "rawdtw_semiglobal_timing", "banded": "rawdtw_banded_traceback_timing"}.get(kind, "rawdtw_traceback_timing")
    return dict(getter(eng, name), finish_ms=took[0], cigars=sum("\taln:s:(" in ln for ln in lines),
                check=hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16])


ARMS = {"banded": arm_banded, "full_steps": arm_full_steps, "semiglobal_tb": arm_semiglobal_tb, "semiglobal_cost": arm_semiglobal_cost,
        "local_scoring": arm_local_scoring, "bench_traceback": arm_bench_traceback,
        "finish_off": lambda: finish("off"), "finish_on": lambda: finish("on"), "finish_local": lambda: finish("local"), "finish_banded": lambda: finish("banded")}

for line in sys.stdin:
    arm = line.strip()
    if not arm:
        continue
    res = ARMS[arm]()
    out_stream.write(json.dumps(res) + "\n")
    out_stream.flush()
