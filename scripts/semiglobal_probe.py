#!/usr/bin/env python3
"""Rates of the semiglobal kernels at the shape of BASELINE.json configs[0]: one 400-event chunk against one strand of a 29 903-event
reference, 16 384 jobs.  Three arms alternate inside one process, medians over the rounds:

  semiglobal   rawdtw_semiglobal_batch over the context's event arena: device time of the fill launches (rawdtw_semiglobal_timing)
  global       the SAME jobs through rawdtw_plan_* as DTW_global (k_full_wave): device time of its launches (rawdtw_plan_run_timed)
  traceback    rawdtw_semiglobal_traceback_steps on the first --tb-jobs of them: fill and walk + finish

and, where oracle/_ref exists, the reference's DTW_semiglobal on --threads host threads for scale.  Rates are cells (n x m a job) per
second of device time.  Costs of the semiglobal arm are checked against the host restatement on a few jobs.

    python scripts/semiglobal_probe.py [--jobs 16384] [--rounds 7] [--out profiles/semiglobal_probe.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rawalign_amd as ra  # noqa: E402
from rawalign_amd.dtw import JOB_DTYPE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=16384)
    ap.add_argument("--tb-jobs", type=int, default=1024)
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--m", type=int, default=29903)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-jobs", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(29903)
    ref = rng.normal(size=args.m).astype(np.float32)  # (event-level signal: normalised, no correlation from one event to the next)
    starts = rng.integers(0, args.m - args.n, args.jobs)
    ev = np.concatenate([ref[s:s + args.n] + rng.normal(0, 0.3, args.n).astype(np.float32) for s in starts]).astype(np.float32)
    eng = ra.Engine(0)
    eng.upload_reference([ref], [ref[::-1].copy()])
    jobs = np.zeros(args.jobs, JOB_DTYPE)
    jobs["ref_off"] = eng.reference_offset(0, 1)
    jobs["read_off"] = np.arange(args.jobs, dtype=np.uint32) * args.n
    jobs["n"], jobs["m"], jobs["band_radius"] = args.n, args.m, -1
    eng.upload_events(ev)
    cells = float(args.jobs) * args.n * args.m
    tb_cells = float(args.tb_jobs) * args.n * args.m
    plan = eng.plan(jobs)
    semi_ms, glob_ms, tb_fill_ms, tb_walk_ms = [], [], [], []
    cost = end_j = None
    for r in range(args.rounds + 1):  # (round 0 warms up and is dropped)
        cost, end_j = eng.semiglobal_batch(jobs)
        s = eng.semiglobal_timing()["fill_ms"]
        g = sum(ms for _, _, ms in plan.run_timed())
        tb = eng.semiglobal_traceback(jobs[:args.tb_jobs])
        t = eng.semiglobal_timing()
        assert tb[0].tobytes() == cost[:args.tb_jobs].tobytes()
        if r:
            semi_ms.append(s); glob_ms.append(g); tb_fill_ms.append(t["fill_ms"]); tb_walk_ms.append(t["walk_ms"])
    plan.close()
    for k in range(0, args.jobs, max(1, args.jobs // 4)):
        c, ej = ra.semiglobal_host(ev[k * args.n:(k + 1) * args.n], ref)
        assert c.view(np.uint32) == cost[k].view(np.uint32) and ej == end_j[k], (k, c, cost[k], ej, end_j[k])
    found = float(np.mean(np.abs(end_j.astype(np.int64) - (starts + args.n - 1)) <= 8))
    med = lambda x: float(np.median(x))  # noqa: E731
    out = {
        "shape": {"jobs": args.jobs, "n": args.n, "m": args.m, "tb_jobs": args.tb_jobs, "rounds": args.rounds},
        "semiglobal_ms": semi_ms, "global_ms": glob_ms, "tb_fill_ms": tb_fill_ms, "tb_walk_ms": tb_walk_ms,
        "semiglobal_tcups": cells / med(semi_ms) * 1e-9, "global_tcups": cells / med(glob_ms) * 1e-9,
        "semiglobal_over_global": med(glob_ms) / med(semi_ms),
        "tb_fill_tcups": tb_cells / med(tb_fill_ms) * 1e-9, "tb_tcups": tb_cells / (med(tb_fill_ms) + med(tb_walk_ms)) * 1e-9,
        "chunks_placed_within_8_events": found,
    }
    from tests.semiglobal_cases import RefSemiglobal  # noqa: E402

    if RefSemiglobal.available():
        rs = RefSemiglobal()
        todo = [ev[k * args.n:(k + 1) * args.n] for k in range(args.host_jobs)]
        with ThreadPoolExecutor(args.threads) as pool:
            t0 = time.perf_counter()
            got = list(pool.map(lambda a: rs.semiglobal(a, ref), todo))
            dt = time.perf_counter() - t0
        assert all(np.float32(g).view(np.uint32) == cost[k].view(np.uint32) for k, g in enumerate(got))
        out["reference_host"] = {"threads": args.threads, "jobs": args.host_jobs, "seconds": dt,
                                 "gcups": args.host_jobs * args.n * args.m / dt * 1e-9}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
