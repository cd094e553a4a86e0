#!/usr/bin/env python
"""The banded traceback against the full-matrix traceback on the same windows: 1 024 jobs of 3 000 x 3 000, radius 300 (the default band
fraction 0.10) through rawdtw_banded_traceback_steps, and the same windows with band_radius = RAWDTW_FULL through
rawdtw_traceback_batch_steps.  The two arms alternate in one process; round 0 warms up and is dropped; medians of --rounds with their
ranges: device time of the fill, of the walk + finish, wall time of the whole call (events uploaded, paths written into the caller's
pageable arrays), direction bytes, and `bar`: whether the banded call's median is not above the full-matrix call's.  A few banded jobs are
checked against the host restatement.  Keys of an existing --out file that the script does not write (`codegen`: the kernels' registers and
LDS from -Rpass-analysis=kernel-resource-usage; notes on other runs) are kept.

    python scripts/banded_tb_probe.py [--jobs 1024] [--rounds 7] [--out profiles/banded_tb_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rawalign_amd as ra  # noqa: E402
from rawalign_amd.dtw import JOB_DTYPE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1024)
    ap.add_argument("--n", type=int, default=3000)
    ap.add_argument("--m", type=int, default=3000)
    ap.add_argument("--radius", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(3000)
    ref = rng.normal(size=max(60000, 2 * args.m)).astype(np.float32)
    starts = rng.integers(0, len(ref) - args.m, args.jobs)
    # a read's events: its stretch of the reference, stretched or squeezed to n events, with noise
    ev = np.concatenate([np.interp(np.linspace(0, args.m - 1, args.n), np.arange(args.m), ref[s:s + args.m]) + rng.normal(0, 0.3, args.n)
                         for s in starts]).astype(np.float32)
    eng = ra.Engine(0)
    eng.upload_reference([ref], [ref[::-1].copy()])
    jobs = np.zeros(args.jobs, JOB_DTYPE)
    jobs["ref_off"] = eng.reference_offset(0, 1) + starts.astype(np.uint64)
    jobs["read_off"] = np.arange(args.jobs, dtype=np.uint32) * args.n
    jobs["n"], jobs["m"], jobs["band_radius"] = args.n, args.m, args.radius
    full = jobs.copy()
    full["band_radius"] = -1
    caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
    off = np.zeros(args.jobs + 1, np.uint64)
    np.cumsum(caps, out=off[1:])
    total = int(off[-1])
    out = (np.empty(args.jobs, np.float32), np.zeros(args.jobs, np.uint32), np.zeros(total, np.uint8), np.zeros(total, np.float32))
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731

    def banded():
        t0 = time.perf_counter()
        eng.banded_traceback(jobs, ev, path_off=off, out=out)
        ms = (time.perf_counter() - t0) * 1e3
        return dict(eng.banded_traceback_timing(), call_ms=ms)

    def full_matrix():
        t0 = time.perf_counter()
        st = eng.lib.rawdtw_traceback_batch_steps(eng._ctx, vp(full), len(full), vp(ev), len(ev), vp(out[0]), vp(off), vp(out[1]), vp(out[2]), vp(out[3]))
        ms = (time.perf_counter() - t0) * 1e3
        assert st == 0, st
        f, w, d, e = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
        assert eng.lib.rawdtw_traceback_timing(eng._ctx, C.byref(f), C.byref(w), C.byref(d), C.byref(e)) == 0
        return {"fill_ms": f.value, "walk_ms": w.value, "direction_bytes": d.value, "path_elements": e.value, "call_ms": ms}

    arms = {"banded": [], "full_matrix": []}
    for r in range(args.rounds + 1):
        b = banded()
        if r == 0:
            for k in range(0, args.jobs, max(1, args.jobs // 4)):  # (the banded arm's answers, before the other arm overwrites the arrays)
                a_k, b_k = ev[k * args.n:(k + 1) * args.n], ref[starts[k]:starts[k] + args.m]
                w = ra.banded_tb_host(a_k, b_k, args.radius)
                s = int(off[k])
                i, j = ra.expand_steps(out[2][s:s + int(out[1][k])])
                assert out[0][k].view(np.uint32) == w.cost.view(np.uint32) and np.array_equal(i, w.i) and np.array_equal(j, w.j), k
        f = full_matrix()
        if r:
            arms["banded"].append(b)
            arms["full_matrix"].append(f)

    def stats(rows, key):
        x = [float(v[key]) for v in rows]
        return {"median": float(np.median(x)), "min": min(x), "max": max(x)}

    res = {"shape": {"jobs": args.jobs, "n": args.n, "m": args.m, "radius": args.radius, "rounds": args.rounds}}
    for name, rows in arms.items():
        res[name] = {k: stats(rows, k) for k in ("fill_ms", "walk_ms", "call_ms")}
        res[name]["direction_bytes"] = int(rows[0]["direction_bytes"])
        res[name]["path_elements"] = int(rows[0]["path_elements"])
    res["banded_call_over_full_matrix_call"] = res["banded"]["call_ms"]["median"] / res["full_matrix"]["call_ms"]["median"]
    res["banded_device_over_full_matrix_device"] = (res["banded"]["fill_ms"]["median"] + res["banded"]["walk_ms"]["median"]) / \
        (res["full_matrix"]["fill_ms"]["median"] + res["full_matrix"]["walk_ms"]["median"])
    res["direction_bytes_ratio"] = res["banded"]["direction_bytes"] / res["full_matrix"]["direction_bytes"]
    res["bar"] = {"rule": "the banded call's median is not above the full-matrix call's median in the same run",
                  "met": res["banded_call_over_full_matrix_call"] <= 1.0}
    print(json.dumps(res))
    if args.out:
        if os.path.exists(args.out):  # what this script does not measure stays: the kernels' registers and LDS (`codegen`), notes on other runs
            with open(args.out) as f:
                old = json.load(f)
            res.update({k: v for k, v in old.items() if k not in res})
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
