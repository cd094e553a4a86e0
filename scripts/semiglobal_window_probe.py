#!/usr/bin/env python3
"""Device time and memory of the semiglobal traceback in windows (include/rawdtw.h, "semiglobal, in windows") at the shape of
scripts/semiglobal_probe.py (BASELINE.json configs[0]): 400-event chunks against one strand of a 29 903-event reference.

Arms, alternating inside one process on one context, medians over the rounds after a warm-up round, device time from
rawdtw_semiglobal_timing and the whole call by the host's clock:

  off         rawdtw_semiglobal_traceback_steps with the setter off: n x m directions (the yardstick of both bars)
  on C        the same call with rawdtw_set_semiglobal_window(C), C = 512, 1 024, 4 096: fill is the cost form with checkpoints, walk is
              k_semi_window (refill and walk are one kernel) plus the finish
  cost        rawdtw_semiglobal_batch on the same jobs: the plain cost form, beside the on arms' fill

at every batch size of --jobs (default 1 024: one wave a SIMD, latency-bound; and 16 384, where `off` needs sub-batches).  Every on arm's
paths must be the off arm's, byte for byte.  Recorded: whole call, fill, walk, direction bytes, checkpoint bytes, the windows a job
(histogram, counted from the paths), "tb_sub_batches", and registers / LDS / scratch of the new kernels (--codegen: the rows of
scripts/kernel_codegen.py for rawdtw_semiglobal_kernels.hip).  The file is rewritten after every batch size.

    python scripts/semiglobal_window_probe.py [--jobs 1024,16384] [--rounds 7] [--out FILE]   (default: profiles/semiglobal_window_probe.json)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rawalign_amd as ra  # noqa: E402
from rawalign_amd.dtw import JOB_DTYPE  # noqa: E402


def windows_a_job(tb, n, m, C):
    """windows each path enters: positions with i > 0 whose window j // C is not the one of the position before (end first)"""
    cost, j0, off, plen, step, pd = tb
    out = np.zeros(len(cost), np.int64)
    for k in range(len(cost)):
        s = step[int(off[k]):int(off[k]) + int(plen[k])]
        i = np.cumsum(s & 1, dtype=np.int64)[::-1]
        w = ((np.cumsum(s >> 1, dtype=np.int64) + int(j0[k])) // C)[::-1]
        new = np.ones(len(w), bool)
        new[1:] = w[1:] != w[:-1]
        out[k] = int(((i > 0) & new).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="1024,16384")
    ap.add_argument("--columns", default="512,1024,4096")
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--m", type=int, default=29903)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--codegen", default=os.path.join(ROOT, "profiles", "semiglobal_window_codegen.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semiglobal_window_probe.json"), help="'' writes no file")
    args = ap.parse_args()
    batch_sizes = [int(x) for x in args.jobs.split(",")]
    columns = [int(x) for x in args.columns.split(",")]
    most = max(batch_sizes)
    rng = np.random.default_rng(29903)
    ref = rng.normal(size=args.m).astype(np.float32)  # (event-level signal: normalised, no correlation from one event to the next)
    starts = rng.integers(0, args.m - args.n, most)
    ev = np.concatenate([ref[s:s + args.n] + rng.normal(0, 0.3, args.n).astype(np.float32) for s in starts]).astype(np.float32)
    eng = ra.Engine(0)
    eng.upload_reference([ref], [ref[::-1].copy()])
    all_jobs = np.zeros(most, JOB_DTYPE)
    all_jobs["ref_off"] = eng.reference_offset(0, 1)
    all_jobs["read_off"] = np.arange(most, dtype=np.uint32) * args.n
    all_jobs["n"], all_jobs["m"], all_jobs["band_radius"] = args.n, args.m, -1
    eng.upload_events(ev)
    med = lambda x: float(np.median(x))  # noqa: E731
    out = {"shape": {"n": args.n, "m": args.m, "rounds": args.rounds, "columns": columns}, "batches": {}}
    if os.path.exists(args.codegen):
        rows = [r for r in json.load(open(args.codegen)) if r.get("new") and ("k_semi_window" in r.get("kernel", "") or "k_semi_ckpt_wave" in r.get("kernel", ""))]
        out["new_kernels"] = {r["kernel"].replace("rawdtw::", ""): {k: r["new"][k] for k in ("vgpr", "sgpr", "scratch_bytes", "lds_bytes", "occupancy")} for r in rows}
    else:
        print("note: %s is missing, the output has no new_kernels block (scripts/kernel_codegen.py writes it)" % args.codegen, file=sys.stderr)
    for n_jobs in batch_sizes:
        jobs = all_jobs[:n_jobs]
        arms = {"off": {"call_ms": [], "fill_ms": [], "walk_ms": []}, "cost": {"fill_ms": []}}
        for c in columns:
            arms["on_%d" % c] = {"call_ms": [], "fill_ms": [], "walk_ms": []}
        for r in range(args.rounds + 1):  # (round 0 warms up and is dropped)
            print("%d jobs, round %d" % (n_jobs, r), file=sys.stderr, flush=True)
            eng.set_semiglobal_window(0)
            t0 = time.perf_counter()
            off = eng.semiglobal_traceback(jobs)
            ms = (time.perf_counter() - t0) * 1e3
            t = eng.semiglobal_timing()
            if r:
                arms["off"]["call_ms"].append(ms); arms["off"]["fill_ms"].append(t["fill_ms"]); arms["off"]["walk_ms"].append(t["walk_ms"])
            arms["off"].update(direction_bytes=t["direction_bytes"], tb_sub_batches=eng.get_option("tb_sub_batches"), path_elements=t["path_elements"])
            for c in columns:
                eng.set_semiglobal_window(c)
                t0 = time.perf_counter()
                on = eng.semiglobal_traceback(jobs)
                ms = (time.perf_counter() - t0) * 1e3
                t, st = eng.semiglobal_timing(), eng.semiglobal_window_stats()
                a = arms["on_%d" % c]
                if r:
                    a["call_ms"].append(ms); a["fill_ms"].append(t["fill_ms"]); a["walk_ms"].append(t["walk_ms"])
                else:
                    for x, y in zip(off, on):
                        assert x.tobytes() == y.tobytes(), "the windowed paths are not the n x m form's"
                    per_job = windows_a_job(off, args.n, args.m, c)
                    assert int(per_job.sum()) == st["windows"] and int(per_job.max()) == st["max_windows_a_job"], (c, st)
                    a["windows_a_job_histogram"] = {str(k): int(v) for k, v in zip(*np.unique(per_job, return_counts=True))}
                a.update(direction_bytes=t["direction_bytes"], checkpoint_bytes=st["checkpoint_bytes"], windows=st["windows"],
                         max_windows_a_job=st["max_windows_a_job"], tb_sub_batches=eng.get_option("tb_sub_batches"))
                del on
            eng.set_semiglobal_window(0)
            eng.semiglobal_batch(jobs)
            if r:
                arms["cost"]["fill_ms"].append(eng.semiglobal_timing()["fill_ms"])
            del off
        cells = float(n_jobs) * args.n * args.m
        res = {"arms": arms, "median_ms": {k: {q: med(v[q]) for q in ("call_ms", "fill_ms", "walk_ms") if q in v} for k, v in arms.items()}}
        res["cost_tcups"] = cells / med(arms["cost"]["fill_ms"]) * 1e-9
        res["off_fill_tcups"] = cells / med(arms["off"]["fill_ms"]) * 1e-9
        for c in columns:
            a = arms["on_%d" % c]
            dev_on = med([f + w for f, w in zip(a["fill_ms"], a["walk_ms"])])
            dev_off = med([f + w for f, w in zip(arms["off"]["fill_ms"], arms["off"]["walk_ms"])])
            res["on_%d" % c] = {"device_ms": dev_on, "off_device_ms": dev_off, "device_speedup": dev_off / dev_on,
                                "call_speedup": med(arms["off"]["call_ms"]) / med(a["call_ms"]),
                                "fill_over_plain_cost": med(a["fill_ms"]) / med(arms["cost"]["fill_ms"]),
                                "direction_bytes_over_off": a["direction_bytes"] / arms["off"]["direction_bytes"],
                                "bar_b_on_not_slower": bool(med(a["call_ms"]) <= med(arms["off"]["call_ms"]))}
        out["batches"][str(n_jobs)] = res
        print(json.dumps({"jobs": n_jobs, "median_ms": res["median_ms"], **{k: res[k] for k in res if k.startswith("on_")}}), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
