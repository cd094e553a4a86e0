#!/usr/bin/env python3
"""Device time of the semiglobal span at the shape of scripts/semiglobal_probe.py (BASELINE.json configs[0]): 400-event chunks against
one strand of a 29 903-event reference.  Three arms alternate inside one process, medians over the rounds, device time from
rawdtw_semiglobal_timing:

  span        rawdtw_semiglobal_span_batch on --jobs jobs over the context's event arena
  cost        rawdtw_semiglobal_batch on the same jobs: bar (b), the ratio is reported
  traceback   rawdtw_semiglobal_traceback_steps on the first --tb-jobs of them (fill and walk + finish), and the span on the same
              --tb-jobs jobs beside it: bar (a), the span takes less device time than fill + walk of the call it replaces

The span's (cost, end_j) must be the cost arm's and its j0 the traceback's; a few jobs are held to rawdtw_semiglobal_span_host.
--codegen: the rows of scripts/kernel_codegen.py for rawdtw_semiglobal_kernels.hip; the span instantiations' registers and waves a
SIMD go into the output beside the times.

    python scripts/semiglobal_span_probe.py [--jobs 16384] [--rounds 7] [--out FILE]     (default: profiles/semiglobal_span_probe.json)
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--codegen", default=os.path.join(ROOT, "profiles", "semiglobal_span_codegen.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semiglobal_span_probe.json"), help="'' writes no file")
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
    few = jobs[:args.tb_jobs]
    span_ms, cost_ms, span_few_ms, tb_fill_ms, tb_walk_ms = [], [], [], [], []
    span = None
    for r in range(args.rounds + 1):  # (round 0 warms up and is dropped)
        span = eng.semiglobal_span(jobs)
        s = eng.semiglobal_timing()
        assert s["walk_ms"] == 0 and s["direction_bytes"] == 0 and s["path_elements"] == 0
        cost, end_j = eng.semiglobal_batch(jobs)
        c = eng.semiglobal_timing()["fill_ms"]
        span_few = eng.semiglobal_span(few)
        sf = eng.semiglobal_timing()["fill_ms"]
        tb = eng.semiglobal_traceback(few)
        t = eng.semiglobal_timing()
        assert span[0].tobytes() == cost.tobytes() and span[2].tobytes() == end_j.tobytes()
        assert span_few[1].tobytes() == tb[1].tobytes() == span[1][:args.tb_jobs].tobytes() and span_few[0].tobytes() == tb[0].tobytes()
        if r:
            span_ms.append(s["fill_ms"]); cost_ms.append(c); span_few_ms.append(sf)
            tb_fill_ms.append(t["fill_ms"]); tb_walk_ms.append(t["walk_ms"])
    for k in range(0, args.jobs, max(1, args.jobs // 4)):
        c, j0, ej = ra.semiglobal_span_host(ev[k * args.n:(k + 1) * args.n], ref)
        assert c.view(np.uint32) == span[0][k].view(np.uint32) and (j0, ej) == (span[1][k], span[2][k]), (k, c, j0, ej)
    med = lambda x: float(np.median(x))  # noqa: E731
    cells, few_cells = float(args.jobs) * args.n * args.m, float(args.tb_jobs) * args.n * args.m
    tb_ms = [f + w for f, w in zip(tb_fill_ms, tb_walk_ms)]
    out = {
        "shape": {"jobs": args.jobs, "n": args.n, "m": args.m, "tb_jobs": args.tb_jobs, "rounds": args.rounds},
        "span_ms": span_ms, "cost_ms": cost_ms, "span_tb_jobs_ms": span_few_ms, "tb_fill_ms": tb_fill_ms, "tb_walk_ms": tb_walk_ms,
        "median_ms": {"span": med(span_ms), "cost": med(cost_ms), "span_tb_jobs": med(span_few_ms), "tb_fill": med(tb_fill_ms),
                      "tb_walk": med(tb_walk_ms), "tb_fill_plus_walk": med(tb_ms)},
        "span_tcups": cells / med(span_ms) * 1e-9, "cost_tcups": cells / med(cost_ms) * 1e-9,
        "span_tb_jobs_tcups": few_cells / med(span_few_ms) * 1e-9, "tb_tcups": few_cells / med(tb_ms) * 1e-9,
        "bar_a_span_over_traceback_time": med(span_few_ms) / med(tb_ms), "bar_a_met": bool(med(span_few_ms) < med(tb_ms)),
        "bar_b_span_over_cost_rate": med(cost_ms) / med(span_ms),
        "starts_within_8_events": float(np.mean(np.abs(span[1].astype(np.int64) - starts) <= 8)),
        "ends_within_8_events": float(np.mean(np.abs(span[2].astype(np.int64) - (starts + args.n - 1)) <= 8)),
    }
    if os.path.exists(args.codegen):
        rows = [r for r in json.load(open(args.codegen)) if "k_semi_span_wave" in r.get("kernel", "")]
        out["span_kernels"] = {r["kernel"].replace("rawdtw::", ""): {"vgpr": r["new"]["vgpr"], "sgpr": r["new"]["sgpr"],
                                                                    "waves_per_simd": r["new"]["occupancy"]} for r in rows}
    else:
        print("note: %s is missing, the output has no span_kernels block (scripts/kernel_codegen.py writes it)" % args.codegen, file=sys.stderr)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
