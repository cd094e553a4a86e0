#!/usr/bin/env python3
"""Two measurements of the local border constraint (include/rawdtw.h, "local border") on one GPU, written as one JSON file
(profiles/local_probe.json):

  (a) scoring: the synthetic 16 384-read candidate batch of bench.py (same reference, same generator and seed) scored as local, as
      global + full and as global + banded -- three batches on one context, one untimed run each, then 7 rounds that alternate the three;
      a round's time is a host clock around one run and the wait for the stream.  Medians, and local / global-full.
  (b) device arrays: create + first run + fetch of the same local batch handed over in device memory (rawdtw_batch_submit_device), with
      the job records written on the device (k_local_jobs) and with the anchors brought home (RAWDTW_LOCAL_JOBS=host when the context is
      created) -- two contexts on one shared reference, 7 alternating rounds after one untimed round each; medians, the host path's spread
      (max - min) and the bytes that crossed the link either way.  k_local_jobs is the default for device arrays only if its median is
      below the host path's by more than that spread.

    python scripts/local_probe.py [--reads 16384] [--out profiles/local_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra  # noqa: E402
from rawalign_amd import synth  # noqa: E402

SEED = 20231005 + 2   # bench.py's
REPS = 7
MODES = {"local": dict(dtw_border_constraint=2), "global_full": dict(dtw_border_constraint=0, dtw_fill_method=0),
         "global_banded": dict(dtw_border_constraint=0, dtw_fill_method=1)}


def timed(fn, sync):
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=16384)
    ap.add_argument("--genome", type=int, default=4_600_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_probe.json"))
    args = ap.parse_args()
    ref = synth.make_reference([args.genome], seed=SEED)
    eng = ra.Engine(0)
    eng.upload_reference(ref.forward, ref.reverse)
    eng.set_border_local(True)
    offs = {(0, st): eng.reference_offset(0, st) for st in (0, 1)}
    cb, info = synth.make_candidate_batch(ref, offs, synth.SynthParams(n_reads=args.reads), seed=SEED)
    eng.upload_events(cb.events)
    out = {"reads": cb.n_reads, "chains": cb.n_chains, "anchors": int(len(cb.anchors)), "events": int(len(cb.events)), "reps": REPS}

    # ---- (a) ----
    batches, a = {}, {}
    for name, kw in MODES.items():
        b = batches[name] = ra.Batch(eng, ra.MapOpt(**kw), cb)
        inf = b.info()
        a[name] = {"jobs": inf["n_jobs"], "cells": inf["cells"], "launches": inf["n_launches"], "ms": []}
        b.run()
        eng.sync()
    for _ in range(REPS):
        for name, b in batches.items():
            a[name]["ms"].append(timed(b.run, eng.sync))
    for name, d in a.items():
        d["median_ms"] = statistics.median(d["ms"])
        d["spread_ms"] = max(d["ms"]) - min(d["ms"])
        d["GCUPS"] = d["cells"] / d["median_ms"] / 1e6
    costs = {name: b.fetch(with_job_costs=True)[2] for name, b in batches.items()}
    a["local_over_global_full"] = a["local"]["median_ms"] / a["global_full"]["median_ms"]
    a["local_le_global_full_everywhere"] = bool((costs["local"] <= costs["global_full"]).all())
    a["local_strictly_below_share"] = float((costs["local"] < costs["global_full"]).mean())
    for b in batches.values():
        b.close()
    out["scoring"] = a

    # ---- (b) ----
    dev = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to("cuda:0") for x in (cb.anchors, cb.ref_base, cb.read_base)]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in dev]
    engines = {}
    for path in ("device", "host"):
        if path == "host":
            os.environ["RAWDTW_LOCAL_JOBS"] = "host"   # (read when a context is created)
        e = engines[path] = ra.Engine(0)
        os.environ.pop("RAWDTW_LOCAL_JOBS", None)
        e._check(e.lib.rawdtw_share_reference(e._ctx, eng._ctx))
        e.set_border_local(True)
        e.upload_events(cb.events)
    opt = ra.MapOpt(**MODES["local"])
    b_, got = {p: {"ms": []} for p in engines}, {}

    def one(path):
        e = engines[path]
        t0 = time.perf_counter()
        bt = ra.Batch(e, opt, cb, device_ptrs=ptrs)
        got[path] = bt.fetch(with_job_costs=True)
        ms = (time.perf_counter() - t0) * 1e3
        b_[path].update(bt.hand_over_stats())
        bt.close()
        return ms

    for path in engines:
        one(path)
    for _ in range(REPS):
        for path in engines:
            b_[path]["ms"].append(one(path))
    for d in b_.values():
        d["median_ms"] = statistics.median(d["ms"])
        d["spread_ms"] = max(d["ms"]) - min(d["ms"])
    same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got["device"], got["host"]))
    same = same and np.array_equal(got["device"][2].view(np.uint32), costs["local"].view(np.uint32))
    b_["results_identical"] = bool(same)
    b_["device_is_default_by_the_rule"] = bool(b_["device"]["median_ms"] < b_["host"]["median_ms"] - b_["host"]["spread_ms"])
    out["device_arrays"] = b_
    for e in engines.values():
        e.close()
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"scoring": {k: (round(v["median_ms"], 3), round(v["spread_ms"], 3)) for k, v in a.items() if isinstance(v, dict)},
                      "local_over_global_full": round(a["local_over_global_full"], 4),
                      "device_arrays": {k: (round(v["median_ms"], 3), round(v["spread_ms"], 3)) for k, v in b_.items() if isinstance(v, dict)},
                      "device_is_default_by_the_rule": b_["device_is_default_by_the_rule"], "results_identical": same}))


if __name__ == "__main__":
    main()
