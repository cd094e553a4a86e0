#!/usr/bin/env python3
"""Event detection on the device against its own input copy and the host restatement: 16 384 chunks of 4 000 samples from
synth.make_raw_reads at the default options (roptions.c:37-41).  Prints one JSON line (profiles/events_probe.json):
  kernel_ms        the five launches' device time (HIP events, rawdtw_detect_end)
  call_ms          rawdtw_detect_begin ... rawdtw_detect_end from page-locked memory, host wall time
  h2d_ms           a plain host-to-device copy of the same samples from page-locked memory, timed in the same run
  host_1t_ms, host_16t_ms   rawdtw_detect_events_host on 1 and 16 threads
each the median of --reps runs after a warm-up of at least 200 ms.  python scripts/events_probe.py [--chunks N] [--reps R]
[--no-host1] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warm_s=0.2):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t) * 1e3 if r is None else r)
    return float(np.median(out)), [round(x, 4) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=16384)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host1", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch  # (the plain copy; torch's HIP runtime initialises first, as in the tests)

    torch.cuda.init()
    import rawalign_amd as ra
    from rawalign_amd.events import PinnedArray
    from rawalign_amd.synth import make_raw_reads

    lib = ra.load_library()
    reads = make_raw_reads(a.chunks, a.samples, seed=20240601)
    n = a.chunks
    N = n * a.samples
    sig = PinnedArray(N, np.float32)
    sig.array[:] = np.concatenate(reads)
    off = PinnedArray(n + 1, np.uint64)
    off.array[:] = np.arange(n + 1, dtype=np.uint64) * np.uint64(a.samples)
    eoff, ev = PinnedArray(n + 1, np.uint64), PinnedArray(N, np.float32)
    eng = ra.Engine(0)
    ms = C.c_float()

    def call():
        st = lib.rawdtw_detect_begin(eng._ctx, None, n, off.ptr, sig.ptr, eoff.ptr, ev.ptr, N)
        st = st or lib.rawdtw_detect_end(eng._ctx, C.byref(ms))
        assert st == 0, lib.rawdtw_last_error(eng._ctx)

    call_ms, call_runs = timed(call, a.reps)

    def kernels():
        call()
        return ms.value

    kernel_ms, kernel_runs = timed(kernels, a.reps)
    n_events = int(eoff.array[n])
    # the plain copy of the same bytes from page-locked memory, in the same process
    h = torch.from_numpy(sig.array[:N])
    d = torch.empty(N, dtype=torch.float32, device="cuda:0")

    def h2d():
        d.copy_(h, non_blocking=True)
        torch.cuda.synchronize()

    h2d_ms, h2d_runs = timed(h2d, a.reps)
    # results against the host restatement (the whole batch, bit for bit)
    hs, ho = sig.array[:N], off.array[:n + 1]
    want_off, want = ra.detect_events_host(hs, ho, threads=16)
    got = ev.array[:n_events]
    same = bool(np.array_equal(want_off, eoff.array[:n + 1]) and np.array_equal(
        np.where(np.isnan(got), np.float32(np.nan), got).view(np.uint32), np.where(np.isnan(want), np.float32(np.nan), want).view(np.uint32)))
    host16_ms, host16_runs = timed(lambda: ra.detect_events_host(hs, ho, threads=16) and None, a.reps)
    host1_ms = None
    if not a.no_host1:
        host1_ms, _ = timed(lambda: ra.detect_events_host(hs, ho, threads=1) and None, max(5, a.reps // 2), warm_s=0.0)
    rec = {
        "probe": "events", "chunks": n, "samples_per_chunk": a.samples, "samples": N, "events": n_events, "bit_exact_vs_host": same,
        "kernel_ms": round(kernel_ms, 4), "call_ms": round(call_ms, 4), "h2d_ms": round(h2d_ms, 4),
        "call_over_h2d": round(call_ms / h2d_ms, 3), "host_16t_ms": round(host16_ms, 3),
        "host_1t_ms": None if host1_ms is None else round(host1_ms, 3),
        "call_vs_host16_speedup": round(host16_ms / call_ms, 2),
        "kernel_samples_per_s": round(N / (kernel_ms * 1e-3), 0), "call_samples_per_s": round(N / (call_ms * 1e-3), 0),
        "call_events_per_s": round(n_events / (call_ms * 1e-3), 0),
        "host_1t_ns_per_sample": None if host1_ms is None else round(host1_ms * 1e6 / N, 2),
        "runs": {"kernel_ms": kernel_runs, "call_ms": call_runs, "h2d_ms": h2d_runs, "host_16t_ms": host16_runs}, "reps": a.reps,
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
