#!/usr/bin/env python3
"""Seeding on the device against its own copies, the host path and the reference's own code: 16 384 chunks of about 400 events,
noisy stretches (a few events dropped or doubled) of both strands of a 4.6 Mb synthetic reference, at the parameters of
ri_idxopt_init (e 6, q 9, lq 3, w 0; --w N: the index and the chunks' sketches at a minimizer window of N, which the device seeds
only with --opts seed_minimizer=1).  Prints one JSON line (profiles/seed_probe.json):
  kernel_ms        the four launches' device time (HIP events, rawdtw_seed_end)
  call_ms          rawdtw_seed_begin ... rawdtw_seed_end from and into page-locked memory, host wall time
  h2d_ms, d2h_ms   plain copies of the events up and of as many bytes as the hits down, page-locked, timed in the same run
  host_1t_ms, host_16t_ms   rawdtw_seed_hits_host on 1 and 16 threads
  ref_1t_ms        the reference's own ri_sketch + ri_idx_get (oracle.loader.RefMap.hits, oracle/_ref) on one thread over the first
                   --ref-chunks chunks, scaled to the whole batch by hits (not code under test: the baseline)
each the median of --reps runs after a warm-up of at least 200 ms (the host's and the reference's legs: fewer runs, no warm-up).
python scripts/seed_probe.py [--chunks N] [--ref-bp B] [--reps R] [--ref-chunks K] [--w N] [--opts name=value,...] [--out PATH]"""
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


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def make_chunks(ref, n, rng, events=400, sd=0.05):
    lens = np.array([len(x) for x in ref.forward])
    out = []
    for k in range(n):
        s = int(rng.integers(0, len(lens)))
        arr = ref.forward[s] if k % 2 else ref.reverse[s]
        lo = int(rng.integers(0, lens[s] - events))
        idx = np.repeat(np.arange(lo, lo + events), rng.choice(3, size=events, p=(0.02, 0.95, 0.03)))[:events]
        out.append((arr[idx] + rng.normal(0, sd, len(idx))).astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=16384)
    ap.add_argument("--ref-bp", type=int, default=4_600_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref-chunks", type=int, default=1024)
    ap.add_argument("--no-host1", action="store_true")
    ap.add_argument("--device-only", action="store_true", help="the device call alone, a few times (for a profiler run)")
    ap.add_argument("--w", type=int, default=0, help="the minimizer window of the index and the sketches (0: every e-mer)")
    ap.add_argument("--opts", default="", help="context options, name=value,name=value (rawdtw_set_option)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch  # (the plain copies; torch's HIP runtime initialises first, as in the tests)

    torch.cuda.init()
    import rawalign_amd as ra
    from rawalign_amd import seeding, synth
    from rawalign_amd.events import PinnedArray

    lib = ra.load_library()
    rng = np.random.default_rng(20241016)
    ref = synth.make_reference([a.ref_bp], seed=20241017)
    say("reference made")
    t = time.perf_counter()
    pars = seeding.SeedParams(w=a.w)
    six = seeding.SeedIndex.from_signals(ref.forward, ref.reverse, pars, threads=16)
    build_ms = (time.perf_counter() - t) * 1e3
    say("index built: %d keys, %d positions, %.0f MB" % (six.n_keys, six.n_positions, six.table_bytes / 1e6))
    chunks = make_chunks(ref, a.chunks, rng)
    n = a.chunks
    N = sum(len(c) for c in chunks)
    ev = PinnedArray(N, np.float32)
    ev.array[:N] = np.concatenate(chunks)
    off = PinnedArray(n + 1, np.uint64)
    off.array[:n + 1] = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint64)
    hev, hoff_in = ev.array[:N], off.array[:n + 1]
    host16_ms, host16_runs = timed(lambda: seeding.seed_hits_host(six, hev, hoff_in, threads=16) and None, 3, warm_s=0.0)
    want_off, want = seeding.seed_hits_host(six, hev, hoff_in, threads=16)
    H = int(want_off[n])
    say("host: %d hits, %.1f ms on 16 threads" % (H, host16_ms))
    hoff, hits = PinnedArray(n + 1, np.uint64), PinnedArray(H, seeding.HIT_DTYPE)
    eng = ra.Engine(0)
    for item in filter(None, a.opts.split(",")):
        name, value = item.split("=")
        eng.set_option(name, int(value))
    t = time.perf_counter()
    eng.upload_seed_index(six)
    upload_ms = (time.perf_counter() - t) * 1e3
    ms = C.c_float()

    def call():
        st = lib.rawdtw_seed_begin(eng._ctx, n, off.ptr, ev.ptr, hoff.ptr, hits.ptr, H)
        st = st or lib.rawdtw_seed_end(eng._ctx, C.byref(ms))
        assert st == 0, lib.rawdtw_last_error(eng._ctx)

    if a.device_only:
        for _ in range(5):
            call()
        eng.close()
        return
    call_ms, call_runs = timed(call, a.reps)

    def kernels():
        call()
        return ms.value

    kernel_ms, kernel_runs = timed(kernels, a.reps)
    same = bool(np.array_equal(hoff.array[:n + 1], want_off) and hits.array[:H].tobytes() == want.tobytes())
    say("device: call %.2f ms, kernels %.2f ms, equal to the host: %s" % (call_ms, kernel_ms, same))
    # plain copies of the same bytes, page-locked, in the same process
    h_ev, d_ev = torch.from_numpy(ev.array[:N]), torch.empty(N, dtype=torch.float32, device="cuda:0")
    h_hits = torch.from_numpy(hits.array[:H].view(np.uint8).reshape(-1))
    d_hits = torch.empty(H * 16, dtype=torch.uint8, device="cuda:0")

    def h2d():
        d_ev.copy_(h_ev, non_blocking=True)
        torch.cuda.synchronize()

    def d2h():
        h_hits.copy_(d_hits, non_blocking=True)
        torch.cuda.synchronize()

    h2d_ms, h2d_runs = timed(h2d, a.reps)
    d2h_ms, d2h_runs = timed(d2h, a.reps)
    host1_ms = None
    if not a.no_host1:
        host1_ms, _ = timed(lambda: seeding.seed_hits_host(six, hev, hoff_in, threads=1) and None, 3, warm_s=0.0)
        say("host: %.1f ms on 1 thread" % host1_ms)
    # the reference's own code on one thread, over the first chunks
    ref_ms = ref_scaled = None
    ref_same = None
    from oracle.loader import RefMap

    if RefMap.available() and a.ref_chunks:
        rm = RefMap(ref.forward, ref.reverse, w=a.w)
        k = min(a.ref_chunks, n)
        say("reference index built")

        def ref_run():
            for c in chunks[:k]:
                rm.hits(c)

        ref_ms, _ = timed(ref_run, 3, warm_s=0.0)
        got = np.concatenate([rm.hits(c) for c in chunks[:16]])
        w16 = want[:int(want_off[16])]
        ref_same = bool(np.array_equal(got, np.stack([w16["ref_seq"], w16["strand"].astype(np.uint32), w16["target_position"], w16["query_position"]], 1)))
        ref_scaled = ref_ms * H / max(int(want_off[k]), 1)
    lookups = int(sum(max(0, len(seeding.sketch(c, pars)[0])) for c in chunks[:256])) * n / 256   # (estimated from the first 256 chunks)
    rec = {
        "probe": "seed", "w": a.w, "opts": a.opts, "elements_per_event": round(lookups / N, 4), "chunks": n, "events": N, "hits": H, "hits_per_chunk": round(H / n, 1), "lookups_est": int(lookups),
        "reference_bp": a.ref_bp, "keys": six.n_keys, "positions": six.n_positions, "table_bytes": six.table_bytes,
        "index_build_16t_ms": round(build_ms, 1), "table_upload_ms": round(upload_ms, 1), "equal_to_host": same,
        "kernel_ms": round(kernel_ms, 4), "call_ms": round(call_ms, 4), "h2d_ms": round(h2d_ms, 4), "d2h_ms": round(d2h_ms, 4),
        "event_bytes": N * 4, "hit_bytes": H * 16,
        "host_16t_ms": round(host16_ms, 3), "host_1t_ms": None if host1_ms is None else round(host1_ms, 3),
        "ref_1t_ms_on_ref_chunks": None if ref_ms is None else round(ref_ms, 3), "ref_chunks": a.ref_chunks,
        "ref_1t_ms_scaled": None if ref_scaled is None else round(ref_scaled, 3),
        "ref_1t_over_16_ms": None if ref_scaled is None else round(ref_scaled / 16, 3), "ref_equal_on_16_chunks": ref_same,
        "call_vs_host16_speedup": round(host16_ms / call_ms, 2),
        "kernel_hits_per_s": round(H / (kernel_ms * 1e-3), 0),   # (the probe launch's own rate: lookups_est over its time in the kernel trace)
        "runs": {"kernel_ms": kernel_runs, "call_ms": call_runs, "h2d_ms": h2d_runs, "d2h_ms": d2h_runs, "host_16t_ms": host16_runs},
        "reps": a.reps,
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
