#!/usr/bin/env python3
"""--dtw-output-cigar behind rounds from signal ("signal_cigar"): what rawdtw_mapper_finish costs when it reads the reads' events in the
event arena against the parent's path, and what rawdtw_events_fetch costs against a plain copy.  scripts/round_signal_probe.py's workload cut
down to what finishes in seconds: --reads int16 windows of 4 000 samples (reads drawn from both strands of a synthetic genome, converted to
DAC samples on one channel), the index of that genome, device chaining, one group, flag 0x4 on both mappers, one chunk a read.
  (a) the parent's path: rawdtw_detect_raw_begin / rawdtw_detect_end + rawdtw_mapper_round_seeded_resident on the host's events, then
      rawdtw_mapper_finish -- it lays the mapped reads' host copies one behind the other and uploads them
  (b) "signal_cigar" = 1: rawdtw_mapper_round_raw_resident, then rawdtw_mapper_finish -- the jobs index the reads' slots, nothing goes up
  (c) one rawdtw_events_fetch of every read's events out of (b)'s arena, into page-locked and into pageable memory, against a plain
      device-to-host copy of as many bytes into page-locked memory
Method: each of the timed calls once as a warm-up, then seven times; the figure is the median of the seven, with their minimum and maximum.
rawdtw_mapper_finish can be repeated on a mapper: it recomputes the same strings.  Prints one JSON line
(profiles/signal_cigar_probe.json) with the figures and the checks that must hold whatever the times are: the same PAF lines from both
mappers, no event byte crossed in (b), the fetched events equal to (a)'s host events.  A probe, not a threshold: nothing is asserted of a time.
python scripts/signal_cigar_probe.py [--reads N] [--ref-bp B] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 7


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def seven(fn):
    """fn() once untimed, then REPS times: (median, min, max) in ms"""
    fn()
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--ref-bp", type=int, default=500_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch  # (first: PyTorch bundles its own HIP runtime)

    import rawalign_amd as ra
    from rawalign_amd import mapper, seeding, synth
    from rawalign_amd.events import PinnedArray
    from rawalign_amd.mapping import StopOpt
    from rawalign_amd.rawsig import CHANNEL_DTYPE, Channel

    n, W, SLOT = a.reads, 4000, 1024
    ref = synth.make_reference([a.ref_bp], seed=20241017)
    six = seeding.SeedIndex.from_signals(ref.forward, ref.reverse, threads=16)
    g = synth.make_genome(a.ref_bp, 20241017)
    rng = np.random.default_rng(20250301)
    pa = synth.make_genome_raw_reads(g, rng.integers(0, a.ref_bp - 800, n), [700] * n, rng.integers(0, 2, n), seed=20250302)
    chan = Channel(8192.0, 1450.0, 3.0)
    assert all(len(x) >= W for x in pa)
    raw, off, ch = PinnedArray(n * W + 8, np.int16), PinnedArray(n + 1, np.uint64), PinnedArray(n, CHANNEL_DTYPE)
    raw.array[:n * W] = np.stack([np.round(x[:W] * (chan.digitisation / chan.range) - chan.offset).astype(np.int16) for x in pa]).reshape(-1)
    off.array[:n + 1] = np.arange(n + 1, dtype=np.uint64) * W
    ch.array[:n] = (chan.digitisation, chan.range, chan.offset)
    slen, eoff, ev = PinnedArray(n, np.uint32), PinnedArray(n + 1, np.uint64), PinnedArray(n * W, np.float32)

    opt = ra.MapOpt(flag=ra.MapOpt().flag | 0x4)
    engines, mappers, ids = {}, {}, {}
    for p in ("a", "b"):
        e = ra.Engine(0)
        e.upload_reference(ref.forward, ref.reverse)
        e.upload_seed_index(six)
        if p == "b":
            e.set_option("signal_cigar", 1)
        engines[p] = e
        mappers[p] = mapper.CMapper(e, opt, StopOpt(), ["synth_0"], [len(ref.forward[0])], slot_events=SLOT, max_reads=n, threads=16, carry=False,
                                    device_chain=True)
        ids[p] = np.array([mappers[p].add_read("r%d" % r, W, 1) for r in range(n)], np.uint32)
    ea, eb, ca, cb = engines["a"], engines["b"], mappers["a"], mappers["b"]
    lib = ea.lib
    # the one round of either mapper
    assert lib.rawdtw_detect_raw_begin(ea._ctx, None, n, off.ptr, raw.ptr, ch.ptr, slen.ptr, eoff.ptr, ev.ptr, n * W) == 0, lib.rawdtw_last_error(ea._ctx)
    assert lib.rawdtw_detect_end(ea._ctx, None) == 0, lib.rawdtw_last_error(ea._ctx)
    assert lib.rawdtw_mapper_round_seeded_resident(ca._h, six._h, n, ids["a"].ctypes.data, eoff.ptr, ev.ptr) == 0, lib.rawdtw_mapper_last_error(ca._h)
    assert lib.rawdtw_mapper_round_raw_resident(cb._h, six._h, None, n, ids["b"].ctypes.data, off.ptr, raw.ptr, ch.ptr) == 0, lib.rawdtw_mapper_last_error(cb._h)
    n_events = int(eoff.array[n])
    say("%d windows of %d samples, %d events" % (n, W, n_events))

    def finish(cm):
        st = cm.finish()
        assert st == 0, lib.rawdtw_mapper_last_error(cm._h)

    up_before = cb.timing()["event_bytes"]
    fin_a = seven(lambda: finish(ca))
    fin_b = seven(lambda: finish(cb))
    lines_a, lines_b = [ca.paf(int(i)) for i in ids["a"]], [cb.paf(int(i)) for i in ids["b"]]
    with_cigar = sum("\taln:s:(" in ln for ln in lines_b)
    fin_a["spread_ms"] = round(fin_a["max_ms"] - fin_a["min_ms"], 3)
    import ctypes as C

    def tb_timing(e):   # (the kernels of the engine's last traceback call: rawdtw_traceback_timing)
        f, w, db, pe = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
        assert lib.rawdtw_traceback_timing(e._ctx, C.byref(f), C.byref(w), C.byref(db), C.byref(pe)) == 0
        return dict(fill_ms=round(f.value, 3), walk_ms=round(w.value, 3), direction_bytes=db.value, path_elements=pe.value)

    tb_a, tb_b = tb_timing(ea), tb_timing(eb)

    # (c) every read's events out of (b)'s arena in one call: read k's slot is k (the reads were added in order)
    lens = np.diff(eoff.array[:n + 1].astype(np.int64)).astype(np.uint32)
    starts = (np.arange(n, dtype=np.uint64) * SLOT).astype(np.uint32)
    ooff = np.zeros(n + 1, np.uint64)
    pin, page = PinnedArray(n_events + 1, np.float32), np.empty(n_events + 1, np.float32)

    def fetch(ptr):
        st = lib.rawdtw_events_fetch(eb._ctx, n, starts.ctypes.data, lens.ctypes.data, ooff.ctypes.data, ptr, n_events)
        assert st == 0, lib.rawdtw_last_error(eb._ctx)

    fetch_pin = seven(lambda: fetch(pin.ptr))
    fetch_page = seven(lambda: fetch(page.ctypes.data))
    same_events = bool(np.array_equal(pin.array[:n_events].view(np.uint32), ev.array[:n_events].view(np.uint32)) and
                       np.array_equal(page[:n_events].view(np.uint32), ev.array[:n_events].view(np.uint32)))
    d_src = torch.zeros(n_events, dtype=torch.float32, device="cuda:0")
    h_dst = torch.empty(n_events, dtype=torch.float32).pin_memory()

    def plain():
        h_dst.copy_(d_src, non_blocking=True)
        torch.cuda.synchronize()

    torch.cuda.synchronize()
    copy_pin = seven(plain)

    checks = {
        "same_lines": lines_a == lines_b,
        "lines_with_cigar": with_cigar > 0,
        "no_event_bytes_crossed_in_b": cb.signal_stats()["event_bytes_crossed"] == 0 and cb.timing()["event_bytes"] == up_before == 0,
        "fetched_events_are_the_hosts": same_events,
    }
    rec = {
        "probe": "signal_cigar", "windows": n, "samples_a_window": W, "reference_bp": a.ref_bp, "events": n_events, "event_bytes": 4 * n_events,
        "lines_with_cigar": with_cigar, "repetitions": REPS,
        "finish_parent": fin_a, "finish_arena": fin_b,
        "arena_minus_parent_ms": round(fin_b["median_ms"] - fin_a["median_ms"], 3),
        "arena_within_parents_spread": bool(fin_b["median_ms"] - fin_a["median_ms"] <= fin_a["spread_ms"]),
        "traceback_kernels_of_last_parent_finish": tb_a, "traceback_kernels_of_last_arena_finish": tb_b,
        "events_fetch_page_locked": fetch_pin, "events_fetch_pageable": fetch_page, "plain_d2h_page_locked": copy_pin,
        "checks": checks,
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    for cm in mappers.values():
        cm.close()
    for e in engines.values():
        e.close()
    if not all(checks.values()):
        sys.exit("a check failed: %s" % checks)


if __name__ == "__main__":
    main()
