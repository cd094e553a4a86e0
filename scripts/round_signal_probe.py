#!/usr/bin/env python3
"""One chunk round from raw signal through the parent's path against the same round through rawdtw_mapper_round_raw_resident, in one
process on the same inputs: 16 384 int16 windows of 4 000 samples (reads drawn from both strands of a synthetic genome, converted to
DAC samples on one channel) and the index of that genome, device chaining, one group.
  (a) rawdtw_detect_raw_begin / rawdtw_detect_end into page-locked arrays, then rawdtw_mapper_round_seeded_resident on them: every
      event comes home and goes up again, and the host waits between detection and seeding
  (b) rawdtw_mapper_round_raw_resident: the samples go up, the events never leave the device
Either path keeps one mapper over all its rounds; a round's reads (one chunk each) are added before and released after the timed
stretch.  Method: a warm-up of either
path, then three brackets a path, alternating; a bracket repeats the round until at least --bracket-ms of timed wall time have passed
and gives the mean of its rounds; the figure is the median of the three brackets.  Prints one JSON line
(profiles/round_signal_probe.json): a_ms (and its two parts), b_ms, b_over_a, the byte counters of either path, and the checks that
must hold whatever the times are -- the same PAF lines from both paths, no event byte crossing in (b).  The *_ms entries of counters_* are
rawdtw_mapper_timing's share of the last round of either path: where the mapper's call spent its time.
python scripts/round_signal_probe.py [--reads N] [--distinct D] [--ref-bp B] [--bracket-ms T] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=16384)
    ap.add_argument("--distinct", type=int, default=2048, help="distinct signals; the windows repeat them (every window is a read of its own)")
    ap.add_argument("--ref-bp", type=int, default=500_000)
    ap.add_argument("--bracket-ms", type=float, default=200.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import rawalign_amd as ra
    from rawalign_amd import mapper, seeding, synth
    from rawalign_amd.events import PinnedArray
    from rawalign_amd.mapping import StopOpt
    from rawalign_amd.rawsig import CHANNEL_DTYPE, Channel

    n, W = a.reads, 4000
    d = min(a.distinct, n)
    ref = synth.make_reference([a.ref_bp], seed=20241017)
    six = seeding.SeedIndex.from_signals(ref.forward, ref.reverse, threads=16)
    g = synth.make_genome(a.ref_bp, 20241017)
    rng = np.random.default_rng(20250301)
    pa = synth.make_genome_raw_reads(g, rng.integers(0, a.ref_bp - 800, d), [700] * d, rng.integers(0, 2, d), seed=20250302)
    chan = Channel(8192.0, 1450.0, 3.0)
    assert all(len(x) >= W for x in pa)
    dac = np.stack([np.round(x[:W] * (chan.digitisation / chan.range) - chan.offset).astype(np.int16) for x in pa])
    raw, off, ch = PinnedArray(n * W + 8, np.int16), PinnedArray(n + 1, np.uint64), PinnedArray(n, CHANNEL_DTYPE)
    raw.array[:n * W] = dac[np.arange(n) % d].reshape(-1)
    off.array[:n + 1] = np.arange(n + 1, dtype=np.uint64) * W
    ch.array[:n] = (chan.digitisation, chan.range, chan.offset)
    slen, eoff, ev = PinnedArray(n, np.uint32), PinnedArray(n + 1, np.uint64), PinnedArray(n * W, np.float32)
    say("%d windows of %d samples (%d distinct), %.1f MB of int16" % (n, W, d, n * W * 2 / 1e6))

    eng = ra.Engine(0)
    eng.upload_reference(ref.forward, ref.reverse)
    eng.upload_seed_index(six)
    lib = eng.lib
    opt = ra.MapOpt()
    stop = StopOpt()

    # one mapper a path, kept over all its rounds: its page-locked buffers grow in the warm-up.  A read has one chunk, so it is finished after
    # its round; it is released and n new reads are added outside the timed stretch.
    mappers = {p: mapper.CMapper(eng, opt, stop, ["synth_0"], [len(ref.forward[0])], slot_events=1024, max_reads=n, threads=16, carry=False,
                                 device_chain=True) for p in ("a", "b")}

    def counters(cm):
        tm = cm.timing()
        c = dict(cm.resident_stats(), **cm.signal_stats(), events_up_bytes=tm["event_bytes"])
        c.update({k: float(v) for k, v in tm.items() if k.endswith("_ms")})   # (rawdtw_mapper_timing: where the call's time went)
        return c

    def one(path):
        """one round: (ms of the round, ms of its detection alone for path a, the round's counters, the first lines)"""
        cm = mappers[path]
        ids = np.array([cm.add_read("r%d" % r, W, 1) for r in range(n)], np.uint32)
        before = counters(cm)
        eng.sync()
        t0 = time.perf_counter()
        t_det = 0.0
        if path == "a":
            st = lib.rawdtw_detect_raw_begin(eng._ctx, None, n, off.ptr, raw.ptr, ch.ptr, slen.ptr, eoff.ptr, ev.ptr, n * W)
            assert st == 0, lib.rawdtw_last_error(eng._ctx)
            st = lib.rawdtw_detect_end(eng._ctx, None)
            assert st == 0, lib.rawdtw_last_error(eng._ctx)
            t_det = (time.perf_counter() - t0) * 1e3
            st = lib.rawdtw_mapper_round_seeded_resident(cm._h, six._h, n, ids.ctypes.data, eoff.ptr, ev.ptr)
        else:
            st = lib.rawdtw_mapper_round_raw_resident(cm._h, six._h, None, n, ids.ctypes.data, off.ptr, raw.ptr, ch.ptr)
        ms = (time.perf_counter() - t0) * 1e3
        assert st == 0, lib.rawdtw_mapper_last_error(cm._h)
        cnt = {k: round(v - before[k], 3) if isinstance(v, float) else v - before[k] for k, v in counters(cm).items()}
        if path == "a":
            cnt["events_home_bytes"] = 4 * int(eoff.array[n])
            cnt["event_bytes_crossed"] = cnt["events_home_bytes"] + cnt["events_up_bytes"]
            cnt["sample_bytes_to_device"] = 2 * n * W
        lines = [cm.paf(int(i)) for i in ids[:256]]
        for i in ids:
            assert cm.state(int(i))[0]
            cm.release_read(int(i))
        return ms, t_det, cnt, lines

    def bracket(path):
        total = det = 0.0
        k = 0
        while total < a.bracket_ms:
            ms, t_det, cnt, lines = one(path)
            total += ms
            det += t_det
            k += 1
        return total / k, det / k, k, cnt, lines

    for path in ("a", "b", "a", "b"):   # warm-up: workspaces, page-locked buffers, the table, the guess of events_cap
        one(path)
    runs = {"a": [], "b": []}
    for _ in range(3):
        for path in ("a", "b"):
            runs[path].append(bracket(path))
            say(path, "%.3f ms a round over %d rounds" % (runs[path][-1][0], runs[path][-1][2]))
    med = lambda path, i: float(np.median([r[i] for r in runs[path]]))  # noqa: E731
    ca, cb = runs["a"][-1][3], runs["b"][-1][3]
    checks = {
        "same_lines": runs["a"][-1][4] == runs["b"][-1][4],
        "no_event_bytes_crossed_in_b": cb["event_bytes_crossed"] == 0 and cb["events_up_bytes"] == 0,
        "b_not_retried": cb["retried_rounds"] == 0,
        "same_round_kind": (ca["resident_rounds"], ca["fallback_rounds"]) == (cb["resident_rounds"], cb["fallback_rounds"]) == (1, 0),
    }
    a_ms, b_ms = med("a", 0), med("b", 0)
    rec = {
        "probe": "round_signal", "windows": n, "samples_a_window": W, "distinct_signals": d, "reference_bp": a.ref_bp,
        "events": int(eoff.array[n]), "mapped_of_first_256": sum("\t*\t" not in ln for ln in runs["b"][-1][4]),
        "a_ms": round(a_ms, 3), "a_detect_ms": round(med("a", 1), 3), "a_round_ms": round(a_ms - med("a", 1), 3), "b_ms": round(b_ms, 3),
        "b_over_a": round(b_ms / a_ms, 4),
        "brackets": {p: [dict(ms=round(r[0], 3), rounds=r[2]) for r in runs[p]] for p in runs},
        "bracket_ms": a.bracket_ms, "counters_a": ca, "counters_b": cb, "checks": checks,
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for cm in mappers.values():
        cm.close()
    eng.close()
    if not all(checks.values()):
        sys.exit("a check failed: %s" % checks)


if __name__ == "__main__":
    main()
