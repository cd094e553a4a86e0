#!/usr/bin/env python3
"""One chunk round through rawdtw_mapper_round_seeded against the same round through rawdtw_mapper_round_seeded_resident, in one
process on the same inputs: 16 384 reads, two chunks of about 400 events each (noisy stretches of both strands of a synthetic
reference, the second where the first ended), device chaining, one group, no read stopping before round 2.  Round 1 has no
previous chains; round 2 has, so its seed lists hold the previous chains' anchors too.  Each repetition maps both rounds on a
fresh mapper through either path; the times are the median of --reps repetitions after one warm-up, with every run listed.
Prints one JSON line (profiles/round_resident_probe.json):
  seeded_ms / resident_ms   host wall time of the round's call, per round
  counters                  rawdtw_mapper_resident_stats and slots 6 and 7 of rawdtw_mapper_timing after the two rounds
  checks                    what must hold whatever the times are: no hit bytes home on the capped workload, 12 bytes a previous
                            anchor up, the events' bytes once, the same PAF lines from both paths
--ref-bp sets the reference: 500 kb keeps every read below the chaining's 2 048-seed cap (checked here on the host); 4.6 Mb, the
reference of scripts/seed_probe.py, puts most reads above it and every round falls back -- the cost of that cap.
--w N builds the index (and so seeds the chunks) at a minimizer window of N; the mapper seeds such a round on its context only with
--opts seed_minimizer=1 (without it rawdtw_mapper_round_seeded seeds on the host and the resident round is refused).
python scripts/round_resident_probe.py [--reads N] [--ref-bp B] [--reps R] [--w N] [--opts name=value,...] [--resident-only] [--out PATH]"""
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


def make_reads(ref, n, rng, events=400, chunks=2, sd=0.05):
    """per read `chunks` chunks of `events` events: one noisy stretch (a few events dropped or doubled) cut into pieces"""
    lens = np.array([len(x) for x in ref.forward])
    out = []
    total = events * chunks
    for k in range(n):
        s = int(rng.integers(0, len(lens)))
        arr = ref.forward[s] if k % 2 else ref.reverse[s]
        lo = int(rng.integers(0, lens[s] - total))
        idx = np.repeat(np.arange(lo, lo + total), rng.choice(3, size=total, p=(0.02, 0.95, 0.03)))[:total]
        x = (arr[idx] + rng.normal(0, sd, len(idx))).astype(np.float32)
        out.append([x[c * events:(c + 1) * events] for c in range(chunks)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=16384)
    ap.add_argument("--ref-bp", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--resident-only", action="store_true", help="the resident rounds alone, a few times (for a profiler run)")
    ap.add_argument("--w", type=int, default=0, help="the minimizer window of the index (0: every e-mer)")
    ap.add_argument("--opts", default="", help="context options, name=value,name=value (rawdtw_set_option)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import rawalign_amd as ra
    from rawalign_amd import mapper, seeding, synth
    from rawalign_amd.events import PinnedArray
    from rawalign_amd.mapping import StopOpt

    rng = np.random.default_rng(20241101)
    ref = synth.make_reference([a.ref_bp], seed=20241017)
    six = seeding.SeedIndex.from_signals(ref.forward, ref.reverse, seeding.SeedParams(w=a.w), threads=16)
    say("index built: %d keys, %d positions" % (six.n_keys, six.n_positions))
    n = a.reads
    reads = make_reads(ref, n, rng)
    rounds = []   # per round: page-locked events and offsets, the host's hit counts
    for c in range(2):
        chunks = [r[c] for r in reads]
        N = sum(len(x) for x in chunks)
        ev, off = PinnedArray(N + 1, np.float32), PinnedArray(n + 1, np.uint64)
        ev.array[:N] = np.concatenate(chunks)
        off.array[:n + 1] = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.uint64)
        hoff = seeding.seed_hits_host(six, ev.array[:N], off.array[:n + 1], threads=16)[0].astype(np.int64)
        rounds.append(dict(ev=ev, off=off, N=N, hits=np.diff(hoff)))
        say("round %d: %d events, %d hits, %.0f a chunk, at most %d" % (c + 1, N, int(hoff[-1]), hoff[-1] / n, int(np.diff(hoff).max())))
    so_far = rounds[0]["hits"] + rounds[1]["hits"]   # (a read's seeds in round 2 are at most its hits so far)
    eng = ra.Engine(0)
    for item in filter(None, a.opts.split(",")):
        name, value = item.split("=")
        eng.set_option(name, int(value))
    eng.upload_reference(ref.forward, ref.reverse)
    eng.upload_seed_index(six)
    opt = ra.MapOpt()
    stop = StopOpt(min_bestmap_ratio=1e9, min_meanmap_ratio=1e9, min_chain_anchor=10 ** 6)   # (no read stops before round 2)
    lib = eng.lib

    def one(resident):
        cm = mapper.CMapper(eng, opt, stop, ["synth_0"], [len(ref.forward[0])], slot_events=1024, max_reads=n, threads=16, carry=False, device_chain=True)
        ids = np.array([cm.add_read("r%d" % r, 8000, 2) for r in range(n)], np.uint32)
        fn = lib.rawdtw_mapper_round_seeded_resident if resident else lib.rawdtw_mapper_round_seeded
        ms, stats = [], []
        for rd in rounds:
            eng.sync()
            t = time.perf_counter()
            st = fn(cm._h, six._h, n, ids.ctypes.data, rd["off"].ptr, rd["ev"].ptr)
            ms.append((time.perf_counter() - t) * 1e3)
            assert st == 0, lib.rawdtw_mapper_last_error(cm._h)
            tm = cm.timing()
            stats.append(dict(cm.resident_stats(), event_bytes=tm["event_bytes"], other_bytes=tm["other_bytes"]))
        lines = [cm.paf(int(i)) for i in ids[:256]]
        cm.close()
        return ms, stats, lines

    if a.resident_only:
        for _ in range(3):
            one(True)
        eng.close()
        return
    one(False), one(True)   # warm-up: workspaces, page-locked buffers, the table
    runs = {False: [], True: []}
    for _ in range(a.reps):
        for resident in (False, True):
            runs[resident].append(one(resident))
    med = lambda res, c: float(np.median([r[0][c] for r in runs[res]]))  # noqa: E731
    s_stats, r_stats = runs[False][-1][1], runs[True][-1][1]
    nr = n
    extra = (nr + 1) * 8 + nr * 5 + (nr + 1) * 8 + nr * 8   # a resident round's own small arrays (rawdtw_mapper_round.cpp, resident_bytes)
    checks = {}
    capped = bool(so_far.max() <= 2048)
    last = r_stats[-1]
    checks["same_lines"] = runs[False][-1][2] == runs[True][-1][2]
    checks["events_counted_once"] = last["event_bytes"] == 4 * (rounds[0]["N"] + rounds[1]["N"])
    fell = [r_stats[c]["fallback_rounds"] - (r_stats[c - 1]["fallback_rounds"] if c else 0) for c in range(2)]
    if capped:
        checks["no_hit_bytes_to_host"] = last["hit_bytes_to_host"] == 0 and last["fallback_rounds"] == 0 and last["resident_rounds"] == 2
        # 12 bytes a previous anchor and nothing else: round 1 has none; in either round slot 7 of the two paths differs by the resident round's
        # small arrays and by 12 bytes for every hit -- what _seeded's seed list holds beyond the previous anchors
        checks["seed_bytes_are_12_a_previous_anchor"] = r_stats[0]["seed_bytes_to_device"] == 0 and last["seed_bytes_to_device"] % 12 == 0 and last["seed_bytes_to_device"] > 0
        for c in range(2):
            d7s = s_stats[c]["other_bytes"] - (s_stats[c - 1]["other_bytes"] if c else 0)
            d7r = r_stats[c]["other_bytes"] - (r_stats[c - 1]["other_bytes"] if c else 0)
            checks["round%d_only_the_hits_stayed_down" % (c + 1)] = d7s - (d7r - extra) == 12 * int(rounds[c]["hits"].sum())
    else:
        checks["fallback_hit_bytes_are_16_a_hit"] = last["hit_bytes_to_host"] == 16 * sum(int(rounds[c]["hits"].sum()) for c in range(2) if fell[c])
    rec = {
        "probe": "round_resident", "reads": n, "reference_bp": a.ref_bp, "events_per_round": [r["N"] for r in rounds],
        "hits_per_round": [int(r["hits"].sum()) for r in rounds], "max_hits_a_chunk": [int(r["hits"].max()) for r in rounds],
        "max_hits_so_far_a_read": int(so_far.max()), "inside_seed_cap": capped,
        "seeded_ms": [round(med(False, c), 3) for c in range(2)], "resident_ms": [round(med(True, c), 3) for c in range(2)],
        "runs": {"seeded_ms": [[round(x, 3) for x in r[0]] for r in runs[False]], "resident_ms": [[round(x, 3) for x in r[0]] for r in runs[True]]},
        "counters_resident": r_stats, "counters_seeded": s_stats, "previous_anchors_round2": last["seed_bytes_to_device"] // 12, "fell_back": fell,
        "checks": checks, "reps": a.reps,
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()
    if not all(checks.values()):
        sys.exit("a check failed: %s" % checks)


if __name__ == "__main__":
    main()
