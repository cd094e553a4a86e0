#!/usr/bin/env python3
"""Resident rounds with the primary chains kept on the device ("resident_chains") against the same rounds without, in one process on the
same inputs: --reads reads (16 384) of --chunks chunks (4) of about 400 events each -- noisy stretches of both strands of a synthetic
reference of --ref-bp (4.6 Mb), a chunk where the one before ended --, device chaining, one group, "device_round_end" on for both, a
stop rule that never fires (the all-chunks flow).  Two contexts and mappers that differ in "resident_chains" alone (0 / --keep, 4 096),
taken in turns; every repetition maps all rounds on a fresh mapper.  Medians of --reps (7) repetitions after two warm-ups, every run
listed.  Per round:
  round_ms                 rawdtw_mapper_round_seeded_resident, host wall time
  host_phase_ms submit_ms  the mapper's timing slots 0 and 2 (rawdtw_mapper_timing)
  seed_bytes_to_device     12 bytes a previous seed actually sent up (rawdtw_mapper_resident_stats)
  kept                     rawdtw_mapper_kept_stats' increase over the round (option on)
  keep_kernel_us           k_keep_primary between its HIP events ("round_keep_kernel_us"; option on)
and over the run the option-off side's own spread (largest minus smallest round_ms of its repetitions, per round): the margin a
difference between the sides has to be read against.  The lines of both mappers must be equal.  --off-only runs the option-off side
alone (what a parent commit can run too).  Prints one JSON line (profiles/round_kept_probe.json).
python scripts/round_kept_probe.py [--reads N] [--ref-bp B] [--chunks C] [--reps R] [--keep N] [--opts name=value,...] [--off-only] [--out PATH]"""
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


def make_reads(ref, n, rng, events, chunks, sd=0.05):
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
    ap.add_argument("--ref-bp", type=int, default=4_600_000)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--events", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--keep", type=int, default=4096, help="\"resident_chains\" of the option-on side")
    ap.add_argument("--opts", default="chain_long_seeds=1048576", help="context options of both sides, name=value,name=value (rawdtw_set_option)")
    ap.add_argument("--off-only", action="store_true", help="the option-off side alone, without naming the option (a commit that has none)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import rawalign_amd as ra
    from rawalign_amd import mapper, seeding, synth
    from rawalign_amd.events import PinnedArray
    from rawalign_amd.mapping import StopOpt

    rng = np.random.default_rng(20241101)
    ref = synth.make_reference([a.ref_bp], seed=20241017)
    six = seeding.SeedIndex.from_signals(ref.forward, ref.reverse, threads=16)
    say("index built: %d keys, %d positions" % (six.n_keys, six.n_positions))
    n, C = a.reads, a.chunks
    reads = make_reads(ref, n, rng, a.events, C)
    rounds = []
    for c in range(C):
        chunks = [r[c] for r in reads]
        N = sum(len(x) for x in chunks)
        ev, off = PinnedArray(N + 1, np.float32), PinnedArray(n + 1, np.uint64)
        ev.array[:N] = np.concatenate(chunks)
        off.array[:n + 1] = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.uint64)
        rounds.append(dict(ev=ev, off=off, N=N))
    stop = StopOpt(min_bestmap_ratio=1e9, min_meanmap_ratio=1e9, min_chain_anchor=10 ** 6, max_num_chunk=C)   # (never fires: all chunks)
    opt = ra.MapOpt()
    sides = {}
    for on in ((0,) if a.off_only else (0, 1)):
        eng = ra.Engine(0)
        for item in filter(None, a.opts.split(",")):
            name, value = item.split("=")
            eng.set_option(name, int(value))
        eng.set_option("device_round_end", 1)
        if not a.off_only:
            eng.set_option("resident_chains", a.keep if on else 0)
        eng.upload_reference(ref.forward, ref.reverse)
        eng.upload_seed_index(six)
        sides[on] = eng
    lib = sides[0].lib

    def one(on):
        eng = sides[on]
        cm = mapper.CMapper(eng, opt, stop, ["synth_0"], [len(ref.forward[0])], slot_events=a.events * C + 64, max_reads=n, threads=16, carry=False,
                            device_chain=True, groups=1)
        ids = np.array([cm.add_read("r%d" % r, 4000 * C, C) for r in range(n)], np.uint32)
        per = []
        for rd in rounds:
            eng.sync()
            t0, s0 = cm.timing(), cm.resident_stats()
            k0 = cm.kept_stats() if not a.off_only else {}
            t = time.perf_counter()
            st = lib.rawdtw_mapper_round_seeded_resident(cm._h, six._h, n, ids.ctypes.data, rd["off"].ptr, rd["ev"].ptr)
            ms = (time.perf_counter() - t) * 1e3
            assert st == 0, lib.rawdtw_mapper_last_error(cm._h)
            t1, s1 = cm.timing(), cm.resident_stats()
            row = dict(round_ms=ms, host_phase_ms=t1["host_phase_ms"] - t0["host_phase_ms"], submit_ms=t1["submit_ms"] - t0["submit_ms"],
                       seed_bytes_to_device=s1["seed_bytes_to_device"] - s0["seed_bytes_to_device"], fell_back=s1["fallback_rounds"] - s0["fallback_rounds"])
            if not a.off_only:
                k1 = cm.kept_stats()
                row["kept"] = {k: k1[k] - k0[k] for k in k1}
                row["keep_kernel_us"] = eng.get_option("round_keep_kernel_us") if on else 0
            per.append(row)
        assert cm.finish() == 0
        lines = [cm.paf(int(i)) for i in ids[:512]]
        cm.close()
        return per, lines

    order = list(sides)
    for _ in range(2):   # warm-ups: workspaces, page-locked buffers, the table, the store
        for on in order:
            one(on)
    runs = {on: [] for on in order}
    same = True
    for rep in range(a.reps):
        res = {on: one(on) for on in (order if rep % 2 == 0 else order[::-1])}
        for on in order:
            runs[on].append(res[on][0])
        same = same and all(res[on][1] == res[0][1] for on in order)

    def side(on):
        rs = runs[on]
        out = []
        for c in range(C):
            ms = [r[c]["round_ms"] for r in rs]
            row = {"round_ms": round(float(np.median(ms)), 3), "round_ms_runs": [round(x, 3) for x in ms], "round_ms_spread": round(max(ms) - min(ms), 3),
                   "host_phase_ms": round(float(np.median([r[c]["host_phase_ms"] for r in rs])), 3),
                   "submit_ms": round(float(np.median([r[c]["submit_ms"] for r in rs])), 3),
                   "seed_bytes_to_device": int(rs[-1][c]["seed_bytes_to_device"]), "fell_back": int(sum(r[c]["fell_back"] for r in rs))}
            if "kept" in rs[-1][c]:
                row["kept"] = rs[-1][c]["kept"]
                row["keep_kernel_us"] = int(np.median([r[c]["keep_kernel_us"] for r in rs]))
            out.append(row)
        return out

    rec = {"probe": "round_kept", "reads": n, "reference_bp": a.ref_bp, "chunks": C, "events_per_chunk": a.events, "reps": a.reps, "host_threads": 16, "groups": 1,
           "options": a.opts, "resident_chains": a.keep, "same_lines": same, "option_off": side(0)}
    if not a.off_only:
        rec["option_on"] = side(1)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for eng in sides.values():
        eng.close()
    if not same:
        sys.exit("the lines differ with the option on")


if __name__ == "__main__":
    main()
