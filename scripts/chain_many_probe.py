#!/usr/bin/env python3
"""rawdtw_chain_round with "chain_max_chains" off and on, in one process on the same seed lists: 16 384 reads, first chunks of 400 events, with
"chain_long_seeds" on.  Two workloads:
  many   a reference of 48 sequences of 10 000 events (synth.make_reference([10_000] * 48, seed=77)); reads with noise of sd 0.05 .. 0.3, every tenth
         from nowhere.  About half the reads have more than 16 chains with equal scores, so with the option off the round is declined: what
         that costs is the declined device attempt plus the host chaining the mapper then does (the lists chained by rawdtw_chain_anchors +
         rawdtw_sort_by_chaining_score on --threads threads; sorted and split beforehand, outside the time: a lower bound).  With the option on
         the round stays on the device.
  one    scripts/chain_long_probe.py's reference of one sequence of 500 000 events: no read declines either way -- the default path, which the
         option must not move.
Per workload and setting, medians of --reps repetitions after a warm-up, every run listed: the host wall time of rawdtw_chain_round (uploads,
k_chain, k_chain_long, scan, compaction, the copies home), the counters of rawdtw_chain_order_stats and rawdtw_chain_round_stats a round, and
whether the device's chains are the host's (host_ms: three runs; it holds one call from Python a list, which the mapper's host chaining does not
pay).  Kernel times are a profiler's: --device-only runs the chosen rounds alone, a few times, for a
kernel trace.  --root PATH imports rawalign_amd from another tree (a build of the parent commit, for an A/B of the default path in one
session); a library without the option runs the settings it has.
Prints one JSON line (profiles/chain_many_probe.json).
python scripts/chain_many_probe.py [--reads N] [--reps R] [--threads T] [--workloads many,one] [--settings off,on] [--max-chains N] [--device-only]
                                   [--root PATH] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED_DTYPE = np.dtype([("key", "<u4"), ("target_position", "<u4"), ("query_position", "<u4")])
REC_DTYPE = np.dtype([("chaining_score", "<f4"), ("key", "<u4"), ("start_position", "<u4"), ("end_position", "<u4"), ("n_anchors", "<u4")])
UNSUPPORTED = 5


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--events", type=int, default=400)
    ap.add_argument("--workloads", default="many,one")
    ap.add_argument("--settings", default="off,on")
    ap.add_argument("--max-chains", type=int, default=512)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))

    import rawalign_amd as ra
    from rawalign_amd import mapping as M
    from rawalign_amd import seeding, synth
    from rawalign_amd.dtw import ANCHOR_DTYPE

    n = a.reads
    eng = ra.Engine(0)
    lib = eng.lib
    has_option = hasattr(eng, "chain_order_stats")
    settings = [s for s in a.settings.split(",") if s == "off" or has_option]
    eng.set_option("chain_long_seeds", 1 << 20)
    copt = M.default_chain_opt(6)
    vp = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    pool = ThreadPoolExecutor(a.threads)

    def make_reads(ref, rng, nowhere):
        reads = []
        for r in range(n):
            if nowhere and r % 10 == 9:
                reads.append(rng.normal(0, 1, a.events).astype(np.float32))
                continue
            arr = (ref.forward, ref.reverse)[r & 1][int(rng.integers(0, len(ref.forward)))]
            at = int(rng.integers(0, len(arr) - a.events))
            sd = rng.uniform(0.05, 0.3) if nowhere else 0.05
            reads.append((arr[at:at + a.events] + rng.normal(0, sd, a.events)).astype(np.float32))
        return reads

    def seed_lists(ref, reads):
        six = seeding.SeedIndex.from_signals(ref.forward, ref.reverse, threads=a.threads)
        off = np.arange(n + 1, dtype=np.uint64) * a.events
        hoff, hits = seeding.seed_hits_host(six, np.concatenate(reads), off, threads=a.threads)
        seeds = np.zeros(len(hits) + 1, SEED_DTYPE)
        seeds["key"][:-1] = hits["ref_seq"] * 2 + (hits["strand"] != 0)
        seeds["target_position"][:-1], seeds["query_position"][:-1] = hits["target_position"], hits["query_position"]
        return hoff.astype(np.uint64), seeds

    def device_round(seed_off, seeds, n_keys):
        cap = max(n * 32, int(seed_off[-1]) // 2 + 1)
        out = dict(chain_off=np.zeros(n + 1, np.uint64), anchor_off=np.zeros(cap + 1, np.uint64), recs=np.zeros(cap, REC_DTYPE),
                   anchors=np.zeros(int(seed_off[-1]) + 1, ANCHOR_DTYPE))
        read_base, key_base = np.zeros(n, np.uint32), np.zeros(n_keys, np.uint64)
        d = [C.c_void_p() for _ in range(3)]
        eng.sync()
        t = time.perf_counter()
        st = lib.rawdtw_chain_round(eng._ctx, C.byref(copt), n, vp(seed_off), vp(seeds), vp(read_base), n_keys, vp(key_base), vp(out["chain_off"]), vp(out["anchor_off"]),
                                    vp(out["recs"]), cap, vp(out["anchors"]), *[C.byref(x) for x in d])
        return st, (time.perf_counter() - t) * 1e3, out

    def host_lists(seed_off, seeds):
        per = []
        for r in range(n):
            s = seeds[int(seed_off[r]):int(seed_off[r + 1])]
            s = s[np.lexsort((s["query_position"], s["target_position"], s["key"]))]
            lists = []
            for g in np.split(s, np.flatnonzero(np.diff(s["key"])) + 1) if len(s) else []:
                an = np.zeros(len(g), ANCHOR_DTYPE)
                an["target_position"], an["query_position"] = g["target_position"], g["query_position"]
                lists.append((int(g["key"][0]), an))
            per.append(lists)
        return per

    def host_read(lists):
        maxs, scores = 0.0, []
        for key, an in lists:
            cs, maxs = M.chain_anchors(an, copt, maxs, key >> 1, key & 1)
            scores += [c.chaining_score for c in cs]
        sc = np.array(scores, np.float32)
        perm = np.zeros(len(sc), np.uint32)
        if len(sc):
            lib.rawdtw_sort_by_chaining_score(vp(sc), len(sc), vp(perm))
        return sc[perm]

    def host_round(per):
        t = time.perf_counter()
        res = list(pool.map(host_read, per, chunksize=max(1, n // (a.threads * 8))))
        return (time.perf_counter() - t) * 1e3, res

    def set_many(on):
        if has_option:
            eng.set_option("chain_max_chains", a.max_chains if on else 0)

    rec = {"probe": "chain_many", "reads": n, "events_a_read": a.events, "reps": a.reps, "host_threads": a.threads, "max_chains": a.max_chains,
           "library_has_the_option": has_option, "workloads": {}}
    ok = True
    for name in a.workloads.split(","):
        if name == "many":
            ref, n_keys = synth.make_reference([10_000] * 48, seed=77), 96
        else:
            ref, n_keys = synth.make_reference([500_000], seed=20241017), 2
        seed_off, seeds = seed_lists(ref, make_reads(ref, np.random.default_rng(20250301), name == "many"))
        lens = np.diff(seed_off.astype(np.int64))
        say("%s: %d seeds, %.0f a read, at most %d" % (name, int(seed_off[-1]), lens.mean(), lens.max()))
        if a.device_only:
            for s in settings:
                set_many(s == "on")
                for _ in range(4):
                    device_round(seed_off, seeds, n_keys)
            continue
        per = host_lists(seed_off, seeds)
        first_host_ms, want = host_round(per)
        chains = np.array([len(x) for x in want])
        tied = np.array([len(x) > 16 and len(np.unique(x)) < len(x) for x in want])
        w = dict(seeds=int(seed_off[-1]), mean_seeds_a_read=round(float(lens.mean()), 1), max_seeds_a_read=int(lens.max()),
                 chains_a_read=dict(median=float(np.median(chains)), p90=float(np.percentile(chains, 90)), max=int(chains.max())),
                 reads_above_16_with_ties=int(tied.sum()), reads_above_32=int((chains > 32).sum()), reads_above_64=int((chains > 64).sum()))
        for s in settings:
            runs = {"device_ms": [], "host_ms": []}
            status, out = None, None
            set_many(s == "on")
            before = (eng.chain_round_stats(), eng.chain_order_stats() if has_option else {})
            for rep in range(a.reps + 1):   # (the first is the warm-up)
                status, ms, out = device_round(seed_off, seeds, n_keys)
                assert status in (0, UNSUPPORTED), lib.rawdtw_last_error(eng._ctx)
                # what the mapper does with a declined round; three runs, the pass that made `want` among them (a host round takes seconds)
                h_ms = (first_host_ms if rep == 1 else host_round(per)[0]) if status == UNSUPPORTED and 1 <= rep <= 3 else None
                if rep:
                    runs["device_ms"].append(round(ms, 3))
                    if h_ms is not None:
                        runs["host_ms"].append(round(h_ms, 3))
            after = (eng.chain_round_stats(), eng.chain_order_stats() if has_option else {})
            med = {k: (round(float(np.median(v)), 3) if v else None) for k, v in runs.items()}
            row = dict(declined=status == UNSUPPORTED, median=med, runs=runs, round_ms=round(med["device_ms"] + (med["host_ms"] or 0.0), 3),
                       counters_a_round={k: (after[i][k] - before[i][k]) // (a.reps + 1) for i in (0, 1) for k in after[i] if k not in ("max_chains_a_read",)},
                       max_chains_a_read=after[1].get("max_chains_a_read"))
            if status == 0:   # the device's chains are the host's: count, order, score bits
                same = True
                for r in range(n):
                    c0, c1 = int(out["chain_off"][r]), int(out["chain_off"][r + 1])
                    same = same and c1 - c0 == len(want[r]) and bool((out["recs"]["chaining_score"][c0:c1].view(np.uint32) == want[r].view(np.uint32)).all())
                row["same_chains_as_host"] = same
                ok = ok and same
            w[s] = row
        if "off" in w and "on" in w:
            w["off_over_on"] = round(w["off"]["round_ms"] / w["on"]["round_ms"], 3)
        rec["workloads"][name] = w
    if not a.device_only:
        line = json.dumps(rec)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
    eng.close()
    if not ok:
        sys.exit("the device's chains are not the host's")


if __name__ == "__main__":
    main()
