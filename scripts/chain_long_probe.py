#!/usr/bin/env python3
"""rawdtw_chain_round with the long path on ("chain_long_seeds") against the same round chained on the host, in one process on the same
seed lists: 16 384 reads, two rounds (chunks of about 400 events of noisy stretches of a synthetic reference, as
scripts/round_resident_probe.py makes them; round 2's seed lists hold round 1's chains' anchors and the second chunk's hits).
--ref-bp sets the reference: 500 kb leaves every read below k_chain's cap of 2 048 seeds (the long launch never runs: the option must cost
nothing there), 4.6 Mb puts every read above it (without the option every such round is chained on the host).
Per round, medians of --reps repetitions after a warm-up, every run listed:
  device_on_ms / device_off_ms   rawdtw_chain_round, host wall time, option on / off (off: only where no read is above the cap)
  host_ms                        the lists chained by rawdtw_chain_anchors + rawdtw_sort_by_chaining_score on --threads threads -- the DP, the
                                 traceback and the order; the lists are sorted and split beforehand, outside the time, so this is a lower
                                 bound of what a declined round costs the host
Prints one JSON line (profiles/chain_long_probe.json).  --device-only runs the device rounds alone, a few times, for a profiler's
kernel trace (profiles/chain_long_kernel_stats.csv).
python scripts/chain_long_probe.py [--reads N] [--ref-bp B] [--reps R] [--threads T] [--device-only] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED_DTYPE = np.dtype([("key", "<u4"), ("target_position", "<u4"), ("query_position", "<u4")])
REC_DTYPE = np.dtype([("chaining_score", "<f4"), ("key", "<u4"), ("start_position", "<u4"), ("end_position", "<u4"), ("n_anchors", "<u4")])


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=16384)
    ap.add_argument("--ref-bp", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--events", type=int, default=400)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import rawalign_amd as ra
    from rawalign_amd import mapping as M
    from rawalign_amd import seeding, synth
    from rawalign_amd.dtw import ANCHOR_DTYPE
    from scripts.round_resident_probe import make_reads

    rng = np.random.default_rng(20241101)
    ref = synth.make_reference([a.ref_bp], seed=20241017)
    six = seeding.SeedIndex.from_signals(ref.forward, ref.reverse, threads=a.threads)
    n = a.reads
    reads = make_reads(ref, n, rng, events=a.events)
    eng = ra.Engine(0)
    lib = eng.lib
    copt = M.default_chain_opt(6)
    vp = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731

    def device_round(seed_off, seeds):
        cap = n * 32
        out = dict(chain_off=np.zeros(n + 1, np.uint64), anchor_off=np.zeros(cap + 1, np.uint64), recs=np.zeros(cap, REC_DTYPE),
                   anchors=np.zeros(int(seed_off[-1]) + 1, ANCHOR_DTYPE))
        read_base, key_base = np.zeros(n, np.uint32), np.zeros(2, np.uint64)
        d = [C.c_void_p() for _ in range(3)]
        eng.sync()
        t = time.perf_counter()
        st = lib.rawdtw_chain_round(eng._ctx, C.byref(copt), n, vp(seed_off), vp(seeds), vp(read_base), 2, vp(key_base), vp(out["chain_off"]), vp(out["anchor_off"]),
                                    vp(out["recs"]), cap, vp(out["anchors"]), *[C.byref(x) for x in d])
        ms = (time.perf_counter() - t) * 1e3
        return st, ms, out

    def host_lists(seed_off, seeds):
        """every read's lists, sorted and split (outside the time)"""
        per = []
        for r in range(n):
            s = seeds[int(seed_off[r]):int(seed_off[r + 1])]
            s = s[np.lexsort((s["query_position"], s["target_position"], s["key"]))]
            cut = np.flatnonzero(np.diff(s["key"])) + 1
            lists = []
            for g in np.split(s, cut) if len(s) else []:
                an = np.zeros(len(g), ANCHOR_DTYPE)
                an["target_position"], an["query_position"] = g["target_position"], g["query_position"]
                lists.append((int(g["key"][0]), an))
            per.append(lists)
        return per

    def host_read(lists):
        maxs, chains = 0.0, []
        for key, an in lists:
            cs, maxs = M.chain_anchors(an, copt, maxs, key >> 1, key & 1)
            chains += [(c, key) for c in cs]
        if chains:
            sc = np.array([c.chaining_score for c, _ in chains], np.float32)
            perm = np.zeros(len(sc), np.uint32)
            lib.rawdtw_sort_by_chaining_score(vp(sc), len(sc), vp(perm))
            chains = [chains[p] for p in perm]
        return chains

    pool = ThreadPoolExecutor(a.threads)

    def host_round(per):
        t = time.perf_counter()
        res = list(pool.map(host_read, per, chunksize=max(1, n // (a.threads * 8))))
        return (time.perf_counter() - t) * 1e3, res

    # the two rounds' seed lists: hits; then the first round's chains' anchors and the second chunk's hits
    rounds, prev = [], None
    for c in range(2):
        chunks = [r[c] for r in reads]
        ev = np.concatenate(chunks)
        off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.uint64)
        hoff, hits = seeding.seed_hits_host(six, ev, off, threads=a.threads)
        hoff = hoff.astype(np.int64)
        hs = np.zeros(len(hits), SEED_DTYPE)
        hs["key"] = hits["ref_seq"] * 2 + (hits["strand"] != 0)
        hs["target_position"], hs["query_position"] = hits["target_position"], hits["query_position"] + np.uint32(c * a.events)
        per = []
        for r in range(n):
            mine = hs[hoff[r]:hoff[r + 1]]
            per.append(np.concatenate([prev[r], mine]) if prev is not None else mine)
        seed_off = np.concatenate([[0], np.cumsum([len(s) for s in per])]).astype(np.uint64)
        seeds = np.concatenate(per + [np.zeros(1, SEED_DTYPE)])
        lens = np.diff(seed_off.astype(np.int64))
        say("round %d: %d seeds, %.0f a read, at most %d; %d reads above 2048" % (c + 1, int(seed_off[-1]), lens.mean(), lens.max(), int((lens > 2048).sum())))
        rounds.append(dict(seed_off=seed_off, seeds=seeds, lens=lens))
        if c == 0:   # round 1's chains, from the device with the option on, as the next round's first seeds
            eng.set_option("chain_long_seeds", 1 << 20)
            st, _, out = device_round(seed_off, seeds)
            assert st == 0, lib.rawdtw_last_error(eng._ctx)
            prev = []
            for r in range(n):
                c0, c1 = int(out["chain_off"][r]), int(out["chain_off"][r + 1])
                an = out["anchors"][int(out["anchor_off"][c0]):int(out["anchor_off"][c1])]
                s = np.zeros(len(an), SEED_DTYPE)
                s["key"] = np.repeat(out["recs"]["key"][c0:c1], out["recs"]["n_anchors"][c0:c1].astype(np.int64))
                s["target_position"], s["query_position"] = an["target_position"], an["query_position"]
                prev.append(s)
    if a.device_only:
        eng.set_option("chain_long_seeds", 1 << 20)
        for _ in range(3):
            for rd in rounds:
                assert device_round(rd["seed_off"], rd["seeds"])[0] == 0
        eng.close()
        return
    rec = {"probe": "chain_long", "reads": n, "reference_bp": a.ref_bp, "reps": a.reps, "host_threads": a.threads, "rounds": []}
    ok = True
    for c, rd in enumerate(rounds):
        short_only = bool(rd["lens"].max() <= 2048)
        per = host_lists(rd["seed_off"], rd["seeds"])
        runs = {"device_on_ms": [], "device_off_ms": [], "host_ms": []}
        before = eng.chain_round_stats()
        for rep in range(a.reps + 1):   # (the first is the warm-up)
            eng.set_option("chain_long_seeds", 1 << 20)
            st, on_ms, out = device_round(rd["seed_off"], rd["seeds"])
            assert st == 0, lib.rawdtw_last_error(eng._ctx)
            off_ms = None
            if short_only:
                eng.set_option("chain_long_seeds", 0)
                st, off_ms, _ = device_round(rd["seed_off"], rd["seeds"])
                assert st == 0
            h_ms, res = host_round(per)
            if rep:
                runs["device_on_ms"].append(round(on_ms, 3)); runs["host_ms"].append(round(h_ms, 3))
                if off_ms is not None:
                    runs["device_off_ms"].append(round(off_ms, 3))
        stats = eng.chain_round_stats()
        # the device's chains are the host's: count, order, score bits
        same = True
        for r in range(n):
            c0, c1 = int(out["chain_off"][r]), int(out["chain_off"][r + 1])
            want = np.array([ch.chaining_score for ch, _ in res[r]], np.float32)
            same = same and c1 - c0 == len(want) and bool((out["recs"]["chaining_score"][c0:c1].view(np.uint32) == want.view(np.uint32)).all())
        ok = ok and same
        med = {k: (round(float(np.median(v)), 3) if v else None) for k, v in runs.items()}
        rec["rounds"].append(dict(seeds=int(rd["seed_off"][-1]), mean_seeds_a_read=round(float(rd["lens"].mean()), 1), max_seeds_a_read=int(rd["lens"].max()),
                                  reads_above_cap=int((rd["lens"] > 2048).sum()), median=med, runs=runs, same_chains_as_host=same,
                                  host_over_device=round(med["host_ms"] / med["device_on_ms"], 3),
                                  long_reads_a_round=(stats["long_reads"] - before["long_reads"]) // (a.reps + 1),
                                  far_steps_a_round=(stats["far_steps"] - before["far_steps"]) // (a.reps + 1)))
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
