#!/usr/bin/env python3
""""chain_decline_reads" off against on, in one process on the same inputs: one resident chunk round of 16 384 reads (first chunks of about
400 events, noisy stretches of both strands of a synthetic reference -- scripts/round_resident_probe.py's workload) with k = 0, 1, 16 and 256
reads above the device chaining's cap on seeds a read.  The reads' hit counts are what they are; k reads are put above the cap by lowering it
(RAWDTW_CHAIN_MAX_SEEDS, read when a context is created) to the (k + 1)-th largest count, so that exactly the k largest reads are above
it.  For each k two engines under that cap, the option off (the parent's behaviour: with k >= 1 the whole round falls back to the host) and on;
each repetition maps the round on a fresh mapper; medians of --reps repetitions after a warm-up, with every run listed.
Prints one JSON line (profiles/chain_decline_probe.json), per k and side:
  round_ms             host wall time of rawdtw_mapper_round_seeded_resident
  host_phase_ms        rawdtw_mapper_timing's slots 0 and 1 (the host's chaining of a fall-back round is in slot 0; the declined reads' is in slot 2's lap)
  submit_ms            slot 2: submissions and waits up to the batch's submission, the declined reads' chaining and append included
  bytes_to_host        the round's hits fetched by a fall-back + the declined reads' seeds
  counters             rawdtw_mapper_resident_stats and rawdtw_mapper_decline_stats
and, at the level of the chaining round alone (rawdtw_chain_round on the same reads' seed lists built on the host), between HIP events on
the context's stream:
  chain_round_ms       the whole round with the option off (k = 0 only: with k >= 1 it is refused) and on; every run in chain_round_runs_ms
  declined_seeds_ms    rawdtw_chain_round_declined_seeds: k_declined_seeds and its wait
  checks               the same PAF lines from both sides; no fall-back and no hit byte home with the option on; the declined reads are the k largest
python scripts/chain_decline_probe.py [--reads N] [--ref-bp B] [--reps R] [--ks 0,1,16,256] [--on-first] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=16384)
    ap.add_argument("--ref-bp", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ks", default="0,1,16,256")
    ap.add_argument("--on-first", action="store_true", help="each repetition runs the option-on side before the option-off one (an order effect shows as a change of sign)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import rawalign_amd as ra
    from rawalign_amd import mapper, seeding, synth
    from rawalign_amd import mapping as M
    from rawalign_amd.dtw import ANCHOR_DTYPE, CHAIN_REC_DTYPE, SEED_DTYPE
    from rawalign_amd.events import PinnedArray
    from rawalign_amd.mapping import StopOpt
    from round_resident_probe import make_reads

    rng = np.random.default_rng(20241101)
    ref = synth.make_reference([a.ref_bp], seed=20241017)
    six = seeding.SeedIndex.from_signals(ref.forward, ref.reverse, threads=16)
    n = a.reads
    chunks = [r[0] for r in make_reads(ref, n, rng, chunks=1)]
    N = sum(len(x) for x in chunks)
    ev, off = PinnedArray(N + 1, np.float32), PinnedArray(n + 1, np.uint64)
    ev.array[:N] = np.concatenate(chunks)
    off.array[:n + 1] = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.uint64)
    hoff, hits = seeding.seed_hits_host(six, ev.array[:N], off.array[:n + 1], threads=16)
    counts = np.diff(hoff.astype(np.int64))
    say("%d reads, %d events, %d hits, at most %d a read" % (n, N, int(hoff[-1]), int(counts.max())))
    assert counts.max() <= 2048, "a read above the device's own cap: use a smaller reference"
    order = np.sort(counts)[::-1]
    seeds = np.zeros(len(hits) + 1, SEED_DTYPE)   # the round's seed lists as the mapper's host phase builds them (first chunks: no previous anchors)
    seeds["key"][:-1] = hits["ref_seq"] * 2 + (hits["strand"] != 0)
    seeds["target_position"][:-1], seeds["query_position"][:-1] = hits["target_position"], hits["query_position"]
    seed_off = hoff.astype(np.uint64)
    opt, copt = ra.MapOpt(), M.default_chain_opt(6)
    stop = StopOpt(min_bestmap_ratio=1e9, min_meanmap_ratio=1e9, min_chain_anchor=10 ** 6)
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    def between_events(eng, fn):
        s = C.c_void_p(eng.stream_handle())
        assert hip.hipEventRecord(ev0, s) == 0
        out = fn()
        assert hip.hipEventRecord(ev1, s) == 0 and hip.hipEventSynchronize(ev1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        return float(ms.value), out

    def engine(cap, on):
        os.environ["RAWDTW_CHAIN_MAX_SEEDS"] = str(cap)
        try:
            e = ra.Engine(0)
        finally:
            del os.environ["RAWDTW_CHAIN_MAX_SEEDS"]
        e.set_option("device_round_end", 1)
        e.set_option("resident_chains", 4096)
        e.set_option("chain_decline_reads", int(on))
        e.upload_reference(ref.forward, ref.reverse)
        e.upload_seed_index(six)
        return e

    def one(eng):
        cm = mapper.CMapper(eng, opt, stop, ["synth_0"], [len(ref.forward[0])], slot_events=1024, max_reads=n, threads=16, carry=False, device_chain=True)
        ids = np.array([cm.add_read("r%d" % r, 8000, 2) for r in range(n)], np.uint32)
        eng.sync()
        t = time.perf_counter()
        st = eng.lib.rawdtw_mapper_round_seeded_resident(cm._h, six._h, n, ids.ctypes.data, off.ptr, ev.ptr)
        ms = (time.perf_counter() - t) * 1e3
        assert st == 0, eng.lib.rawdtw_mapper_last_error(cm._h)
        tm, res, dcs = cm.timing(), cm.resident_stats(), cm.decline_stats()
        lines = [cm.paf(int(i)) for i in ids[:512]]
        cm.close()
        return dict(round_ms=ms, host_phase_ms=tm["host_phase_ms"] + tm["layout_ms"], submit_ms=tm["submit_ms"],
                    bytes_to_host=res["hit_bytes_to_host"] + dcs["seed_bytes_to_host"], resident=res, decline=dcs), lines

    cap_chains = max(n * 32, int(seed_off[-1]) // 2 + 1)
    outs = (np.zeros(n + 1, np.uint64), np.zeros(cap_chains + 1, np.uint64), np.zeros(cap_chains, CHAIN_REC_DTYPE), np.zeros(int(seed_off[-1]) + 1, ANCHOR_DTYPE))
    read_base = (np.arange(n, dtype=np.uint32) * 1024).astype(np.uint32)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731

    def chain_round(eng):
        key_base = np.array([eng.reference_offset(0, st) for st in (0, 1)], np.uint64)
        d = [C.c_void_p() for _ in range(3)]
        return eng.lib.rawdtw_chain_round(eng._ctx, C.byref(copt), n, vp(seed_off), vp(seeds), vp(read_base), 2, vp(key_base), vp(outs[0]), vp(outs[1]), vp(outs[2]),
                                          cap_chains, vp(outs[3]), *[C.byref(x) for x in d])

    med = lambda xs: round(float(np.median(xs)), 3)  # noqa: E731
    rec = {"probe": "chain_decline", "reads": n, "reference_bp": a.ref_bp, "events": N, "hits": int(hoff[-1]), "max_hits_a_read": int(counts.max()),
           "reps": a.reps, "on_first": a.on_first, "k": {}}
    checks = {}
    for k in [int(x) for x in a.ks.split(",")]:
        cap = int(order[k]) if k < n else 1   # (the k largest counts are above it, unless counts tie at the boundary)
        k_real = int((counts > cap).sum())
        engs = {False: engine(cap, False), True: engine(cap, True)}
        for on in (False, True):
            one(engs[on])   # warm-up: workspaces, page-locked buffers
        runs = {False: [], True: []}
        for _ in range(a.reps):
            for on in ((True, False) if a.on_first else (False, True)):
                runs[on].append(one(engs[on]))
        side = {}
        for on in (False, True):
            rs = [r[0] for r in runs[on]]
            side["on" if on else "off"] = dict(round_ms=med([r["round_ms"] for r in rs]), host_phase_ms=med([r["host_phase_ms"] for r in rs]),
                                               submit_ms=med([r["submit_ms"] for r in rs]), bytes_to_host=rs[-1]["bytes_to_host"],
                                               runs_round_ms=[round(r["round_ms"], 3) for r in rs], resident=rs[-1]["resident"], decline=rs[-1]["decline"])
        off_runs = side["off"]["runs_round_ms"]
        side["off_spread_ms"] = round(max(off_runs) - min(off_runs), 3)
        # the chaining round alone, between HIP events
        cr = {"off": [], "on": [], "declined_seeds_ms": []}
        for _ in range(a.reps + 1):
            if k_real == 0:
                ms, st = between_events(engs[False], lambda: chain_round(engs[False]))
                assert st == 0
                cr["off"].append(ms)
            ms, st = between_events(engs[True], lambda: chain_round(engs[True]))
            assert st == 0, engs[True].lib.rawdtw_last_error(engs[True]._ctx)
            cr["on"].append(ms)
            got_reads, _ = engs[True].chain_round_declined()
            if k_real:
                ms, _ = between_events(engs[True], lambda: engs[True].chain_round_declined_seeds(int(counts[got_reads].sum())))
                cr["declined_seeds_ms"].append(ms)
        side["chain_round_ms"] = {s: (med(v[1:]) if v else None) for s, v in cr.items()}   # (the first is the warm-up)
        side["chain_round_runs_ms"] = {s: [round(x, 3) for x in v[1:]] for s, v in cr.items()}
        rec["k"][str(k)] = dict(side, cap=cap, reads_above_cap=k_real)
        checks["k%d_same_lines" % k] = runs[False][-1][1] == runs[True][-1][1]
        checks["k%d_on_stays_resident" % k] = side["on"]["resident"]["fallback_rounds"] == 0 and side["on"]["resident"]["hit_bytes_to_host"] == 0
        checks["k%d_off_falls_back_iff_a_read_is_above" % k] = (side["off"]["resident"]["fallback_rounds"] == 1) == (k_real > 0)
        checks["k%d_declined_are_the_reads_above" % k] = sorted(got_reads.tolist()) == sorted(np.flatnonzero(counts > cap).tolist())
        checks["k%d_seed_bytes" % k] = side["on"]["decline"]["seed_bytes_to_host"] == 12 * int(counts[counts > cap].sum())
        say("k = %d (cap %d, %d above): off %.2f ms, on %.2f ms" % (k, cap, k_real, side["off"]["round_ms"], side["on"]["round_ms"]))
        for e in engs.values():
            e.close()
    rec["checks"] = checks
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(checks.values()):
        sys.exit("a check failed: %s" % checks)


if __name__ == "__main__":
    main()
