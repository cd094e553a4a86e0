#!/usr/bin/env python3
"""The round's end on the device ("device_round_end") against the round's end on the host, in one process: the benchmark's mapper
round -- --reads reads (16 384) of the 4.6 Mb workload, their first chunk, chaining on the device, one read group, the reference's stop
rule (max_num_chunk = 1, so that every read is finished after the round and can be released) -- on two mappers that differ in the option alone, taken in turns.  Per repetition (fresh reads every time, after two warm-ups):
  round_ms        rawdtw_mapper_round, host wall time
  round_end_ms    the mapper's timing slot for the round's end (rawdtw_mapper_timing slot 4: after the fetch, until the commit)
  fetch_wait_ms   the slot in front of it (the wait for the batch; with the option on also the round end's results)
  kernel_us       k_round_end between its HIP events ("round_end_kernel_us"; option on only)
Medians and every run; the lines of both mappers must be the same.  Prints one JSON line (profiles/round_end_probe.json).
python scripts/round_end_probe.py [--reads N] [--genome B] [--reps R] [--threads T] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20231005 + 2   # (bench.py's)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=16384)
    ap.add_argument("--genome", type=int, default=4_600_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import rawalign_amd as ra
    from rawalign_amd import mapper, synth
    from rawalign_amd.mapping import StopOpt

    n = a.reads
    ref = synth.make_reference([a.genome], seed=SEED)
    sc = synth.make_seed_chunks(ref, n, seed=SEED + 17)
    names, lens = [f"seq{s}" for s in range(ref.n_seq)], [len(x) for x in ref.forward]
    slot = int(sc["n_ev"].max()) + 8
    first = sc["chunk_first"][:n].astype(np.int64)
    ev_off, hit_off = sc["ev_off"].astype(np.int64), sc["hit_off"].astype(np.int64)
    # the round: every read's first chunk, the events in page-locked memory as bench.py hands them over
    ecnt, hcnt = ev_off[first + 1] - ev_off[first], hit_off[first + 1] - hit_off[first]
    eo = np.concatenate([[0], np.cumsum(ecnt)]).astype(np.uint64)
    ho = np.concatenate([[0], np.cumsum(hcnt)]).astype(np.uint64)
    eidx = np.repeat(ev_off[first], ecnt) + (np.arange(int(eo[-1])) - np.repeat(eo[:-1].astype(np.int64), ecnt))
    hidx = np.repeat(hit_off[first], hcnt) + (np.arange(int(ho[-1])) - np.repeat(ho[:-1].astype(np.int64), hcnt))
    lib = ra.load_library()
    p = C.c_void_p()
    assert lib.rawdtw_host_alloc((int(eo[-1]) + 1) * 4, C.byref(p)) == 0
    ev = np.frombuffer((C.c_char * ((int(eo[-1]) + 1) * 4)).from_address(p.value), np.float32)
    np.take(sc["events"], eidx, out=ev[:len(eidx)])
    hits = np.ascontiguousarray(sc["hits"][hidx])

    side = {}
    for on in (0, 1):
        eng = ra.Engine(0)
        eng.upload_reference(ref.forward, ref.reverse)
        eng.set_option("device_round_end", on)
        cm = mapper.CMapper(eng, ra.MapOpt(), StopOpt(max_num_chunk=1), names, lens, slot_events=slot, max_reads=n, carry=False, threads=a.threads, groups=1, device_chain=True)
        side[on] = dict(eng=eng, cm=cm, runs=dict(round_ms=[], round_end_ms=[], fetch_wait_ms=[], kernel_us=[]))

    def one(on, keep):
        s = side[on]
        cm = s["cm"]
        ids = np.array([cm.add_read("read_%d" % r, int(sc["qlen"][r]), int(sc["n_chunks"][r])) for r in range(n)], np.uint32)
        t0 = cm.timing()
        t = time.perf_counter()
        cm.round_arrays(ids, eo, ev, ho, hits)
        ms = (time.perf_counter() - t) * 1e3
        t1 = cm.timing()
        if keep:
            s["runs"]["round_ms"].append(round(ms, 3))
            s["runs"]["round_end_ms"].append(round(t1["round_end_ms"] - t0["round_end_ms"], 3))
            s["runs"]["fetch_wait_ms"].append(round(t1["fetch_wait_ms"] - t0["fetch_wait_ms"], 3))
            if on:
                s["runs"]["kernel_us"].append(s["eng"].get_option("round_end_kernel_us"))
        assert cm.finish() == 0
        lines = [cm.paf(int(i)) for i in ids]
        for i in ids:
            cm.release_read(int(i))
        return lines

    same = True
    for rep in range(a.reps + 2):   # (the first two are warm-ups: the pinned buffers and workspaces reach their sizes)
        res = [one(on, rep >= 2) for on in ((0, 1) if rep % 2 == 0 else (1, 0))]
        same = same and res[0] == res[1]
    st = side[1]["cm"].round_end_stats()
    rec = {"probe": "round_end", "reads": n, "genome_bp": a.genome, "reps": a.reps, "host_threads": a.threads, "groups": 1,
           "mapped_after_the_round": int(sum(1 for ln in res[0] if ln.split("\t")[4] in "+-")), "same_lines": same,
           "reads_device_a_round": st["reads_device"] // (a.reps + 2), "reads_declined_a_round": st["reads_declined"] // (a.reps + 2)}
    for on in (0, 1):
        runs = side[on]["runs"]
        rec["option_on" if on else "option_off"] = {"median": {k: round(float(np.median(v)), 3) for k, v in runs.items() if v}, "runs": {k: v for k, v in runs.items() if v}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for s in side.values():
        s["cm"].close()
        s["eng"].close()
    lib.rawdtw_host_free(p)
    if not same:
        sys.exit("the lines differ with the option on")


if __name__ == "__main__":
    main()
