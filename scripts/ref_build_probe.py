"""Where the time of a reference build goes: the signals and the seed table of a synthetic genome, on the device and on the host of the
same commit, in one run.  Medians of --reps after a warm-up of every path; the two sides alternate inside a repetition.  A number is
device time where it comes from HIP events (the launches, the sort) and host time around a synchronised call everywhere else.
  device   rawdtw_reference_from_bases as a whole, its two launches, the steps that went fast and slow;
           rawdtw_seed_index_build_device as a whole and its phases: filter, emit, sort, entries home, fill_table
  host     rawdtw_seq_to_sig_host for both strands on --threads threads + rawdtw_upload_reference; rawdtw_seed_index_build on --threads
With --w N above 0 the table is a minimizer index's: rawdtw_seed_index_build_device_min against rawdtw_seed_index_build at that w, the
emit phase split into its three selection launches (hash, count + scan, write), and the entries an e-mer.
The device's outputs are compared with the host's once, bit for bit, before anything is timed.
Usage: python scripts/ref_build_probe.py [--bp 4600000] [--reps 7] [--w 0] [--out profiles/ref_build_probe.json, ref_build_probe_wN.json for --w N]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rawalign_amd as ra  # noqa: E402
from rawalign_amd import refsig, synth  # noqa: E402
from rawalign_amd.seeding import SeedIndex, SeedParams  # noqa: E402


def med(xs):
    return round(float(np.median(xs)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bp", type=int, default=4_600_000)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--w", type=int, default=0, help="minimizer windows of this many e-mers (0: every e-mer)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "ref_build_probe_w%d.json" % a.w if a.w else "ref_build_probe.json")
    bases = np.frombuffer(b"ACGT", np.uint8)[synth.make_genome(a.bp, 4600)].tobytes()
    pore, pars = synth.make_pore_model(a.k), SeedParams(w=a.w, k=a.k)
    dev, hst = ra.Engine(0), ra.Engine(0)
    pool = ThreadPoolExecutor(a.threads)

    def host_signals():
        # (a strand is one serial recurrence: two strands are all the parallelism one sequence has, whatever the thread count)
        f = [pool.submit(refsig.seq_to_sig, bases, pore, a.k, strand, True) for strand in (1, 0)]
        return f[0].result(), f[1].result()

    t = {k: [] for k in ("dev_ref", "dev_sums", "dev_write", "host_sig", "host_upload", "dev_table", "filter", "emit", "sort", "home", "fill_table",
                         "host_table", "hash", "count_scan", "write")}
    fwd, rev = host_signals()
    for rep in range(-1, a.reps):  # rep -1: the warm-up, and the comparison
        t0 = time.perf_counter()
        dev.reference_from_bases([bases], pore, a.k, True)
        t1 = time.perf_counter()
        st = dev.reference_build_stats()
        t2 = time.perf_counter()
        fwd, rev = host_signals()
        t3 = time.perf_counter()
        hst.upload_reference([fwd], [rev])
        t4 = time.perf_counter()
        six_d = SeedIndex.from_device(dev, pars, minimizer=a.w > 0)
        t5 = time.perf_counter()
        ph = dev.seed_build_stats()
        sel = dev.seed_build_min_stats() if a.w else None
        t6 = time.perf_counter()
        six_h = SeedIndex.from_signals([fwd], [rev], pars, threads=a.threads)
        t7 = time.perf_counter()
        if rep < 0:
            assert dev.reference_fetch(0, 1).tobytes() == fwd.tobytes() and dev.reference_fetch(0, 0).tobytes() == rev.tobytes(), "signals differ"
            assert (six_d.n_keys, six_d.n_positions) == (six_h.n_keys, six_h.n_positions) and np.array_equal(six_d.keys(), six_h.keys()), "tables differ"
            for h in six_h.keys()[::997].tolist():
                assert np.array_equal(six_d.get(h), six_h.get(h)), "tables differ"
        else:
            for k, v in (("dev_ref", t1 - t0), ("host_sig", t3 - t2), ("host_upload", t4 - t3), ("dev_table", t5 - t4), ("host_table", t7 - t6)):
                t[k].append(v * 1e3)
            t["dev_sums"].append(st["sums_ms"]); t["dev_write"].append(st["write_ms"])
            for k in ("filter", "emit", "sort", "home", "fill_table"):
                t[k].append(ph[k + "_ms"])
            for k in ("hash", "count_scan", "write"):
                t[k].append(sel[k + "_ms"] if sel else 0.0)
        info = {"keys": six_d.n_keys, "positions": six_d.n_positions}
        six_d.close(); six_h.close()
    steps = (len(fwd) + 63) // 64 * 2
    rec = {
        "what": "scripts/ref_build_probe.py: ms, medians of %d after a warm-up; device and host of one commit in one run" % a.reps,
        "bases": a.bp, "k": a.k, "signals_a_strand": len(fwd), "host_threads": a.threads, **info,
        "reference": {
            "device_from_bases_ms": med(t["dev_ref"]), "device_sums_launch_ms": med(t["dev_sums"]), "device_write_launch_ms": med(t["dev_write"]),
            "steps_a_sum": steps, "fast_steps": [int(x) for x in st["fast_steps"]], "slow_steps": [int(x) for x in st["slow_steps"]],
            "host_seq_to_sig_ms": med(t["host_sig"]), "host_upload_reference_ms": med(t["host_upload"]),
            "host_total_ms": med(np.add(t["host_sig"], t["host_upload"])),
        },
        "seed_table": {
            "device_build_ms": med(t["dev_table"]), "filter_ms": med(t["filter"]), "emit_ms": med(t["emit"]), "sort_ms": med(t["sort"]),
            "entries_home_ms": med(t["home"]), "fill_table_ms": med(t["fill_table"]), "host_build_ms": med(t["host_table"]),
        },
        **({"selection": {"w": a.w, "emers": sel["emers"], "entries": sel["entries"], "entries_an_emer": round(sel["entries"] / max(sel["emers"], 1), 4),
                          "hash_ms": med(t["hash"]), "count_scan_ms": med(t["count_scan"]), "write_ms": med(t["write"])}} if sel else {}),
        "all_reps": {k: [round(float(x), 3) for x in v] for k, v in t.items()},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: rec[k] for k in ("reference", "seed_table", "selection") if k in rec}))
    dev.close(); hst.close()


if __name__ == "__main__":
    main()
