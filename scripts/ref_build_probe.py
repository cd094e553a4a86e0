"""Where the time of a reference build goes: the signals and the seed table of a synthetic genome, on the device and on the host of the
same commit, in one run.  Medians of --reps after a warm-up of every path; the two sides alternate inside a repetition.  A number is
device time where it comes from HIP events (the launches, the sort) and host time around a synchronised call everywhere else.
  device   rawdtw_reference_from_bases as a whole, its two launches, the steps that went fast and slow;
           rawdtw_seed_index_build_device as a whole and its phases: filter, emit, sort, entries home, fill_table
  host     rawdtw_seq_to_sig_host for both strands on --threads threads + rawdtw_upload_reference; rawdtw_seed_index_build on --threads
With --w N above 0 the table is a minimizer index's: rawdtw_seed_index_build_device_min against rawdtw_seed_index_build at that w, the
emit phase split into its three selection launches (hash, count + scan, write), and the entries an e-mer.
The device's outputs are compared with the host's once, bit for bit, before anything is timed.
With --resident the question is another: from a reference on the device to a table the seeding kernels read, by (a) the path that brings
the entries home -- rawdtw_seed_index_build_device[_min], then rawdtw_seed_index_upload -- and (b) rawdtw_seed_index_build_resident,
alternating in one run.  Both totals, every phase of both, (a)'s min-max spread, and the three tiled filter launches beside k_sb_filter.
Usage: python scripts/ref_build_probe.py [--bp 4600000] [--reps 7] [--w 0] [--resident]
       [--out profiles/ref_build_probe.json, ref_build_probe_wN.json for --w N; with --resident ref_build_resident.json, ref_build_resident_wN.json]"""
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


def resident(a):
    """(a) build_device[_min] + upload against (b) build_resident on one engine and one reference"""
    bases = np.frombuffer(b"ACGT", np.uint8)[synth.make_genome(a.bp, 4600)].tobytes()
    pore, pars = synth.make_pore_model(a.k), SeedParams(w=a.w, k=a.k)
    dev = ra.Engine(0)
    dev.set_option("seed_minimizer", 1)
    dev.reference_from_bases([bases], pore, a.k, True)
    fwd, rev = dev.reference_fetch(0, 1), dev.reference_fetch(0, 0)
    rng = np.random.default_rng(46)
    chunks = [(x[lo:lo + 300] + rng.normal(0, 0.03, 300)).astype(np.float32) for x in (fwd, rev) for lo in rng.integers(0, len(x) - 300, 32).tolist()]
    ev, off = np.concatenate(chunks), np.arange(len(chunks) + 1, dtype=np.uint64) * 300
    names_a = ("filter", "emit", "sort", "home", "fill_table")
    names_b = ("next", "chain", "mark", "emit", "sort", "table")
    t = {k: [] for k in ("a_total", "a_build", "a_upload", "b_total") + tuple("a_" + k for k in names_a) + tuple("b_" + k for k in names_b)}
    for it in range(-1, a.reps):  # it -1: the warm-up, and the comparison
        t0 = time.perf_counter()
        six_a = SeedIndex.from_device(dev, pars, minimizer=a.w > 0)
        t1 = time.perf_counter()
        dev.upload_seed_index(six_a)
        t2 = time.perf_counter()
        ph = dev.seed_build_stats()
        hits_a = dev.seed_hits(ev, off) if it < 0 else None
        t3 = time.perf_counter()
        six_b = SeedIndex.from_device(dev, pars, resident=True)
        t4 = time.perf_counter()
        st = dev.seed_build_resident_stats()
        if it < 0:
            hits_b = dev.seed_hits(ev, off)
            assert np.array_equal(hits_a[0], hits_b[0]) and hits_a[1].tobytes() == hits_b[1].tobytes() and len(hits_a[1]) > len(chunks), "hits differ"
            six_b.fetch(dev)
            assert (six_a.n_keys, six_a.n_positions, six_a.table_bytes) == (six_b.n_keys, six_b.n_positions, six_b.table_bytes), "tables differ"
            assert np.array_equal(six_a.keys(), six_b.keys()), "tables differ"
            for h in six_a.keys()[::97].tolist():
                assert np.array_equal(six_a.get(h), six_b.get(h)), "tables differ"
        else:
            t["a_total"].append((t2 - t0) * 1e3); t["a_build"].append((t1 - t0) * 1e3); t["a_upload"].append((t2 - t1) * 1e3)
            t["b_total"].append((t4 - t3) * 1e3)
            for k in names_a:
                t["a_" + k].append(ph[k + "_ms"])
            for k in names_b:
                t["b_" + k].append(st[k + "_ms"])
        info = {"keys": six_a.n_keys, "positions": six_a.n_positions, "table_bytes": six_a.table_bytes}
        six_a.close(); six_b.close()
    spread = max(t["a_total"]) - min(t["a_total"])
    tiled = med(np.add(np.add(t["b_next"], t["b_chain"]), t["b_mark"]))
    rec = {
        "what": "scripts/ref_build_probe.py --resident: ms, medians of %d after a warm-up, (a) and (b) alternating in one run; outputs compared first" % a.reps,
        "bases": a.bp, "k": a.k, "w": a.w, "signals_a_strand": len(fwd), **info,
        "tile": st["tile"], "tiles": st["tiles"], "kept": st["kept"], "entries": st["entries"], "keys_not_in_their_home_slot": st["displaced"],
        "a_build_device_then_upload": {"total_ms": med(t["a_total"]), "min_ms": round(min(t["a_total"]), 3), "max_ms": round(max(t["a_total"]), 3),
                                       "spread_ms": round(spread, 3), "build_ms": med(t["a_build"]), "upload_ms": med(t["a_upload"]),
                                       **{k + "_ms": med(t["a_" + k]) for k in names_a}},
        "b_build_resident": {"total_ms": med(t["b_total"]), "min_ms": round(min(t["b_total"]), 3), "max_ms": round(max(t["b_total"]), 3),
                             **{k + "_ms": med(t["b_" + k]) for k in names_b}},
        "filter": {"k_sb_filter_ms": med(t["a_filter"]), "tiled_three_launches_ms": tiled, "tiled_is_faster": bool(tiled < med(t["a_filter"]))},
        "b_below_a_by_more_than_a_spread": bool(med(t["a_total"]) - med(t["b_total"]) > spread),
        "all_reps": {k: [round(float(x), 3) for x in v] for k, v in t.items()},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "all_reps"}))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bp", type=int, default=4_600_000)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--w", type=int, default=0, help="minimizer windows of this many e-mers (0: every e-mer)")
    ap.add_argument("--resident", action="store_true", help="build_device[_min] + upload against build_resident")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.resident:
        if a.out is None:
            a.out = os.path.join(ROOT, "profiles", "ref_build_resident_w%d.json" % a.w if a.w else "ref_build_resident.json")
        return resident(a)
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
