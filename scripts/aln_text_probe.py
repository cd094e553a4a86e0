#!/usr/bin/env python3
"""aln:s: made on the device (include/rawdtw.h, "aln text"; rawdtw_mapper_set_device_text): what rawdtw_mapper_finish costs with the
setter off -- steps and distances home, the host formatter (rawdtw_aln_text_host) over them -- and on, on the benchmark's cigar workload:
bench.py's reference (the S. cerevisiae chromosome lengths) and its synthetic reads (synth.SynthParams(max_chunks=6)), global border
constraint + full fill, flag 0x4, mapped by the library's mapper until every read stopped; the finish alone is timed.
Method: fresh mappers, off and on alternating in one process; one of each as a warm-up, then seven of each; the figure is the median of
the seven with their minimum and maximum.  The yardstick is the off arm of the same run.  It records count_ms / write_ms of the on arm's
last finish (rawdtw_aln_text_timing), the text bytes that came home against 5 bytes an element, the off arm's host time an element
(finish less the traceback kernels), and the registers and scratch of the three kernels when --resource-usage names a file with hipcc's
-Rpass-analysis=kernel-resource-usage remarks of rawdtw_aln_text.hip.  Check that must hold whatever the times are: both arms print the
same PAF lines.  A probe, not a threshold: nothing is asserted of a time.  Prints one JSON line (profiles/aln_text_probe.json).
python scripts/aln_text_probe.py [--reads N] [--threads T] [--resource-usage FILE] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 7


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def kernel_resources(path):
    """{kernel: {vgprs, sgprs, scratch_bytes_a_lane, lds_bytes}} from hipcc's kernel-resource-usage remarks"""
    out, name = {}, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            s = m.group(1)
            name = "k_aln_scan" if "k_aln_scan" in s else "k_aln_write" if "ILb1E" in s else "k_aln_count" if "ILb0E" in s else s
            out[name] = {}
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch_bytes_a_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, ln)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--resource-usage", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch  # noqa: F401  (first: PyTorch bundles its own HIP runtime)

    import bench
    import rawalign_amd as ra
    from rawalign_amd import mapper, synth
    from rawalign_amd.mapping import StopOpt

    n = a.reads
    ref = synth.make_reference(bench.YEAST, seed=20231005 + 3)
    made = mapper.SyntheticSeeds(ref, n, seed=77, max_chunks=6)

    class Seeds:
        """the synthetic reads with every chunk built once: sixteen mappers are fed the same arrays"""
        reads = made.reads

        def __init__(self):
            self.cache = {}

        def read_job(self, r):
            return made.read_job(r)

        def chunk(self, r, c):
            if (r, c) not in self.cache:
                self.cache[(r, c)] = made.chunk(r, c)
            return self.cache[(r, c)]

    seeds = Seeds()
    opt = ra.MapOpt(dtw_border_constraint=0, dtw_fill_method=0, flag=ra.MapOpt().flag | 0x4)
    eng = ra.Engine(0)
    eng.upload_reference(ref.forward, ref.reverse)
    lib = eng.lib
    slot = max(rd["n_ev"] for rd in seeds.reads) + 8

    def one(on):
        """a fresh mapper through its rounds and its finish -> (finish ms, lines, traceback timing, text timing)"""
        cm = mapper.CMapper(eng, opt, StopOpt(), [f"seq{s}" for s in range(ref.n_seq)], [len(x) for x in ref.forward], slot_events=slot, max_reads=n,
                            carry=True, threads=a.threads, groups=1)
        took = []
        go = cm.finish

        def timed_finish():
            t0 = time.perf_counter()
            st = go()
            took.append((time.perf_counter() - t0) * 1e3)
            return st
        cm.finish = timed_finish
        lines, _ = mapper.map_reads_c(seeds, list(range(n)), cm, device_text=on)
        cm.close()
        f, w, db, pe = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
        assert lib.rawdtw_traceback_timing(eng._ctx, C.byref(f), C.byref(w), C.byref(db), C.byref(pe)) == 0
        tb = dict(fill_ms=round(f.value, 3), walk_ms=round(w.value, 3), path_elements=pe.value)
        return took[0], lines, tb, eng.aln_text_timing() if on else None

    ms = {False: [], True: []}
    lines, tb, tx = {}, {}, None
    for rep in range(REPS + 1):
        for on in (False, True):
            t, lines[on], tb[on], txt = one(on)
            if on:
                tx = txt
            if rep:   # (the first of each arm is the warm-up)
                ms[on].append(t)
            say("rep %d %s: finish %.2f ms" % (rep, "on " if on else "off", t))

    def fig(v):
        return dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), spread_ms=round(max(v) - min(v), 3))

    off, on = fig(ms[False]), fig(ms[True])
    elems = int(tb[False]["path_elements"])
    with_cigar = sum("\taln:s:(" in ln for ln in lines[True])
    checks = {"same_lines": lines[False] == lines[True], "lines_with_cigar": with_cigar > 0, "same_path_elements": tb[True]["path_elements"] == elems}
    rec = {
        "probe": "aln_text", "workload": "bench.py's reference and synthetic reads, global + full, --dtw-output-cigar, through the mapper", "reads": n,
        "lines_with_cigar": with_cigar, "path_elements": elems, "host_threads": a.threads, "repetitions": REPS,
        "finish_setter_off": off, "finish_setter_on": on,
        "on_minus_off_ms": round(on["median_ms"] - off["median_ms"], 3), "on_not_slower_than_off": bool(on["median_ms"] <= off["median_ms"]),
        "traceback_kernels_off": tb[False], "traceback_kernels_on": tb[True],
        "count_ms": round(tx["count_ms"], 3), "write_ms": round(tx["write_ms"], 3), "text_bytes_home": int(tx["text_bytes"]),
        "step_form_bytes_home": 5 * elems, "text_bytes_an_element": round(tx["text_bytes"] / max(elems, 1), 2),
        "off_arm_host_ns_an_element": round((off["median_ms"] - tb[False]["fill_ms"] - tb[False]["walk_ms"]) * 1e6 / max(elems, 1), 1),
        "kernels": kernel_resources(a.resource_usage) if a.resource_usage else None,
        "checks": checks,
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    eng.close()
    if not all(checks.values()):
        sys.exit("a check failed: %s" % checks)


if __name__ == "__main__":
    main()
