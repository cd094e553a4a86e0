#!/usr/bin/env python3
"""The HIP calls behind the batch entry points, for refactors of rawdtw_batch.cpp that must not move them.  Five things, each between two
markers (a pair of hipDeviceSynchronize, which the library never calls): a device-planned submit and its fetch, a compact submit and its
fetch, a carried round, a job-list create with a timed run and a fetch, and a batch the device-planned path declines, redone at its
fetch.  No diagnostic call is made.

    RAWDTW_LIBRARY=<library> rocprofv3 --hip-trace --output-format csv -d <dir> -o <name> -- python scripts/batch_calls_probe.py
    python scripts/batch_calls_probe.py compare <parent>_hip_api_trace.csv <new>_hip_api_trace.csv [out.json]
`compare`: the ordered lists of HIP API names from the first marker to the last, side by side."""
import csv
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def calls_between_markers(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Function"] for r in rows]
    marks = [i for i in range(len(names) - 1) if names[i] == names[i + 1] == "hipDeviceSynchronize"]
    assert len(marks) >= 2, "no markers in " + path
    return names[marks[0]:marks[-1] + 2], len(marks)


def compare(parent, new, out=None):
    (a, ma), (b, mb) = calls_between_markers(parent), calls_between_markers(new)
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
    res = {"probe": "batch_calls_probe", "what": "HIP API names in order between the script's first and last marker, parent's library and this tree's",
           "markers": {"parent": ma, "new": mb}, "calls": {"parent": len(a), "new": len(b)}, "first_difference": first,
           "verdict": "equal" if a == b else "DIFFERENT at call %d: parent %s, new %s" % (first, a[first:first + 3], b[first:first + 3])}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return a == b


def main():
    import numpy as np

    import rawalign_amd as ra
    from tests.replay_cases import case
    from tests.test_launch_options_gpu import _tiny_batch_with
    from tests.test_stream_path import _match, _two_rounds

    hip = C.CDLL("libamdhip64.so")
    vp = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731

    def mark():
        hip.hipDeviceSynchronize()
        hip.hipDeviceSynchronize()

    cs = case("tiny")
    eng = cs.engine()
    mark()
    b = cs.batch(eng, submit=True)  # 1: rawdtw_batch_submit, rawdtw_batch_fetch
    score, _ = b.fetch()
    b.close()
    mark()
    b = cs.batch(eng, compact=True)  # 2: rawdtw_batch_submit_compact
    score2, _ = b.fetch()
    b.close()
    assert np.array_equal(score.view(np.uint32), score2.view(np.uint32))
    mark()
    eng.close()

    rng = np.random.default_rng(1999)  # 3: a chunk round on top of the round before (rawdtw_batch_submit_carry)
    ref = [rng.normal(size=90000).astype(np.float32), rng.normal(size=90000).astype(np.float32)]
    eng = ra.Engine(0)
    eng.upload_reference([ref[0]], [ref[1]])
    cb1, cb2, prev_read, _ = _two_rounds(rng, eng, n_reads=60)
    eng.upload_events(cb2.events)
    opt = ra.MapOpt(dtw_min_score=5.0)
    copt = opt.c_struct()
    arr, carry, new_off, new_anchors = _match(eng.lib, cb2, cb1, prev_read)
    mark()
    b1 = ra.Batch(eng, opt, cb1)
    b1.run()
    b1.fetch()
    h = C.c_void_p()
    eng._check(eng.lib.rawdtw_batch_submit_carry(eng._ctx, C.byref(copt), cb2.n_reads, vp(arr[0]), vp(arr[1]), vp(arr[2]), vp(new_off), vp(new_anchors), vp(arr[3]),
                                                 vp(arr[4]), b1._h, vp(carry), C.byref(h)))
    score, keep = np.zeros(cb2.n_chains, np.float32), np.zeros(cb2.n_chains, np.uint8)
    eng._check(eng.lib.rawdtw_batch_fetch(eng._ctx, h, vp(score), vp(keep), None))
    eng.lib.rawdtw_batch_destroy(h)
    b1.close()
    mark()
    eng.close()

    cs = case("medium")  # 4: the job-list form, one timed run
    eng = cs.engine(device_plan=0)
    mark()
    b = cs.batch(eng)
    launches = b.run_timed()
    b.fetch()
    b.close()
    mark()
    eng.close()

    rng = np.random.default_rng(77)  # 5: a band wider than k_wide takes: declined, redone through the job list at fetch
    ref = [rng.normal(size=40000).astype(np.float32), rng.normal(size=40000).astype(np.float32)]
    eng = ra.Engine(0)
    eng.upload_reference([ref[0]], [ref[1]])
    cb, _ = _tiny_batch_with(rng, eng, 40000, special=(3000, 2800))
    mark()
    b = ra.Batch(eng, opt, cb)
    b.run()
    b.fetch()
    b.close()
    mark()
    eng.close()
    print("batch_calls_probe: five flows done, %d launches in the job-list batch's timed run" % len(launches))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "compare":
        sys.exit(0 if compare(*sys.argv[2:5]) else 1)
    main()
