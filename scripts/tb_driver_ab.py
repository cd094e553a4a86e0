#!/usr/bin/env python3
"""The traceback calls of a parent build's library against this tree's, alternating (profiles/tb_driver_ab.json): two workers
(scripts/tb_driver_ab_worker.py), one on either library; for every arm one warm-up call on each (the first call of its shape, on a
fresh context for the first arm of a workload: reported, not gated), then 7 rounds parent, new, parent, new ...  Verdict per arm: the
new median of call_ms (finish_ms for a mapper's finish) is at most the parent's median plus the parent's own max - min over its 7
rounds; fill_ms and walk_ms agree within that same spread; same_results: both libraries wrote the same paths (lengths, or the hash of
the mapper's lines) and direction bytes.
    python scripts/tb_driver_ab.py PARENT_LIBRARY OUT.json [ARM ...]      (arms: the worker's ARMS, default all)"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 7
ALL = ["banded", "full_steps", "semiglobal_tb", "semiglobal_cost", "local_scoring", "bench_traceback", "finish_off", "finish_on", "finish_local", "finish_banded"]


def main():
    LIBS = {"parent": os.path.abspath(sys.argv[1]), "new": os.path.join(ROOT, "rawalign_amd", "librawdtw.so")}
    out_path, arms = sys.argv[2], sys.argv[3:] or ALL
    workers = {}
    for name, lib in LIBS.items():
        env = dict(os.environ, RAWDTW_LIBRARY=lib)
        workers[name] = subprocess.Popen([sys.executable, os.path.join(ROOT, "scripts", "tb_driver_ab_worker.py")], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                         text=True, env=env, cwd=ROOT)

    def ask(name, arm):
        w = workers[name]
        w.stdin.write(arm + "\n")
        w.stdin.flush()
        line = w.stdout.readline()
        if not line:   # the worker died: nothing more is started on the GPU
            for x in workers.values():
                x.kill()
            sys.exit("worker %s died in arm %s (exit %s)" % (name, arm, w.wait()))
        return json.loads(line)

    res = {}
    for arm in arms:
        rec = res[arm] = {"first_call": {}, "rounds": {"parent": [], "new": []}}
        for name in LIBS:
            rec["first_call"][name] = ask(name, arm)
        for r in range(ROUNDS):
            for name in LIBS:
                rec["rounds"][name].append(ask(name, arm))
        key = "finish_ms" if "finish_ms" in rec["rounds"]["parent"][0] else "call_ms"
        verdict = {}
        call = [x[key] for x in rec["rounds"]["parent"]]
        call_spread = max(call) - min(call)   # the one margin: the parent's own max - min of the call
        for k in (key, "fill_ms", "walk_ms"):
            if k not in rec["rounds"]["parent"][0]:
                continue
            p = [x[k] for x in rec["rounds"]["parent"]]
            n = [x[k] for x in rec["rounds"]["new"]]
            spread = max(p) - min(p)
            pm, nm = statistics.median(p), statistics.median(n)
            ok = nm <= pm + call_spread if k == key else abs(nm - pm) <= call_spread
            verdict[k] = {"parent_median": round(pm, 4), "new_median": round(nm, 4), "parent_spread": round(spread, 4), "new_min": round(min(n), 4),
                          "new_max": round(max(n), 4), "met": bool(ok)}
        rec["verdict"] = verdict
        rec["first_call_ms"] = {name: round(rec["first_call"][name].get(key, 0.0), 3) for name in LIBS}
        rec["same_results"] = rec["rounds"]["parent"][0].get("check") == rec["rounds"]["new"][0].get("check") and \
            rec["rounds"]["parent"][0].get("direction_bytes") == rec["rounds"]["new"][0].get("direction_bytes")
        print(arm, json.dumps(verdict), "first", rec["first_call_ms"], "same", rec["same_results"], flush=True)
        with open(out_path, "w") as f:
            json.dump({"rounds": ROUNDS, "arms": res, "every_gated_arm_met": all(v["met"] for r in res.values() for v in r["verdict"].values())}, f, indent=1)
            f.write("\n")
    for w in workers.values():
        w.stdin.close()
    for w in workers.values():
        w.wait(timeout=120)


if __name__ == "__main__":
    main()
