"""The context options' one table (rawalign_amd/csrc/rawdtw_options.h) against what the hand-written setter did before it
(tests/option_cases.py, recorded from that setter): every recorded (name, value) through the table's set and get by a stand-alone C++
program, tests/abi/options.cpp, built plain and with AddressSanitizer + UndefinedBehaviorSanitizer (its own main: nothing is preloaded).
Then the same through the library -- the setter and the getter on a default context record cannot be reached from here, but the dry run's
options can -- and the option block of include/rawdtw.h against the table's names."""
import os
import re
import subprocess

import numpy as np
import pytest

from rawalign_amd._lib import RawDTWError
from rawalign_amd.dtw import JOB_DTYPE, plan_dry_run
from tests import option_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")
N_CASES = sum(len(v) for v in oc.CASES.values())


def build(tmp_path, flags=()):
    exe = os.path.join(str(tmp_path), "options")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "abi", "options.cpp"), "-o", exe], check=True)
    return exe


def test_recorded_cases_are_the_issue_s():
    """the probe values every option was recorded at, and its own bounds' neighbours (a clamp shows as a value stored that was not given)"""
    common = [-2**63, -1, 0, 1, 2, 255, 256, 511, 512, 1023, 1024, 4096, 4097, 40000, 40001, 65535, 65536, 2**20, 2**20 + 1, 2**24 + 1, 2**30 + 1,
              2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**63 - 1]
    assert len(oc.CASES) == 45 and list(oc.CASES) == list(oc.DEFAULTS) and len(oc.PLANNER) == 15 and len(oc.READ_ONLY) == 3
    for name, cases in oc.CASES.items():
        values = [c[0] for c in cases]
        assert len(set(values)) == len(values) and set(common) <= set(values), name
        for value, status, stored, err in cases:   # a value that was moved was moved to a bound: its neighbours are recorded too
            assert (status == 0) == (err is None) and (status != 0 or stored == value or {stored - 1, stored, stored + 1} <= set(values)), (name, value)
        taken = [c[0] for c in cases if c[1] == 0]   # (and so are those of a range that refuses)
        assert {min(taken) - 1, max(taken) + 1} <= set(values) | {-2**63 - 1, 2**63}, name


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_table_does_what_the_setter_did(tmp_path, flags):
    exe = build(tmp_path, flags)
    lines = ["default %s %d" % kv for kv in oc.DEFAULTS.items()]
    lines += ["case %s %d %d %d %s" % (name, value, status, stored, err or "") for name, cases in oc.CASES.items() for value, status, stored, err in cases]
    lines += ["refused %s %d %s" % (name, status, err) for name, (status, err) in oc.REFUSED.items()]
    path = os.path.join(str(tmp_path), "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok %d %d" % (len(oc.CASES) + len(oc.READ_ONLY), N_CASES), run.stdout + run.stderr   # (none was skipped)
    assert set(oc.REFUSED) == set(oc.READ_ONLY) | {"no_such_option"} and oc.REFUSED["no_such_option"] == (1, "unknown option no_such_option")


def test_header_lists_every_option_once(tmp_path):
    """include/rawdtw.h's option block: an entry a line ('"name"' first) for each row of the table and for nothing else, and no other name quoted in it"""
    rows = [ln.split() for ln in subprocess.run([build(tmp_path), "--names"], capture_output=True, text=True, check=True).stdout.splitlines()]
    names = [r[0] for r in rows]
    assert sorted(names) == sorted(list(oc.CASES) + oc.READ_ONLY)
    assert [r[0] for r in rows if len(r) > 1] == oc.READ_ONLY
    with open(os.path.join(ROOT, "include", "rawdtw.h")) as f:
        text = f.read()
    block = text[text.index("/* ---- options"):text.index("int rawdtw_get_option(")]
    entries = re.findall(r'^ \*   "([a-z0-9_]+)"', block, re.M)
    assert sorted(entries) == sorted(names), (set(entries) ^ set(names), [e for e in entries if entries.count(e) > 1])
    assert set(re.findall(r'"([a-z0-9_]+)"', block)) == set(names)
    for r in rows:   # a read-only row says so in its entry, no other does
        entry = re.search(r'^ \*   "%s"(.*)$' % r[0], block, re.M).group(1)
        assert ("read-only" in entry) == (len(r) > 1), r[0]


def _jobs():
    """one job of every class the planner's options move: micro shapes, grouped bands, tiles of radius 1 .. 8, a long side, full matrices"""
    rng = np.random.default_rng(7)
    shapes = [(n, r) for n in (3, 4, 5, 8, 9, 16, 17, 40, 72, 73, 74, 95, 96, 97, 120, 199, 200, 201, 260) for r in (1, 2, 3, 4, 6, 8, 12)] + [(n, -1) for n in (50, 130, 200, 300, 1100)]
    jobs = np.zeros(len(shapes) * 40, JOB_DTYPE)
    for k in range(len(jobs)):
        n, r = shapes[k % len(shapes)]
        m = max(2, n - int(rng.integers(0, 3)))
        jobs[k]["n"], jobs[k]["m"], jobs[k]["band_radius"], jobs[k]["exclude_last"] = n, m, r, k & 1
        span = 1_500 if k < len(jobs) // 2 else 60_000   # (the first half's windows overlap: tiles of many jobs; the second half's lie apart)
        jobs[k]["read_off"], jobs[k]["ref_off"] = rng.integers(0, span - n), rng.integers(0, span - m)
    return jobs


def test_dry_run_takes_the_planner_s_options_and_no_other():
    jobs = _jobs()[:8]
    for name in oc.PLANNER + ["verify"]:
        plan_dry_run(jobs, 60_000, 60_000, options={name: 1})
    for name in [n for n in oc.CASES if n not in oc.PLANNER] + oc.READ_ONLY + ["no_such_option"]:
        with pytest.raises(RawDTWError, match=r"^rawdtw status 1: unknown option %s$" % name):
            plan_dry_run(jobs, 60_000, 60_000, options={name: 1})


def test_dry_run_clamps_as_the_setter_did():
    """at each bound of a planner option, one below and one above: the plan is the one of the value the setter stored for it"""
    jobs = _jobs()
    plans = {}

    def plan(name, value):
        if (name, value) not in plans:
            plans[(name, value)] = plan_dry_run(jobs, 60_000, 60_000, threads=2, options={name: value})
        return plans[(name, value)]

    moved = set()
    for name in oc.PLANNER:
        stored = {value: s for value, status, s, _ in oc.CASES[name] if status == 0}
        kept = sorted(v for v, s in stored.items() if v == s)   # (the values the option admits, among the recorded ones)
        lo, hi = kept[0], kept[-1]
        assert {lo - 1, hi + 1} <= set(stored) and stored[lo - 1] != lo - 1 and stored[hi + 1] != hi + 1, name
        for value in (lo - 1, lo, hi, hi + 1):
            assert plan(name, value) == plan(name, stored[value]), (name, value)
        if plan(name, lo) != plan(name, hi):
            moved.add(name)
    # (the job list is one the options act on: else the comparison above says nothing)
    # (the four that stay need company: "sort_n" / "sort_r1_n" at 255 are past the tiles' longest side, "sorted_tile_jobs" and "lane_hi_max_n" act
    # only under "sort_*" and "lane_hi")
    assert moved >= set(oc.PLANNER) - {"sort_n", "sort_r1_n", "sorted_tile_jobs", "lane_hi_max_n"}, moved
