"""The packed records a device-planned batch hands from k_plan to k_runs (rawalign_amd/csrc/rawdtw_plan_fmt.h) and the host's
reader of a plan (rawdtw_plan_check.cpp: the stream half of verify_plan) checked by a stand-alone C++ program,
tests/abi/plan_fmt.cpp: neither has a HIP include, a plain compiler takes them.  Every format round-trips field by field;
a hand-built plan is accepted and twelve single corruptions of it are rejected.  Built plain and with AddressSanitizer +
UndefinedBehaviorSanitizer (its own main: nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")


def sweep(*maxima):
    """cases of tests/abi/plan_fmt.cpp's sweep(): each field over its range, the others at every combination of their extremes"""
    return sum((m + 1) << (len(maxima) - 1) for m in maxima)


CASES = (sweep(127, 127, 3, 1, 511) + 2 * sweep(0xFFFF, 0xFFFF) + sweep(0xFFFF, 63, 1023)  # records, entries
         + 64 * 4 + 4 * (1 << 20)                                                          # a copy order's source offset
         + (3 * 128) ** 2)                                                                 # pairs of sort bins
PLANS = 1 + 12 + 1  # the plan, its corruptions, the empty second pass that corruption 10 starts from


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_plan_fmt_and_checker(tmp_path, flags):
    exe = os.path.join(str(tmp_path), "plan_fmt")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "abi", "plan_fmt.cpp"),
                    os.path.join(CSRC, "rawdtw_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok %d %d" % (CASES, PLANS), run.stdout + run.stderr
    # every corruption was rejected with a message of its own line: "<n> <what>: <message>"
    said = [ln for ln in run.stderr.splitlines() if ln[:1].isdigit()]
    assert [int(ln.split()[0]) for ln in said] == list(range(1, 13)) and all(ln.split(": ", 1)[1].strip() for ln in said), run.stderr
