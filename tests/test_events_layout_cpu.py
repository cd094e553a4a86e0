"""The detection workspace's layout (rawalign_amd/csrc/rawdtw_events_layout.h: where the arrays of a float or raw, plain or resident
detection lie in the device block and in the page-locked block) checked by a stand-alone C++ program, tests/abi/events_layout.cpp:
the header has no HIP include, a plain compiler takes it.  Regions aligned, inside the block, disjoint, large enough for what the
kernels index, empty where the kind does not use them; both totals and the pinned words' places equal to what detect_enqueue and
the two ends used to compute by hand; 28 bytes a sample (30 a raw sample).  Built plain and with AddressSanitizer +
UndefinedBehaviorSanitizer (its own main: nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")

CASES = 2 * 2 * 6 * 6   # raw x arena x n x N


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_events_layout(tmp_path, flags):
    exe = os.path.join(str(tmp_path), "events_layout")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "abi", "events_layout.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok %d" % CASES, run.stdout + run.stderr
