"""The seeding workspace's layout (rawalign_amd/csrc/rawdtw_seed_layout.h: where the arrays of a plain, a resident and a detected
seeding lie in the device block and in the page-locked block) checked by a stand-alone C++ program, tests/abi/seed_layout.cpp: the
header has no HIP include, a plain compiler takes it.  Regions aligned, inside the block, disjoint, large enough for what the
kernels index, empty where the kind does not use them; both totals equal to the sums the three begins used to compute each for
itself.  Built plain and with AddressSanitizer + UndefinedBehaviorSanitizer (its own main: nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")

CASES = 3 * 6 * 6 * 2   # kinds x n x N x w


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_seed_layout(tmp_path, flags):
    exe = os.path.join(str(tmp_path), "seed_layout")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "abi", "seed_layout.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok %d" % CASES, run.stdout + run.stderr
