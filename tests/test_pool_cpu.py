"""The mapper's pool of threads (rawalign_amd/csrc/rawdtw_pool.h: spin-then-sleep workers, two condition variables, a generation counter)
driven by a stand-alone C++ program, tests/abi/pool.cpp: the header has no include beyond the standard library, a plain compiler takes
it.  1, 2, 4 and 8 threads; empty, inline, ragged and grain-1 loops; thousands of loops back to back (workers spinning), loops 5 ms apart
(workers asleep), a loop with a slow worker (the caller asleep), destruction in each of those states.  Every index writes its own plain
element and the caller reads them all after run().  Built plain, with ThreadSanitizer, and with AddressSanitizer +
UndefinedBehaviorSanitizer (its own main: nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")

LOOPS = 4 * (6 + 3000 + 4 + 3 + 1)   # thread counts x (shapes, spinning, asleep, slow worker, destruction)


@pytest.mark.parametrize("flags", [(), ("-fsanitize=thread", "-g"), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "tsan", "asan_ubsan"])
def test_pool(tmp_path, flags):
    exe = os.path.join(str(tmp_path), "pool")
    subprocess.run(["g++", "-std=c++17", "-pthread", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "abi", "pool.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok %d" % LOOPS, run.stdout + run.stderr
