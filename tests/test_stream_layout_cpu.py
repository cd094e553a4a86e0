"""The device-planned batch's workspace layout (rawalign_amd/csrc/rawdtw_stream_layout.h: where the arrays of a plain, a compact and a
carried batch lie in the pooled device block and in the page-locked block, and rawdtw_events_append's staging) checked by a stand-alone
C++ program, tests/abi/stream_layout.cpp: the header has no HIP include, a plain compiler takes it.  Regions aligned, inside the block,
disjoint, in the order the offsets were handed out in, large enough for what the kernels index, empty where the kind does not use them;
the results one behind the other from offset 0 and the pinned block at the same offsets; the derived counts and both totals equal to
what batch_create_stream used to compute by hand.  Built plain and with AddressSanitizer + UndefinedBehaviorSanitizer (its own main:
nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")

NA = (1, 511, 512, 513, 8191, 8192, 8193, 100_000)
NC_NR = sum(1 if nc == 1 else 2 for na in NA for nc in sorted({1, 2, 255, 257, na}) if nc <= na)   # nr in {1, nc}
BATCH = NC_NR * 3 * (1 + 2 + 2)   # pass_pool x (plain; compact x n_wide; round x n_full)
APPEND = 6 * 5                    # n_new x n_segments
CASES = BATCH + APPEND


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_stream_layout(tmp_path, flags):
    assert CASES == 990
    exe = os.path.join(str(tmp_path), "stream_layout")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "abi", "stream_layout.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok %d" % CASES, run.stdout + run.stderr
