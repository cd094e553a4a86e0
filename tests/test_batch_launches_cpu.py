"""A batch's launch table (rawalign_amd/csrc/rawdtw_launches.h: which launches a batch reports, under which kinds, which of them travel
inside the merged launch, and where the event pairs of timed runs lie) checked by a stand-alone C++ program, tests/abi/batch_launches.cpp:
the header has no HIP include, a plain compiler takes it.  The device-planned form and every job-list launch list of up to one launch of
each kind the planner emits, in two orders, under every combination of the four settings the merge reads; and the table of wave classes
(rows a lane, waves a job, reported parameter; both conversions, an unknown parameter rejected).  Built plain and with
AddressSanitizer + UndefinedBehaviorSanitizer (its own main: nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")

KINDS = 8              # lane; wreg -16, -8, 0, 4; wave; full; lane-hi: each in a list or not
JOB_LISTS = 2 ** KINDS * 2 * 2 ** 4   # lists x orders x (merge_small, tile_threads, side streams, serial_launches)
CASES = 1 + JOB_LISTS  # (and the device-planned form)


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_batch_launches(tmp_path, flags):
    assert CASES == 8193
    exe = os.path.join(str(tmp_path), "batch_launches")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "abi", "batch_launches.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok %d" % CASES, run.stdout + run.stderr
