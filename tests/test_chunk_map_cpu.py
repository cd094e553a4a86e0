"""The chunk map of the tile launch (rawalign_amd/csrc/rawdtw_chunks.h: which of a pass's sorted job records a wave of k_runs takes
together) checked exhaustively by a stand-alone C++ program, tests/abi/chunk_map.cpp: the header has no HIP include, a plain
compiler takes it.  Built plain and with AddressSanitizer + UndefinedBehaviorSanitizer (its own main: nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every n3 <= 64, n3 <= n_hi <= n_jobs <= 512
CASES = sum(min(64, n_hi) + 1 for n_jobs in range(513) for n_hi in range(n_jobs + 1))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_chunk_map_exhaustive(tmp_path, flags):
    exe = os.path.join(str(tmp_path), "chunk_map")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "rawalign_amd", "csrc"),
                    os.path.join(ROOT, "tests", "abi", "chunk_map.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok %d" % CASES, run.stdout + run.stderr
