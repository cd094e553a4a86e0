"""The traceback driver's layout and split (rawalign_amd/csrc/rawdtw_tb_layout.h) checked by a stand-alone C++ program,
tests/abi/tb_layout.cpp: the header has no HIP include, a plain compiler takes it.  Built plain and with AddressSanitizer +
UndefinedBehaviorSanitizer (its own main: nothing is preloaded).  Its sweep checks the slots' regions and the totals against the three
former drivers' formulas; its split is held here to the three Python models of the cut (tests/traceback_cases.py,
tests/banded_tb_cases.py, tests/high_offset_cases.py).  And the premises of tests/test_tb_driver_gpu.py's lists."""
import os
import subprocess

import numpy as np
import pytest

import rawalign_amd as ra
from tests import banded_tb_cases as bc
from tests import high_offset_cases as hc
from tests import tb_driver_cases as dc
from tests import traceback_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")
CASES = 6 * 6 * 2 * 2 * 2   # cnt x acc x form x extra word x records
FLAGS = {"plain": (), "asan_ubsan": ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")}


@pytest.fixture(scope="module", params=sorted(FLAGS))
def program(request, tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("tb_layout")), "tb_layout")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *FLAGS[request.param], "-I", CSRC, os.path.join(ROOT, "tests", "abi", "tb_layout.cpp"),
                    "-o", exe], check=True)
    return exe


def test_layout_sweep(program):
    run = subprocess.run([program], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok %d" % CASES, run.stdout + run.stderr


def cuts(program, job_bytes, budget):
    """[(first job, job count)] from the program's split"""
    text = "%d\n" % budget + "\n".join(str(int(b)) for b in job_bytes) + "\n"
    run = subprocess.run([program, "split"], input=text, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    return [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()]


def full_bytes(shapes):
    return [tc.dir_bytes_for(n, m) + 256 for n, m in shapes]


def over_budget_lists():
    """a list with one job over a budget of 1 MiB first, last and in the middle"""
    small, big = [(300, 400)] * 9, (3000, 2049)
    assert tc.dir_bytes_for(*big) > tc.MIB > tc.dir_bytes_for(*small[0]) + 256
    return [[big] + small, small + [big], small[:4] + [big] + small[4:]]


def test_split_equals_the_full_matrix_model(program):
    lists = [(tc.shapes_of(tc.CASES[name]()), budget) for name in sorted(tc.CASES) for budget in (tc.MIB, 2 * tc.MIB, 16 * tc.MIB, tc.DEFAULT_BUDGET)]
    lists += [(shapes, tc.MIB) for shapes in over_budget_lists()] + [([], tc.MIB)]
    for shapes, budget in lists:
        assert cuts(program, full_bytes(shapes), budget) == tc.split(shapes, budget), (len(shapes), budget)
    assert [c for _, c in cuts(program, full_bytes(over_budget_lists()[2]), tc.MIB)] == [4, 1, 5]


def counts(program, job_bytes, budget):
    got = cuts(program, job_bytes, budget)
    assert [b for b, _ in got] == [0] + list(np.cumsum([c for _, c in got])[:-1])   # whole jobs in job order
    return [c for _, c in got]


def test_split_equals_the_banded_and_semiglobal_models(program):
    banded = dc.banded_cases()
    jobs = [dict(n=len(a), m=len(b), band_radius=R) for a, b, R, _ in banded]
    for mb in (1, 2, 16384):
        assert counts(program, dc.banded_job_bytes(banded), mb << 20) == bc.sub_batches(jobs, mb) == hc.sub_batches("banded", jobs, mb << 20)
    semi = dc.semiglobal_cases()
    jobs = [dict(n=len(a), m=len(b)) for a, b, _ in semi]
    for mb in (1, 2, 16384):
        assert counts(program, [b + 256 for b in dc.semiglobal_job_bytes(semi)], mb << 20) == hc.sub_batches("semiglobal", jobs, mb << 20)
    for shapes in over_budget_lists():   # the full-matrix shapes as semiglobal jobs
        jobs = [dict(n=n, m=m) for n, m in shapes]
        assert counts(program, [hc.semi_dir_bytes(n, m) + 256 for n, m in shapes], tc.MIB) == hc.sub_batches("semiglobal", jobs, tc.MIB)


# ---- the premises of tests/test_tb_driver_gpu.py ---------------------------------------------------------------------------------------
def premise(split, job_bytes):
    assert len(split) >= 5 and len(set(split)) >= 3, split                  # unequal job counts
    q = dc.sub_batch_of(split, dc.BIG_AT)
    assert 2 <= q <= len(split) - 3 and split[q] == 1, (q, split)             # alone, in the middle: both slots were used before it and are after it
    assert job_bytes[dc.BIG_AT] > dc.BUDGET_MB << 20 and max(b for k, b in enumerate(job_bytes) if k != dc.BIG_AT) < (dc.BUDGET_MB << 20) // 2
    return q


def test_the_banded_list_is_what_it_is_there_for():
    cases = dc.banded_cases()
    split = dc.banded_split(cases)
    premise(split, dc.banded_job_bytes(cases))
    assert {ex for _, _, _, ex in cases} == {0, 1}
    a, b, R, ex = cases[dc.NO_PATH_AT]
    q = dc.sub_batch_of(split, dc.NO_PATH_AT)
    assert len(ra.banded_tb_host(a, b, R, ex)) == 0 and ex == 1 and 0 < q < len(split) - 1 and split[q] > 1   # no path: exclude_last has nothing to pop
    assert sum(len(a) + len(b) - 1 for a, b, _, _ in cases) < 1 << 20


def test_the_semiglobal_list_is_what_it_is_there_for():
    cases = dc.semiglobal_cases()
    split = dc.semiglobal_split(cases)
    premise(split, [b + 256 for b in dc.semiglobal_job_bytes(cases)])
    assert {ex for _, _, ex in cases} == {0, 1}
    starts = [ra.semiglobal_host(a, b, ex, traceback=True)[0].j[0] for a, b, ex in cases[:8]]
    assert min(starts) >= 30, starts                                         # j0 > 0: the (i, j) form must seed j with it
    assert sum(len(a) + len(b) - 1 for a, b, _ in cases) < 1 << 20
