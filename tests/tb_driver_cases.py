"""Case lists for the traceback driver (rawalign_amd/csrc/rawdtw_tb_driver.cpp) on the two paths that ran one sub-batch at a time before
it: banded and semiglobal.  Shared by tests/test_tb_driver_cpu.py (the lists have the properties they are there for, decided with the
CPU models of the split and the host restatements) and tests/test_tb_driver_gpu.py.

At a budget of 1 MiB each list is cut into at least five sub-batches of unequal job counts; one job in the middle of the list is over
the budget alone and goes alone; so both slots of every buffer are used, a slot is reused, and a sub-batch of one job lies between
sub-batches of many.  exclude_last alternates.  The banded list has a job without a path (path_len 0) in a middle sub-batch, the
semiglobal list's chunks are planted in their references, so that their paths start at a column j0 > 0."""
import functools

import numpy as np

from tests import banded_tb_cases as bc
from tests import high_offset_cases as hc

BUDGET_MB = 1
BIG_AT = 31        # where the job over the budget sits
NO_PATH_AT = 20    # banded: the job without a path


@functools.lru_cache(maxsize=None)
def banded_cases():
    """[(a, b, R, exclude_last)]: 60 jobs of 300 .. 1 200 events at the mapper's radius (a tenth of n), b a resampled noisy a; a
    2 000 x 2 000 job at radius 1 000 (16 chunks a row: 1.09 MB of directions) and bc.SMALLEST_NO_PATH"""
    rng = np.random.default_rng(6161)
    cases = []
    for k in range(60):
        n = int(rng.integers(300, 1201))
        m = max(1, int(n * rng.uniform(0.7, 1.3)))
        a = rng.normal(size=n).astype(np.float32)
        b = (np.interp(np.linspace(0, n - 1, m), np.arange(n), a) + rng.normal(0, 0.2, m)).astype(np.float32)
        cases.append((a, b, max(1, n // 10), k & 1))
    a = rng.normal(size=2000).astype(np.float32)
    cases[BIG_AT] = (a, (a + rng.normal(0, 0.2, 2000)).astype(np.float32), 1000, 1)
    a, b, R = bc.SMALLEST_NO_PATH
    cases[NO_PATH_AT] = (a, b, R, 1)
    return cases


@functools.lru_cache(maxsize=None)
def semiglobal_cases():
    """[(a, b, exclude_last)]: 50 chunks of 50 .. 600 events, each a noisy stretch of its reference of 300 .. 2 000 events that starts
    at least 40 columns in; a 1 600 x 2 000 job (four strips: 1.06 MB of directions)"""
    rng = np.random.default_rng(6262)
    cases = []
    for k in range(50):
        n = int(rng.integers(50, 601))
        m = int(rng.integers(max(300, n + 80), 2001))
        b = rng.normal(size=m).astype(np.float32)
        s = int(rng.integers(40, m - n - 20))
        cases.append(((b[s:s + n] + rng.normal(0, 0.05, n)).astype(np.float32), b, k & 1))
    b = rng.normal(size=2000).astype(np.float32)
    cases[BIG_AT] = ((b[200:1800] + rng.normal(0, 0.05, 1600)).astype(np.float32), b, 1)
    return cases


def banded_job_bytes(cases):
    """a job's direction bytes as the split counts them and as the timing getter sums them: rounded up to 256"""
    return [hc.al256(bc.dir_bytes(len(a), len(b), R)) for a, b, R, _ in cases]


def semiglobal_job_bytes(cases):
    """as the timing getter sums them (a multiple of 1 024 each); the split counts 256 more a job"""
    return [hc.al256(hc.semi_dir_bytes(len(a), len(b))) for a, b, _ in cases]


def banded_split(cases, mb=BUDGET_MB):
    """job counts of the sub-batches (bc.sub_batches over the shapes)"""
    return bc.sub_batches([dict(n=len(a), m=len(b), band_radius=R) for a, b, R, _ in cases], mb)


def semiglobal_split(cases, mb=BUDGET_MB):
    return hc.sub_batches("semiglobal", [dict(n=len(a), m=len(b)) for a, b, _ in cases], mb << 20)


def sub_batch_of(counts, k):
    """which sub-batch job k is in"""
    return int(np.searchsorted(np.cumsum(counts), k, side="right"))
