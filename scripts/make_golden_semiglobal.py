#!/usr/bin/env python3
"""Generate tests/golden/semiglobal_ref.npz from the REFERENCE's own compiled dtw.cpp: DTW_semiglobal, DTW_semiglobal_slow and
DTW_semiglobal_tb on tests/semiglobal_cases.fixture_cases().

Runs only where the reference's sources are (oracle/Makefile's REF_SRC): `make -C oracle ref` compiles them where they lie into
oracle/_ref/ (never copied); the three functions are called through their C++ symbols (tests/semiglobal_cases.RefSemiglobal).  The
fixture holds data only.

    python scripts/make_golden_semiglobal.py

semiglobal_ref.npz (K cases; index 0 / 1 of a pair is exclude_last_element):
  tag            <U   [K]      the case's family (a value domain of tests/value_cases.py, or normal / int / tall / two-minima)
  n, m           int32[K]      lengths;  a_off, b_off int64[K] into  a, b float32[...]: the inputs
  fast           uint32[K, 2]  bits of DTW_semiglobal (it ignores the flag: both columns are equal)
  slow, tb_cost  uint32[K, 2]  bits of DTW_semiglobal_slow and of DTW_semiglobal_tb's cost
  end_j          int32[K]      the last element's j of the path with the flag off
  tb_len         int32[K, 2]   path lengths;  tb_off int64[K, 2] into  path_i, path_j uint16[...], path_d float32[...]
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import semiglobal_cases as sc  # noqa: E402
from tests.golden_util import golden_path  # noqa: E402


def main():
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    ref = sc.RefSemiglobal()
    cases = sc.fixture_cases()
    K = len(cases)
    fast, slow, tbc = np.zeros((K, 2), np.uint32), np.zeros((K, 2), np.uint32), np.zeros((K, 2), np.uint32)
    tb_len, tb_off, end_j = np.zeros((K, 2), np.int32), np.zeros((K, 2), np.int64), np.zeros(K, np.int32)
    pi, pj, pd, at = [], [], [], 0
    for k, (tag, a, b) in enumerate(cases):
        for ex in (0, 1):
            fast[k, ex] = sc.bits(ref.semiglobal(a, b, ex))[0]
            slow[k, ex] = sc.bits(ref.slow(a, b, ex))[0]
            c, i, j, d = ref.tb(a, b, ex)
            tbc[k, ex] = sc.bits(c)[0]
            tb_len[k, ex], tb_off[k, ex] = len(i), at
            pi.append(i.astype(np.uint16)); pj.append(j.astype(np.uint16)); pd.append(d.astype(np.float32))
            at += len(i)
            if ex == 0:
                end_j[k] = int(j[-1])
    a_off = np.cumsum([0] + [len(a) for _, a, _ in cases])[:-1].astype(np.int64)
    b_off = np.cumsum([0] + [len(b) for _, _, b in cases])[:-1].astype(np.int64)
    out = golden_path(sc.FIXTURE)
    np.savez_compressed(out, tag=np.array([t for t, _, _ in cases]), n=np.array([len(a) for _, a, _ in cases], np.int32),
                        m=np.array([len(b) for _, _, b in cases], np.int32), a_off=a_off, b_off=b_off,
                        a=np.concatenate([a for _, a, _ in cases]).astype(np.float32),
                        b=np.concatenate([b for _, _, b in cases]).astype(np.float32), fast=fast, slow=slow, tb_cost=tbc, end_j=end_j,
                        tb_len=tb_len, tb_off=tb_off, path_i=np.concatenate(pi), path_j=np.concatenate(pj), path_d=np.concatenate(pd))
    print("%s: %d cases, %d path elements, %d bytes" % (sc.FIXTURE, K, at, os.path.getsize(out)))


if __name__ == "__main__":
    main()
