#!/usr/bin/env python3
"""Generate tests/golden/dtw_ref_random.npz and tests/golden/find_outlier_ref.npz from the REFERENCE's own compiled code.

Runs only where the reference's sources are (oracle/Makefile's REF_SRC): `make -C oracle ref ref_outlier` compiles them
where they lie into oracle/_ref/ (never copied).  The fixtures hold data only -- inputs or their digest, and what the
reference returns -- so that tests/test_oracle.py and tests/test_mapping_host.py check against the reference anywhere.

    python scripts/make_golden_ref.py

dtw_ref_random.npz (the 3000 seeded random cases of tests.golden_util.dtw_random_inputs):
  inputs_sha256  uint8[32]          digest of the inputs the answers belong to
  global_        uint32[n]          bits of DTW_global
  banded         uint32[n]          bits of DTW_global_slantedbanded_antidiagonalwise
  tb_case        int64[k]           cases with a traceback (every 7th)
  tb_cost        uint32[k]          bits of DTW_global_tb's cost
  tb_len         int64[k]           path length
  tb_digest      uint8[k, 32]       tests.golden_util.path_digest of (i, j, d)
find_outlier_ref.npz:
  shapes         int64[c, 2]        (points, dims) of each input
  vals           float32[...]       the inputs, row-major, one after the other
  plain          uint32[c]          bits of find_outlier, built with contraction off
  contracted     uint32[c]          bits of find_outlier, built as the reference's Makefile builds it on an FMA host
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.loader import RefDTW  # noqa: E402
from tests.golden_util import bits, dtw_random_inputs, golden_path, path_digest  # noqa: E402


def dtw_random():
    ref = RefDTW()
    cases, digest = dtw_random_inputs()
    g, bd, tb_case, tb_cost, tb_len, tb_dig = [], [], [], [], [], []
    for t, (a, b, R0, ex) in enumerate(cases):
        g.append(bits(ref.dtw_global(a, b, ex)))
        bd.append(bits(ref.dtw_banded(a, b, R0, ex)))
        if t % 7 == 0:
            c, i, j, d = ref.dtw_global_tb(a, b, ex)
            tb_case.append(t); tb_cost.append(bits(c)); tb_len.append(len(i)); tb_dig.append(np.frombuffer(path_digest(i, j, d), np.uint8))
    np.savez_compressed(golden_path("dtw_ref_random.npz"), inputs_sha256=np.frombuffer(digest, np.uint8),
                        global_=np.array(g, np.uint32), banded=np.array(bd, np.uint32), tb_case=np.array(tb_case, np.int64),
                        tb_cost=np.array(tb_cost, np.uint32), tb_len=np.array(tb_len, np.int64), tb_digest=np.array(tb_dig, np.uint8))
    print("dtw_ref_random.npz: %d cases, %d paths" % (len(cases), len(tb_case)))


def find_outlier():
    # the inputs tests/test_mapping_host.py has always drawn: five from its seeded generator, then twelve more
    rng = np.random.default_rng(2)
    xs = [rng.random((5, n)).astype(np.float32) for n in (1, 3, 8, 17, 40)]
    xs += [rng.random((4, n)).astype(np.float32) for n in (2, 4, 5, 7, 9, 12, 15, 16, 31, 33, 100, 257)]
    got = {}
    for name, so in (("plain", "libsu0.so"), ("contracted", "libsu1.so")):
        lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", so))
        lib.find_outlier.restype = C.c_float
        got[name] = []
        for x in xs:
            rows = (C.c_void_p * len(x))(*[x[i].ctypes.data for i in range(len(x))])
            got[name].append(bits(np.float32(lib.find_outlier(rows, x.shape[1], len(x)))))
    np.savez_compressed(golden_path("find_outlier_ref.npz"), shapes=np.array([x.shape for x in xs], np.int64),
                        vals=np.concatenate([x.ravel() for x in xs]).astype(np.float32),
                        plain=np.array(got["plain"], np.uint32), contracted=np.array(got["contracted"], np.uint32))
    print("find_outlier_ref.npz: %d inputs" % len(xs))


def main():
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref", "ref_outlier"], check=True)
    dtw_random()
    find_outlier()


if __name__ == "__main__":
    main()
