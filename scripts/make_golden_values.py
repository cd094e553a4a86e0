#!/usr/bin/env python3
"""Generate tests/golden/dtw_ref_values.npz from the REFERENCE's own compiled dtw.cpp: its answers on the value domains of
tests/value_cases.py (costs around and far above the banded DP's 1e10 literal, subnormals, zeros, integers).

Runs only where the reference's sources are (oracle/Makefile's REF_SRC): `make -C oracle ref` compiles them where they lie
into oracle/_ref/ (never copied).  The fixture holds bits and digests only -- no inputs (tests/value_cases.py regenerates
them from its seeds; their SHA-256 is recorded) and nothing of the reference's text.

    python scripts/make_golden_values.py

dtw_ref_values.npz (D domains in value_cases.DOMAIN_NAMES order, N cases each, R = 1 + len(FIXED_RADII) radii a case):
  inputs_sha256  uint8[32]           value_cases.inputs_sha256 of the inputs the answers belong to
  global_        uint32[D, N]        bits of DTW_global
  banded         uint32[D, N, R]     bits of DTW_global_slantedbanded_antidiagonalwise at value_cases.fixture_radii(n)
  tb_cost        uint32[D, N / 3]    bits of DTW_global_tb's cost, every third case
  tb_len         int32[D, N / 3]     path length
  tb_digest      uint8[D, N / 3, 32] tests.golden_util.path_digest of (i, j, d)
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.loader import RefDTW  # noqa: E402
from tests import value_cases as vc  # noqa: E402
from tests.golden_util import bits, golden_path, path_digest  # noqa: E402


def main():
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    ref = RefDTW()
    cases = {name: vc.fixture_cases(name) for name in vc.DOMAIN_NAMES}
    g, bd, tc, tl, td = [], [], [], [], []
    for name in vc.DOMAIN_NAMES:
        g.append([bits(ref.dtw_global(a, b, ex)) for a, b, ex in cases[name]])
        bd.append([[bits(ref.dtw_banded(a, b, R, ex)) for R in vc.fixture_radii(len(a))] for a, b, ex in cases[name]])
        tb = [ref.dtw_global_tb(a, b, ex) for a, b, ex in cases[name][::vc.TB_EVERY]]
        tc.append([bits(c) for c, _, _, _ in tb])
        tl.append([len(i) for _, i, _, _ in tb])
        td.append([np.frombuffer(path_digest(i, j, d), np.uint8) for _, i, j, d in tb])
    out = golden_path("dtw_ref_values.npz")
    np.savez_compressed(out, inputs_sha256=np.frombuffer(vc.inputs_sha256(cases), np.uint8), global_=np.array(g, np.uint32),
                        banded=np.array(bd, np.uint32), tb_cost=np.array(tc, np.uint32), tb_len=np.array(tl, np.int32),
                        tb_digest=np.array(td, np.uint8))
    print("dtw_ref_values.npz: %d domains x %d cases, %d bytes" % (len(vc.DOMAIN_NAMES), vc.N_FIXTURE_CASES, os.path.getsize(out)))


if __name__ == "__main__":
    main()
