#!/usr/bin/env python3
"""Generate tests/golden/local_ref.npz from the REFERENCE's own compiled dtw.cpp: DTW_semiglobal_slow and DTW_semiglobal_tb on the window
pair of every chain of tests/local_cases.make_case() (the local border constraint's one job a chain: include/rawdtw.h, "local border").

Runs only where the reference's sources are (oracle/Makefile's REF_SRC): `make -C oracle ref` compiles them where they lie into
oracle/_ref/ (never copied); the functions are called through their C++ symbols (tests/semiglobal_cases.RefSemiglobal).  The fixture
holds data only.

    python scripts/make_golden_local.py

local_ref.npz (C chains, every one with anchors):
  events float32[...], chain_off / anchor_off uint64, anchors (target, query) uint32 pairs, ref_base uint64 (virtual: forward at 0, reverse
  behind it), read_base uint32, forward / reverse float32[...]: the case's inputs
  n, m           int32[C]   the windows' lengths
  slow, tb_cost  uint32[C]  bits of DTW_semiglobal_slow(a, n, b, m, false) and of DTW_semiglobal_tb's cost
  j0, end_j      int32[C]   the columns of the path's first and last element
  path_len int32[C], path_off int64[C] into path_step uint8[...] (bit 0: i advanced, bit 1: j advanced; a path's first byte is 0) and
  path_d float32[...]
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rawalign_amd.dtw import ANCHOR_DTYPE  # noqa: E402
from tests import local_cases as lc  # noqa: E402
from tests import semiglobal_cases as sc  # noqa: E402
from tests.golden_util import golden_path  # noqa: E402


def main():
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    ref = sc.RefSemiglobal()
    case = lc.make_case()
    cb = case.cb
    C = cb.n_chains
    n, m, slow, tbc = np.zeros(C, np.int32), np.zeros(C, np.int32), np.zeros(C, np.uint32), np.zeros(C, np.uint32)
    j0, end_j, plen, poff = np.zeros(C, np.int32), np.zeros(C, np.int32), np.zeros(C, np.int32), np.zeros(C, np.int64)
    steps, pds, at = [], [], 0
    for c in range(C):
        a, b, _, _ = lc.windows(cb, case.arena, c)
        n[c], m[c] = len(a), len(b)
        slow[c] = sc.bits(ref.slow(a, b, False))[0]
        cost, i, j, d = ref.tb(a, b, False)
        tbc[c] = sc.bits(cost)[0]
        j0[c], end_j[c], plen[c], poff[c] = int(j[0]), int(j[-1]), len(i), at
        di, dj = np.diff(i.astype(np.int64), prepend=int(i[0])), np.diff(j.astype(np.int64), prepend=int(j[0]))
        assert i[0] == 0 and ((di == 0) | (di == 1)).all() and ((dj == 0) | (dj == 1)).all()
        steps.append((di | (dj << 1)).astype(np.uint8)); pds.append(d.astype(np.float32))
        at += len(i)
    out = golden_path(lc.FIXTURE)
    np.savez_compressed(out, events=cb.events, chain_off=cb.chain_off, anchor_off=cb.anchor_off, anchors=np.ascontiguousarray(cb.anchors, ANCHOR_DTYPE),
                        ref_base=cb.ref_base, read_base=cb.read_base, forward=case.ref.forward[0], reverse=case.ref.reverse[0], n=n, m=m, slow=slow,
                        tb_cost=tbc, j0=j0, end_j=end_j, path_len=plen, path_off=poff, path_step=np.concatenate(steps), path_d=np.concatenate(pds))
    print("%s: %d chains, n %d..%d, m %d..%d, %d path elements, %d bytes" % (lc.FIXTURE, C, n.min(), n.max(), m.min(), m.max(), at, os.path.getsize(out)))


if __name__ == "__main__":
    main()
