#!/usr/bin/env python
"""Record tests/golden/seed_min_ref.npz: the reference's own minimizer seeding on the cases of tests/seed_min_cases.py.

Needs oracle/_ref/libref_map{0,1}.so (make -C oracle ref_map, only where the reference's sources are).  Per case and chunk: the
sketch (ri_sketch, called as scripts/make_golden_seed.py calls it) and the hits in the order gen_chains meets them
(oracle.loader.RefMap.hits), from both builds, asserted equal.  Kept per case: the inputs' SHA-256, the sketch in full, hit_off,
and the hit rows where there are at most MAX_ROWS of them, else their SHA-256."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from make_golden_seed import ref_sketch  # noqa: E402
from oracle.loader import RefMap  # noqa: E402
from tests import seed_cases as sc  # noqa: E402
from tests import seed_min_cases as smc  # noqa: E402


def small(a):
    a = np.asarray(a)
    return a.astype(np.uint16 if a.size == 0 or a.max() < 65536 else np.uint32)


def main():
    assert RefMap.available(), "build oracle/_ref first (make -C oracle ref_map)"
    out = {}
    for name in smc.CASES:
        fwd, rev, p, chunks = smc.build_case(name)
        rms = [RefMap(fwd, rev, fused=bool(f), e=p.e, q=p.q, lq=p.lq, k=p.k, w=p.w, n=p.n) for f in (0, 1)]
        sk_off, sk_h, sk_p, hit_off, hits = [0], [], [], [0], []
        for ev in chunks:
            if len(ev):
                h0, h1 = rms[0].hits(ev), rms[1].hits(ev)
                assert np.array_equal(h0, h1), "the two builds seed differently"
                s0, s1 = ref_sketch(rms[0].lib, ev, p), ref_sketch(rms[1].lib, ev, p)
                assert np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1])
            else:   # (ri_sketch_min asserts len > 0; an empty chunk has no sketch and no hits)
                h0, s0 = np.zeros((0, 4), np.uint32), (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
            sk_h.append(s0[0]); sk_p.append(s0[1]); hits.append(h0)
            sk_off.append(sk_off[-1] + len(s0[0])); hit_off.append(hit_off[-1] + len(h0))
        out[name + "/sha256"] = np.frombuffer(sc.case_sha256(fwd, rev, chunks), np.uint8)
        out[name + "/sk_off"], out[name + "/hit_off"] = np.array(sk_off, np.int64), np.array(hit_off, np.int64)
        out[name + "/sk_hash"], out[name + "/sk_pos"] = np.concatenate(sk_h).astype(np.uint32), small(np.concatenate(sk_p))
        hh = np.concatenate(hits).astype(np.uint32).reshape(-1, 4)
        if len(hh) <= smc.MAX_ROWS:
            out[name + "/hits"] = small(hh)
        else:
            out[name + "/hits_sha256"] = np.frombuffer(smc.rows_sha256(hh), np.uint8)
        print("%-18s chunks %3d  sketch elements %6d  hits %8d  %s" % (name, len(chunks), sk_off[-1], hit_off[-1], "rows" if len(hh) <= smc.MAX_ROWS else "digest"))
    np.savez_compressed(smc.FIXTURE, **out)
    print(smc.FIXTURE, os.path.getsize(smc.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
