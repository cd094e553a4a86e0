#!/usr/bin/env python
"""Record tests/golden/seed_ref.npz: the reference's own seeding on the cases of tests/seed_cases.py.

Needs oracle/_ref/libref_map{0,1}.so (make -C oracle ref_map, only where the reference's sources are).  Per case and chunk: the
sketch (the library's exported ri_sketch, src/rsketch.c:276, called through ctypes) and the hits in the order gen_chains meets
them (oracle.loader.RefMap.hits), from both builds, asserted equal.  The inputs are regenerated from seeds by
tests/seed_cases.py; the fixture keeps their SHA-256."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.loader import RefMap  # noqa: E402
from tests import seed_cases as sc  # noqa: E402


class Mm128V(C.Structure):
    """mm128_v (src/rsketch.h): size_t n, m; mm128_t *a"""
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.POINTER(C.c_uint64))]


def ref_sketch(lib, ev, p):
    """ri_sketch as gen_chains calls it (rmap.cpp:367: id 0, strand 0): (hash, pos) per element"""
    lib.ri_sketch.restype = None
    lib.ri_sketch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int] + [C.c_int] * 6 + [C.POINTER(Mm128V)]
    v = Mm128V(0, 0, None)
    ev = np.ascontiguousarray(ev, np.float32)
    lib.ri_sketch(None, ev.ctypes.data, 0, 0, len(ev), p.w, p.e, p.n, p.q, p.lq, p.k, C.byref(v))
    xy = np.array([v.a[i] for i in range(2 * v.n)], np.uint64).reshape(-1, 2)
    C.CDLL(None).free(v.a)
    return (xy[:, 0] >> np.uint64(6)).astype(np.uint32), ((xy[:, 1] & np.uint64(0xFFFFFFFF)) >> np.uint64(1)).astype(np.uint32)


def main():
    assert RefMap.available(), "build oracle/_ref first (make -C oracle ref_map)"
    out = {}
    for name in sc.CASES:
        fwd, rev, p, chunks = sc.build_case(name)
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
        out[name + "/sk_hash"], out[name + "/sk_pos"] = np.concatenate(sk_h), np.concatenate(sk_p).astype(np.uint16)
        hh = np.concatenate(hits)
        out[name + "/hits"] = hh.astype(np.uint16 if hh.size == 0 or hh.max() < 65536 else np.uint32)
        print("%-6s chunks %2d  sketch elements %5d  hits %6d  longest list %d" % (
            name, len(chunks), sk_off[-1], hit_off[-1], max([0] + [int(np.max(np.unique(h[:, 3], return_counts=True)[1])) for h in hits if len(h)])))
    np.savez_compressed(sc.FIXTURE, **out)
    print(sc.FIXTURE, os.path.getsize(sc.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
