"""FASTA + k-mer pore model -> a complete .ind (signals and hash buckets, ri_idx_dump's layout) with the signals and the seed table
built on the device: Engine.reference_from_bases, SeedIndex.from_device, then index.write_index(buckets=).  A table with minimizer
windows (-w above 0) is built on the device too (rawdtw_seed_index_build_device_min); the signals are fetched for the file alone.
--resident: the table's slots and lists are built on the device as well (rawdtw_seed_index_build_resident) and fetched for the file:
the same .ind, byte for byte.
Usage: python scripts/build_index.py FASTA MODEL OUT.ind [-w 0 -e 6 -q 9 --lq 3] [--plain] [--resident] [--device 0]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rawalign_amd as ra  # noqa: E402
from rawalign_amd import index, refsig  # noqa: E402
from rawalign_amd.seeding import SeedIndex, SeedParams  # noqa: E402


def build_index(fasta: str, model: str, out: str, w=0, e=6, n=0, q=9, lq=3, contracted=True, device=0, threads=16, resident=False) -> dict:
    records = refsig.read_fasta(fasta)
    pore, k = refsig.read_pore_model(model)
    pars = SeedParams(w, e, n, q, lq, k)
    eng = ra.Engine(device)
    try:
        eng.reference_from_bases([s for _, s in records], pore, k, contracted)
        fwd = [eng.reference_fetch(i, 1) for i in range(len(records))]
        rev = [eng.reference_fetch(i, 0) for i in range(len(records))]
        six = SeedIndex.from_device(eng, pars, resident=True).fetch(eng) if resident else SeedIndex.from_device(eng, pars, minimizer=w > 0)
        # ri_idx_dump writes l_seq floats a strand (rawindex.cpp:293-295): the s_len values, then the k - 1 zeros ri_kcalloc left
        pad = [np.zeros(len(s) - len(x), np.float32) for (_, s), x in zip(records, fwd)]
        index.write_index(out, [name for name, _ in records], [np.concatenate([x, z]) for x, z in zip(fwd, pad)],
                          [np.concatenate([x, z]) for x, z in zip(rev, pad)], w=w, e=e, n=n, q=q, lq=lq, k=k, buckets=six)
        return {"n_seq": len(records), "k": k, "signals": int(sum(len(x) for x in fwd)), "keys": six.n_keys, "positions": six.n_positions,
                "bytes": os.path.getsize(out)}
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("fasta")
    ap.add_argument("model")
    ap.add_argument("out")
    ap.add_argument("-w", type=int, default=0)
    ap.add_argument("-e", type=int, default=6)
    ap.add_argument("-n", type=int, default=0)
    ap.add_argument("-q", type=int, default=9)
    ap.add_argument("--lq", type=int, default=3)
    ap.add_argument("--plain", action="store_true", help="one rounding an operation (default: the form an FMA build of the reference computes)")
    ap.add_argument("--resident", action="store_true", help="build the table's slots and lists on the device too, then fetch them")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    print(build_index(a.fasta, a.model, a.out, a.w, a.e, a.n, a.q, a.lq, not a.plain, a.device, resident=a.resident))


if __name__ == "__main__":
    main()
