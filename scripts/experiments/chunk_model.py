"""CPU model of where the lanes of k_runs go, and of what a chunk boundary at the first radius-1 record is worth.  No GPU.

The batch: synth.make_candidate_batch, 2 048 reads on a 600 kb reference, default SynthParams (the bench batch's mix at 1/8
scale).  Its tile-class parts (radius <= 3, longer side <= 73) are cut into tiles of 512 anchors, each tile sorted by k_plan's
key (3 - R) * 64 + 63 - min(N, 63) and cut into chunks as run_dp cuts it (rawalign_amd/csrc/rawdtw_chunks.h); a chunk is
charged its longest side times the per-column cost of the body it runs (lane_dp_r1 15, lane_dp_r2 and
lane_dp_r12 36.5, lane_dp_gen 56, quad_dp_r3 30).  A tile is taken as one pass (the image budget is not modelled).  The
schedule: four waves pull a pass's chunks in order; every chunk costs a fixed 40 instructions on top (records, ballots, the
result store, the counter round trip -- a guess, the same for both maps).

Usage: python scripts/experiments/chunk_model.py [--reads 2048] [--genome 600000] [--hit-prob P] [--decoy-gap-median G]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from rawalign_amd import synth  # noqa: E402

COST = {"quad_r3": 30.0, "lane_r2": 36.5, "lane_r12": 36.5, "lane_r1": 15.0, "lane_gen": 56.0}
FIXED, WAVES, TILE = 40.0, 4, 512


def tile_parts(cb, frac=0.1, max_radius=3, max_n=73):
    """(tile, N, R) of every tile-class part: part i runs from anchors[i + 1] to anchors[i] and belongs to the tile of anchor i"""
    q = cb.anchors["query_position"].astype(np.int64)
    t = cb.anchors["target_position"].astype(np.int64)
    idx = np.arange(len(q) - 1)
    last = np.zeros(len(q), bool)  # a chain's last entry: no part ends there
    last[cb.anchor_off[1:].astype(np.int64) - 1] = True
    idx = idx[~last[:-1]]
    n, m = q[idx] - q[idx + 1] + 1, t[idx] - t[idx + 1] + 1
    r0 = np.maximum(1, (n.astype(np.float32) * np.float32(frac)).astype(np.int64))
    N, M = np.maximum(n, m), np.minimum(n, m)
    R = r0 + ((N - M) * r0 + N - 1) // N
    ok = (R <= max_radius) & (N <= max_n)
    return idx[ok] // TILE, N[ok], R[ok]


def chunks_of(N, R, split):
    """a sorted pass's chunks: (class, records, columns = its longest side)"""
    n_jobs = len(N)
    n3 = int(np.sum(R[:64] == 3))
    n_hi = int(np.sum(R >= 2)) if split else n_jobs
    out = []
    for lo in range(0, n3, 16):
        out.append(("quad_r3", min(16, n3 - lo), int(N[lo:min(lo + 16, n3)].max())))
    for a, b in ((n3, n_hi), (n_hi, n_jobs)):
        for lo in range(a, b, 64):
            hi = min(lo + 64, b)
            radii = set(R[lo:hi].tolist())
            cls = "lane_r2" if radii == {2} else "lane_r1" if radii == {1} else "lane_r12" if radii <= {1, 2} else "lane_gen"
            out.append((cls, hi - lo, int(N[lo:hi].max())))
    return out


def model(tiles, N, R, split):
    order = np.lexsort(((3 - R) * 64 + 63 - np.minimum(N, 63), tiles))  # by tile, then by the planner's key (stable)
    tiles, N, R = tiles[order], N[order], R[order]
    cuts = np.flatnonzero(np.diff(tiles)) + 1
    per = {c: {"jobs": 0, "chunks": 0, "chunk_columns": 0, "job_columns": 0} for c in COST}
    tot = crit = bal = 0.0
    n_pass = 0
    for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(N)]])):
        ch = chunks_of(N[a:b], R[a:b], split)
        at = a
        waves = [0.0] * WAVES
        for cls, recs, cols in ch:
            p = per[cls]
            p["jobs"] += recs; p["chunks"] += 1; p["chunk_columns"] += cols; p["job_columns"] += int(N[at:at + recs].sum())
            at += recs
            w = min(range(WAVES), key=lambda k: waves[k])  # the wave that is free first pulls the next chunk
            waves[w] += cols * COST[cls] + FIXED
        n_pass += 1
        tot += sum(waves); crit += max(waves); bal += sum(waves) / WAVES / max(waves)
    loop = sum(p["chunk_columns"] * COST[c] for c, p in per.items())
    for c, p in per.items():
        p["share_of_column_loop"] = round(p["chunk_columns"] * COST[c] / loop, 4)
        p["instructions_per_chunk"] = round(p["chunk_columns"] * COST[c] / p["chunks"], 1) if p["chunks"] else None
        p["occupancy"] = round(p["job_columns"] / ((16 if c == "quad_r3" else 64) * p["chunk_columns"]), 4) if p["chunks"] else None
    return {"passes": n_pass, "column_loop_instructions": loop, "instructions_per_pass": round(tot / n_pass, 1),
            "critical_path_per_pass": round(crit / n_pass, 1), "balance": round(bal / n_pass, 3), "classes": per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--genome", type=int, default=600_000)
    ap.add_argument("--hit-prob", type=float, default=None)
    ap.add_argument("--decoy-gap-median", type=float, default=None)
    args = ap.parse_args()
    ref = synth.make_reference([args.genome], seed=20231007)
    pad = (args.genome + 3) & ~3  # the arena's layout: forward, then reverse, 16-byte aligned
    P = synth.SynthParams(n_reads=args.reads)
    if args.hit_prob is not None:
        P.hit_prob = args.hit_prob
    if args.decoy_gap_median is not None:
        P.decoy_gap_median = args.decoy_gap_median
    cb, _ = synth.make_candidate_batch(ref, {(0, 1): 0, (0, 0): pad}, P, seed=20231007 + 7919)
    tiles, N, R = tile_parts(cb)
    res = {"reads": args.reads, "genome": args.genome, "tile_class_parts": int(len(N)),
           "flat": model(tiles, N, R, False), "split": model(tiles, N, R, True)}
    f, s = res["flat"], res["split"]
    res["delta"] = {"column_loop_instructions": round(s["column_loop_instructions"] / f["column_loop_instructions"] - 1, 4),
                    "instructions_per_pass": round(s["instructions_per_pass"] / f["instructions_per_pass"] - 1, 4),
                    "critical_path_per_pass": round(s["critical_path_per_pass"] / f["critical_path_per_pass"] - 1, 4),
                    "chunks": round(sum(p["chunks"] for p in s["classes"].values()) / sum(p["chunks"] for p in f["classes"].values()) - 1, 4)}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
