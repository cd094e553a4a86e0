#!/usr/bin/env python3
"""Lane occupancy of the fold's adds for one bench-like batch (scripts/stream_probe.py's), counted on the host from chain_off /
anchor_off for two work splits: sum of parts / (64 x sum over waves of the longest lane's parts).  No device.

  windowed   a wave per 8 reads, a chain a lane (chain cA + lane + 64 k), the reads' stretch swept in windows of 2 048 costs from
             the top down: a window's inner loop runs for the lane with the most parts in it
  lanes      two waves per 64 reads, a read a lane: wave 0 the read's first chain, wave 1 its other chains one after the other

Usage: python scripts/fold_occupancy.py [n_reads] [out.json]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rawalign_amd import synth  # noqa: E402

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
ref = synth.make_reference([int(os.environ.get("RAWDTW_PROBE_GENOME", 4_600_000))], seed=20231007)
offs = {(0, 1): 0, (0, 0): (len(ref.forward[0]) + 3) & ~3}
cb, _ = synth.make_candidate_batch(ref, offs, synth.SynthParams(n_reads=n_reads), seed=20231007 + 7919)
chain_off, anchor_off = cb.chain_off.astype(np.int64), cb.anchor_off.astype(np.int64)
parts = np.maximum(np.diff(anchor_off) - 1, 0)
total = int(parts.sum())

# ---- the windowed split ----
WIN, READS = 2048, 8
w_waves, w_longest, w_windows = 0, 0, 0
for r0 in range(0, n_reads, READS):
    cA, cB = chain_off[r0], chain_off[min(r0 + READS, n_reads)]
    if cB <= cA:
        continue
    w_waves += 1
    aA, hi = anchor_off[cA], anchor_off[cB]
    lane_of = (np.arange(cA, cB) - cA) % 64
    lo_c, hi_c = anchor_off[cA:cB], anchor_off[cA + 1:cB + 1] - 1  # a chain's costs: [a0, a1 - 2]
    while hi > aA:
        lo4 = max(hi - WIN, aA) & ~3
        inside = np.maximum(np.minimum(hi_c, hi) - np.maximum(lo_c, lo4), 0)  # parts of every chain in [lo4, hi)
        per_lane = np.bincount(lane_of, weights=inside, minlength=64)
        w_longest += int(per_lane.max())
        w_windows += 1
        hi = lo4

# ---- a read a lane ----
first = np.zeros(n_reads, np.int64)
has = chain_off[1:] > chain_off[:-1]
first[has] = parts[chain_off[:-1][has]]
csum = np.concatenate([[0], np.cumsum(parts)])
rest = csum[chain_off[1:]] - csum[chain_off[:-1]] - first
l_longest = [0, 0]
for r0 in range(0, n_reads, 64):
    l_longest[0] += int(first[r0:r0 + 64].max())
    l_longest[1] += int(rest[r0:r0 + 64].max())
n_wg = (n_reads + 63) // 64
out = {
    "batch": {"reads": n_reads, "chains": int(cb.n_chains), "parts": total, "chains_per_read": round(cb.n_chains / n_reads, 3),
              "parts_first_chain_mean": round(float(first.mean()), 1), "parts_first_chain_max": int(first.max()),
              "parts_other_chains_of_a_read_mean": round(float(rest.mean()), 1), "parts_other_chains_of_a_read_max": int(rest.max())},
    "windowed": {"waves": w_waves, "windows": w_windows, "sum_longest_lane_parts": w_longest, "lane_occupancy": round(total / (64.0 * w_longest), 4)},
    "lanes": {"waves": 2 * n_wg, "sum_longest_lane_parts": {"wave0_first_chains": l_longest[0], "wave1_other_chains": l_longest[1]},
              "lane_occupancy": round(total / (64.0 * sum(l_longest)), 4),
              "lane_occupancy_wave0": round(float(first.sum()) / (64.0 * l_longest[0]), 4),
              "lane_occupancy_wave1": round(float(rest.sum()) / (64.0 * max(l_longest[1], 1)), 4)},
}
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    json.dump(out, open(sys.argv[2], "w"), indent=1)
