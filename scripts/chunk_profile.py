"""Per-class profile of the tile launch for a bench batch (GPU box): how k_runs' waves are filled, counted on the host from the
plan the device left (rawdtw_batch_chunk_profile) -- per body class (quad radius 3 / radius 2 / radii 1 and 2 mixed / radius 1 /
generic) jobs, chunks, the chunks' columns, the jobs' own columns and the lane occupancy they give -- under the chunk map
k_runs walks ("split": the radius-1 records from a chunk boundary of their own) and under the map of the versions before it
("flat": cut every 64 records), both from the same records.  With the column costs of DESIGN section 5 the column-loop
instructions either map asks for.  Usage: python scripts/chunk_profile.py [n_reads] > profile.json"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (initialise torch's HIP runtime first)

import rawalign_amd as ra  # noqa: E402
from rawalign_amd import synth  # noqa: E402

COST = {"quad_r3": 30.0, "lane_r2": 36.5, "lane_r12": 36.5, "lane_r1": 15.0, "lane_gen": 56.0}  # instructions a column

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
ref = synth.make_reference([int(os.environ.get("RAWDTW_PROBE_GENOME", 4_600_000))], seed=20231007)
eng = ra.Engine(0)
eng.upload_reference(ref.forward, ref.reverse)
offs = {(0, st): eng.reference_offset(0, st) for st in (0, 1)}
cb, _ = synth.make_candidate_batch(ref, offs, synth.SynthParams(n_reads=n_reads), seed=20231007 + 7919)
eng.upload_events(cb.events)
b = ra.Batch(eng, ra.MapOpt(), cb)
assert b.verify_plan() is True
out = {"reads": n_reads, "anchors": int(len(cb.anchors))}
for name, flat in (("split", False), ("flat", True)):
    p = b.chunk_profile(flat_map=flat)
    p["column_loop_instructions"] = sum(p[c]["chunk_columns"] * COST[c] for c in COST)
    p["chunks"] = sum(p[c]["chunks"] for c in COST)
    out[name] = p
out["split_vs_flat"] = {"column_loop_instructions": out["split"]["column_loop_instructions"] - out["flat"]["column_loop_instructions"],
                        "chunks": out["split"]["chunks"] - out["flat"]["chunks"]}
print(json.dumps(out, indent=1))
b.close()
eng.close()
