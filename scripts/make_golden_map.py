#!/usr/bin/env python3
"""Record tests/golden/map_ref_inputs.npz and tests/golden/map_ref_rounds.npz: the answers of the REFERENCE's own mapping code.

Runs only where the reference's sources are: `make -C oracle ref_map` compiles src/rmap.cpp and the units it calls where they
lie into oracle/_ref/libref_map0.so (contraction off) and libref_map1.so (the FMA build); oracle/ref_map_wrap.cpp is the glue.
The fixtures hold data only, so tests/test_map_ref.py and tests/test_map_ref_gpu.py check against the reference anywhere.

    python scripts/make_golden_map.py

Inputs (tests/map_ref_cases.py): a three-sequence reference with one stretch copied exactly and two copied with noise, 42
event-level reads in chunks of 400 events, and nine raw reads drawn from the reference's genomes.  map_ref_inputs.npz holds, per (read, chunk), the events and the seed hits the
reference's ri_sketch + ri_idx_get give (both builds give the same: asserted), and the SHA-256 of the inputs.
map_ref_rounds.npz holds per option set and build ("<set>/<form>/..."), per (read, round):
  chains / chain_off   reg->chains after the round's gen_chains (CHAIN_REC: score bits, sequence, strand, mapq, start, end,
                       n_anchors, 8 bytes of the SHA-256 of the anchors)
  mapped               is_mapped_with_high_confidence under the default stop options (the run itself never stops: a read's
                       rounds up to its first mapped round are what the default stop rule would have run)
  cands / cand_off     the round's candidate chains in evaluation order (the project's host chaining: the reference does not
                       show them) with the reference's align_chain score each, scored in sequence with the running best of
                       rmap.cpp:515-524 (CAND_REC)
  and for the cigar set, per read that maps: the reference's align_chain(cigar) of the best chain at its stop round.
map_ref_reads.npz holds the whole-read route: per build and (raw read, chunk of 4000 samples) the reference's detect_events output
and its seed hits, and per option set (all with --output-chains), build and read the record map_worker_for leaves in reg0 (mapped,
ref_id, read and fragment positions, mapq, rev) and its tags without the wall-clock mt:f: -- what the reference itself prints.
The generator asserts that primary selection and mapq on the scored candidates reproduce what gen_chains returned, and the
coverage conditions printed at the end."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import map_ref_cases as K  # noqa: E402


def main():
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref_map"], check=True, capture_output=True)
    ref = K.make_reference()
    reads = K.make_reads(ref)
    zi = K.record_inputs(ref, reads)
    np.savez_compressed(K.INPUTS, **zi)
    fx = K.Fixture(zi, {}, ref)
    out = {}
    cov = dict(cut=0, below=0, kept=0, ties=0)
    for name in K.OPTION_SETS:
        for form in K.FORMS:
            K.run_set(fx, ref, name, form, out, cov)
    np.savez_compressed(K.ROUNDS, **out)
    whole = K.record_whole_reads(ref, K.make_raw_reads())
    np.savez_compressed(K.READS, **whole)
    for form in K.FORMS:
        recs = whole["default/%d/records" % form]
        print("whole reads, build %d: %d of %d mapped under the default options; ci: %s" % (
            form, int(recs[:, 0].sum()), len(recs), [str(t).split("\t")[0] for t in whole["default/%d/tags" % form]]))
    from tests.test_map_ref import coverage  # the same conditions the suite checks from the stored fixture

    coverage(K.Fixture(), verbose=True)
    print("candidate scores over all sets and builds: %d cut (-1e10), %d below dtw_min_score, %d kept; (read, round) pairs with tied chaining scores: %d"
          % (cov["cut"], cov["below"], cov["kept"], cov["ties"]))
    for p in (K.INPUTS, K.ROUNDS, K.READS):
        print("%s: %d bytes" % (os.path.relpath(p, ROOT), os.path.getsize(p)))


if __name__ == "__main__":
    main()
