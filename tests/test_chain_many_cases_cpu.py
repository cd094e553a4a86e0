"""tests/chain_many_cases.py on the host alone: the rounds that tests/test_chain_many_gpu.py sends to the device do hold what they are there
for -- reads above 16 chains with equal scores, reads above 32 -- and the mapper's fixture stays within k_round_end's 64 chains a read.
The figures are printed; a generator that drifts fails here, without a GPU."""
import rawalign_amd as ra
from rawalign_amd import mapping as M
from rawalign_amd.mapping import StopOpt
from tests import chain_many_cases as cm
from tests import map_ref_cases as mc
from tests import optins_cases as oc


def test_the_constructed_round_has_many_chains_with_ties():
    lib, copt = ra.load_library(), M.default_chain_opt(6)
    per_read = cm.mixed_round()
    cnt, _ = cm.counts(lib, copt, per_read)
    print("mixed: tied above 16", cm.tied_above(cnt, 16), "above 32", cm.above(cnt, 32), "above 64", cm.above(cnt, 64), "most", max(n for n, _ in cnt))
    assert len(per_read) == 100 and cm.tied_above(cnt, 16) >= 30
    assert cm.above(cnt, 32) >= 10 and cm.above(cnt, 64) >= 1
    assert sum(1 for n, _ in cnt if n <= 16) >= 50   # (the random reads)
    assert max(int(s["key"].max()) for s in per_read) < cm.MIXED_KEYS


def test_the_seeded_round_has_reads_above_16_with_ties_and_above_32():
    lib, copt = ra.load_library(), M.default_chain_opt(6)
    reads, per_read = cm.seeded_round()
    cnt, _ = cm.counts(lib, copt, per_read)
    print("seeded: seeds a read", min(len(s) for s in per_read), max(len(s) for s in per_read), "tied above 16", cm.tied_above(cnt, 16),
          "above 32", cm.above(cnt, 32), "most", max(n for n, _ in cnt))
    assert len(reads) == len(per_read) == 60 and all(len(x) == 400 for x in reads)
    assert cm.tied_above(cnt, 16) >= 20 and cm.above(cnt, 32) >= 3
    assert max(len(s) for s in per_read) <= 2048 and sum(len(s) > 60 for s in per_read) >= 50   # (k_chain's reads; k_chain_long's under a cap of 60)
    assert max(int(s["key"].max()) for s in per_read if len(s)) < 2 * cm.N_SEQ


def test_the_mappers_reads_stay_within_64_chains_a_read_and_pass_32():
    from oracle.loader import Oracle

    src = cm.mapper_reads()
    opt, copt = mc.whole_project_opts("default", 0)
    for stop in (oc.never(), StopOpt()):
        rounds = oc.candidate_counts(src, Oracle(), cm.reference(), opt, copt, stop)
        most = [max(row.values()) for row in rounds]
        print("mapper: reads a round", [len(row) for row in rounds], "most chains a read", most, "reads above 32", [sum(v > 32 for v in row.values()) for row in rounds])
        assert len(rounds) == cm.MAPPER_CHUNKS and max(most) <= 64
        assert sum(v > 32 for v in rounds[0].values()) >= 1   # (the first round declines with the option off)
