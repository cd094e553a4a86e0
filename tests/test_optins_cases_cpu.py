"""The inputs of tests/test_optins_together_gpu.py have the shape its cases rely on -- decided on the host alone: per (read, round) the seed
count the device chaining will see (previous primary-chain anchors from the Python mirror with the oracle's scorer, the chunk's hits from
seeding.seed_hits_host, the events from the host's detection of the same windows), against the caps and figures written down in
tests/optins_cases.py.  A generator that drifts fails here, not silently on the GPU.  Run with -s to see the measured figures.  No device."""
import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex, SeedParams
from tests import map_ref_cases as mc
from tests import optins_cases as oc
from tests.test_signal_round_gpu import FLOW_CHUNKS, FLOW_READS, flow  # noqa: F401  (the fixture itself)


@pytest.fixture(scope="module")
def ref():
    return mc.make_reference()


@pytest.fixture(scope="module")
def raws():
    raws = mc.make_raw_reads()
    assert mc.raw_sha256(raws) == np.load(mc.READS)["raw_sha256"].tobytes(), "synth.make_genome_raw_reads or tests/map_ref_cases.py drifted"
    return raws


@pytest.fixture(scope="module")
def indexes(ref):
    return {0: SeedIndex.from_signals(ref.forward, ref.reverse, threads=4), 5: SeedIndex.from_signals(ref.forward, ref.reverse, SeedParams(w=5), threads=4)}


def figures(rounds, declined, *caps):
    prev = oc.with_previous(rounds)
    fc = oc.flat_counts(rounds)
    return dict(pairs=len(fc), smallest=fc[0], largest=fc[-1], median=int(np.median(fc)), maxima=oc.maxima(rounds), above=[oc.above(rounds, c) for c in caps],
                prev_reads=[p[0] for p in prev], prev_seeds=[p[1] for p in prev], declined=declined)


def check(got, want, cap, what):
    print(what, got)
    assert got["smallest"] <= cap < got["largest"], what               # reads on both sides of the cap
    assert 0 < got["above"][0] < got["pairs"], what                    # (the same, as rawdtw_chain_round_stats will count it)
    assert got["declined"] == 0, what                                  # every read the round end takes is kept: no previous seed from the host
    for k, v in want.items():
        assert got[k] == v, (what, k, got[k], v)


@pytest.mark.parametrize("form", mc.FORMS)
def test_whole_reads_have_chained_reads_on_both_sides_of_l_mix(oracle, ref, raws, indexes, form):
    """cases A and D.  The host's events and hits of the pA windows are the fixture's; the three option sets of case A chain the same lists
    (their DTW options change no primary chain of these reads); L_MIX cuts between them, L_ALL leaves the few reads with under 60 seeds to
    k_chain; under a stop rule that never fires C_FB lets rounds 1, 2 and 4 through and stops round 3"""
    wr = mc.WholeReads(form, ref=ref)
    src = oc.whole_chunks(indexes[0], wr, raws, form)
    for r in range(wr.n_reads):
        assert src.n_chunks(r) == wr.n_chunks(r)
        for c in range(wr.n_chunks(r)):
            ev, hits = wr.chunk(r, c)
            assert np.array_equal(src.chunk(r, c)[0].view(np.uint32), np.asarray(ev, np.float32).view(np.uint32)) and src.chunk(r, c)[1] == list(hits), (r, c)
    for name in oc.A_SETS:
        opt, copt = mc.whole_project_opts(name, form)
        got = figures(*oc.seed_counts(src, oracle, ref, opt, copt, StopOpt()), oc.L_MIX, oc.L_ALL)
        check(got, oc.WHOLE[form], oc.L_MIX, "whole reads, %s, build %d, L_MIX = %d, L_ALL = %d:" % (name, form, oc.L_MIX, oc.L_ALL))
        assert got["above"][0] < got["above"][1] < got["pairs"]
    if form == 0:
        opt, copt = mc.whole_project_opts("default", 0)
        got = figures(*oc.seed_counts(src, oracle, ref, opt, copt, oc.never()), oc.C_FB)
        print("whole reads, a stop rule that never fires, C_FB = %d:" % oc.C_FB, got)
        mx = got["maxima"]
        assert mx == oc.FB_MAXIMA and got["declined"] == 0
        assert list(zip(got["prev_reads"], got["prev_seeds"])) == oc.FB_PREVIOUS
        over = [k for k, m in enumerate(mx) if m > oc.C_FB]
        assert mx[0] <= oc.C_FB and over and over[0] >= 2 and any(m <= oc.C_FB for m in mx[over[0] + 1:])
        assert [m > oc.C_FB for m in mx] == oc.FB_FALLS_BACK
        assert max(mx) <= oc.ALL_ON["resident_chains"]   # (no read's chains outgrow a half of the store)


@pytest.mark.parametrize("form", mc.FORMS)
def test_whole_reads_under_the_minimizer_index_have_reads_on_both_sides_of_l_mix5(oracle, ref, raws, indexes, form):
    """case C"""
    wr = mc.WholeReads(form, ref=ref)
    src = oc.whole_chunks(indexes[5], wr, raws, form)
    opt, copt = mc.whole_project_opts("default", form)
    got = figures(*oc.seed_counts(src, oracle, ref, opt, copt, StopOpt()), oc.L_MIX5)
    check(got, oc.WHOLE5[form], oc.L_MIX5, "whole reads, w = 5, build %d, L_MIX5 = %d:" % (form, oc.L_MIX5))


def test_the_int16_flow_has_reads_on_both_sides_of_l_mix_flow(oracle, flow):  # noqa: F811
    """case B.  Under the default stop rule no read of the flow ever enters a round holding chains (the even reads map in their first round,
    the odd ones in the first round that is not from nowhere): the store's counters cannot move there.  The variant with a stop rule that asks
    for 100 anchors in a sole primary chain, and read 0's second window cut to 300 samples, has reads with previous anchors in every round
    from the second on, and read 0 sits round 2 out holding the 65 anchors round 1 left it."""
    sref = flow[0]
    src = oc.flow_chunks(flow, FLOW_READS, FLOW_CHUNKS)
    got = figures(*oc.seed_counts(src, oracle, sref, ra.MapOpt(), None, StopOpt()), oc.L_MIX_FLOW)
    check(got, oc.FLOW, oc.L_MIX_FLOW, "int16 flow, default stop rule, L_MIX_FLOW = %d:" % oc.L_MIX_FLOW)
    assert not any(got["prev_reads"])
    src = oc.flow_chunks(oc.flow_with_a_sitter(flow), FLOW_READS, FLOW_CHUNKS)
    assert len(src.chunk(oc.SITTER, 1)[0]) < StopOpt().min_events
    rounds, declined = oc.seed_counts(src, oracle, sref, ra.MapOpt(), None, StopOpt(**oc.SIT_STOP))
    got = figures(rounds, declined, oc.L_MIX_FLOW)
    check(got, oc.FLOW_SIT, oc.L_MIX_FLOW, "int16 flow with a read that sits out, L_MIX_FLOW = %d:" % oc.L_MIX_FLOW)
    assert got["prev_reads"][0] == 0 and all(got["prev_reads"][1:])
    assert oc.SITTER not in rounds[1] and rounds[2][oc.SITTER][0] == oc.SITTER_ANCHORS > 0
    assert sum(1 for row in rounds[1:] for r in row if r == 3) and 3 not in rounds[1]   # (the fixture's own short window: read 3, which holds no chains)


def test_the_constructed_read_has_more_chains_than_the_device_chaining_keeps(oracle):
    """the sixth case: in its second round read DECLINER has more than 32 candidate chains and fewer seeds than the device's cap, so the round
    is begun on the device and declined at its end; every other (read, round) stays far below both of the chaining's limits on chains (32, and
    16 when scores tie); the other three reads hold chains when that round comes"""
    dref, reads = oc.decline_case()
    si = SeedIndex.from_signals(dref.forward, dref.reverse, threads=4)
    src = oc.EventReads(si, reads, [len(x) for x in dref.forward])
    opt, copt = mc.whole_project_opts("default", 0)
    rounds, declined = oc.seed_counts(src, oracle, dref, opt, copt, oc.never())
    cands = oc.candidate_counts(src, oracle, dref, opt, copt, oc.never())
    print("the constructed decline:", oc.maxima(rounds), oc.with_previous(rounds), cands, declined)
    assert oc.maxima(rounds) == oc.DECLINE_MAXIMA and max(oc.DECLINE_MAXIMA) <= 2048 and declined == 0
    assert oc.with_previous(rounds) == oc.DECLINE_PREVIOUS
    for k, row in enumerate(cands):
        for r, n in row.items():
            if (r, k) == (oc.DECLINER, oc.DECLINED_ROUND):
                assert n == oc.DECLINE_CANDIDATES > 32
            else:
                assert 1 <= n <= 16, (r, k, n)
    assert oc.DECLINE_PREVIOUS[oc.DECLINED_ROUND][0] == 3 and oc.DECLINER in rounds[oc.DECLINED_ROUND]
