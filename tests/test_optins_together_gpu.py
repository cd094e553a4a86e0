"""The opt-in device paths where they meet: rounds from signal (detection, rawdtw_seed_detected_begin and the chaining with no host step
between) with "device_round_end" (k_round_end), "resident_chains" (k_keep_primary, the writer launch that reads the store), "chain_long_seeds"
(k_chain_sort_long / k_chain_long) and "seed_minimizer" (k_seed_min) on one context -- each of them has a test file of its own, none of those
turns on more than it needs.  Expected lines are the reference's recorded ones (tests/golden/) or those of a mapper with every opt-in off on an
engine of its own; every case also reads, from the counters, that the paths it names ran, against figures the host alone arrived at
(tests/optins_cases.py, checked by tests/test_optins_cases_cpu.py).  RAWDTW_CHAIN_MAX_SEEDS is read when a context is created: it is set
before the engine under test, and after the engine of the all-off run."""
import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from rawalign_amd import mapper
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex, SeedParams
from tests import map_ref_cases as mc
from tests import optins_cases as oc
from tests.test_map_ref import check_lines_after_c_chunks, check_lines_default_stop
from tests.test_rawsig_host import raw_batch
from tests.test_round_keep_gpu import STRICT_SETS, drive, whole_mapper
from tests.test_signal_round_gpu import FLOW_CHUNKS, FLOW_READS, _Signal, flow  # noqa: F401  (flow: the fixture itself)

pytestmark = pytest.mark.gpu
CAP = "RAWDTW_CHAIN_MAX_SEEDS"
NO_KEPT = dict(reads_from_device=0, reads_from_host=0, seeds_from_device=0, seeds_from_host=0, reads_not_kept=0)


@pytest.fixture(scope="module")
def ref():
    return mc.make_reference()


@pytest.fixture(scope="module")
def six(ref):
    return SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)


@pytest.fixture(scope="module")
def six5(ref):
    return SeedIndex.from_signals(ref.forward, ref.reverse, SeedParams(w=5), threads=4)


@pytest.fixture(scope="module")
def raw_reads():
    raws = mc.make_raw_reads()
    assert mc.raw_sha256(raws) == np.load(mc.READS)["raw_sha256"].tobytes(), "synth.make_genome_raw_reads or tests/map_ref_cases.py drifted"
    return raws


def delta(after, before):
    return {k: after[k] - before[k] for k in after}


def whole_reads_from_signal(ref, si, wr, raw_reads, name, form, **more):
    """map_reads_c(..., signal=True) over the whole reads' pA windows on an engine with every opt-in on:
    (lines, rounds, signal / resident / round-end / kept stats, the context's chaining stats)"""
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        oc.all_on(e, **more)
        opt, copt = mc.whole_project_opts(name, form)
        cm = whole_mapper(e, wr, opt, copt)
        got, rounds = mapper.map_reads_c(_Signal(wr, raw_reads), list(range(wr.n_reads)), cm, seed_index=si, signal=True,
                                         event_opt=ra.EventOptions(contracted=bool(form)))
        out = (got, rounds, cm.signal_stats(), cm.resident_stats(), cm.round_end_stats(), cm.kept_stats(), e.chain_round_stats())
        cm.close()
        return out
    finally:
        e.close()


def check_counters(want, rounds, sg, res, re_, kp, ch, above):
    """what the host says the run must have counted (`want`: optins_cases.WHOLE / WHOLE5 of the build; `above`: the index of the cap)"""
    assert sg["event_bytes_crossed"] == 0 and sg["rounds"] == rounds
    assert res["fallback_rounds"] == 0 and res["resident_rounds"] == rounds == len(want["prev_reads"])
    assert ch["rounds"] == rounds
    assert 0 < ch["long_reads"] < want["pairs"] and ch["long_reads"] == want["above"][above]   # k_chain and k_chain_long both took reads
    assert re_["reads_device"] == want["pairs"] > 0 and re_["reads_declined"] == 0 and re_["rounds"] == rounds
    assert kp["seeds_from_device"] == sum(want["prev_seeds"]) > 0 and kp["reads_from_device"] == sum(want["prev_reads"]) > 0
    assert kp["seeds_from_host"] == 0 and kp["reads_from_host"] == 0 and kp["reads_not_kept"] == 0 and res["seed_bytes_to_device"] == 0


# ---- A. whole reads from pA signal, every opt-in on: the reference's lines ------------------------------------------------------------
@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("name,cap", [(n, "L_MIX") for n in oc.A_SETS] + [("default", "L_ALL")])
def test_whole_reads_from_signal_with_every_optin_on_give_the_references_lines(ref, six, raw_reads, name, cap, form, monkeypatch):
    """Detection, seeding, k_chain / k_chain_long, DTW, k_round_end and k_keep_primary with nothing of a round on the host but its counts: every
    line is the one the reference's map_worker_for left in the fixture.  At L_MIX half of the (read, round) pairs are above the cap, one is
    exactly at it; at L_ALL all but the four pairs of reads from nowhere are.  The reads that enter a round with chains take them from the
    store -- as many reads and seeds as the Python mirror counts -- and none from the host."""
    assert name in STRICT_SETS
    monkeypatch.setenv(CAP, str(getattr(oc, cap)))
    wr = mc.WholeReads(form, ref=ref)
    want = [wr.expected_line(name, r) for r in range(wr.n_reads)]
    got, rounds, sg, res, re_, kp, ch = whole_reads_from_signal(ref, six, wr, raw_reads, name, form)
    print(name, cap, form, rounds, sg, res, re_, kp, ch)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, cap, form, r)
    check_counters(oc.WHOLE[form], rounds, sg, res, re_, kp, ch, 0 if cap == "L_MIX" else 1)


# ---- B. the int16 flow, all on against all off ------------------------------------------------------------------------------------------
def flow_pair(flw, stop, monkeypatch):
    """mapper A: the parent's path with nothing set (rawdtw_detect_raw_begin + rawdtw_mapper_round_seeded_resident); mapper B:
    rawdtw_mapper_round_raw_resident with every opt-in on and the cap at L_MIX_FLOW.  Per round the same states.  -> (lines A, lines B, per round
    B's kept stats' increase, B's resident / signal / round-end stats, B's context's chaining stats)"""
    sref, si, chan, window, _ = flw
    n = FLOW_READS
    names, lens = ["synth_0"], [len(sref.forward[0])]
    ea = ra.Engine(0)
    monkeypatch.setenv(CAP, str(oc.L_MIX_FLOW))
    eb = ra.Engine(0)
    try:
        for e in (ea, eb):
            e.upload_reference(sref.forward, sref.reverse)
        oc.all_on(eb)
        ca, cb = (mapper.CMapper(e, ra.MapOpt(), stop, names, lens, slot_events=4096, max_reads=n, threads=3, carry=False, groups=1, device_chain=True)
                  for e in (ea, eb))
        ids = [ca.add_read("read_%d" % r, 4000 * FLOW_CHUNKS, FLOW_CHUNKS) for r in range(n)]
        assert ids == [cb.add_read("read_%d" % r, 4000 * FLOW_CHUNKS, FLOW_CHUNKS) for r in range(n)]
        deltas = []
        for c in range(FLOW_CHUNKS):
            sa, sb = [ca.state(i) for i in ids], [cb.state(i) for i in ids]
            assert sa == sb, c
            act = [r for r in range(n) if not sa[r][0]]
            if not act:
                break
            wins = [window(r, c) for r in act]
            raw, off = raw_batch(wins)
            _, eoff, ev = ea.detect_events_raw(raw, off, chan)
            ca.round([ids[r] for r in act], [(ev[int(eoff[k]):int(eoff[k + 1])], []) for k in range(len(act))], seed_index=si, resident=True)
            before = cb.kept_stats()
            cb.round_signal([ids[r] for r in act], wins, si, channels=chan)
            deltas.append(delta(cb.kept_stats(), before))
        assert [ca.state(i) for i in ids] == [cb.state(i) for i in ids]
        assert ca.finish() == 0 and cb.finish() == 0
        assert ea.chain_round_stats()["long_reads"] == 0 and ca.kept_stats() == NO_KEPT and ca.round_end_stats()["rounds"] == 0   # (A: nothing on)
        out = ([ca.paf(i) for i in ids], [cb.paf(i) for i in ids], deltas, cb.resident_stats(), cb.signal_stats(), cb.round_end_stats(), eb.chain_round_stats())
        ca.close()
        cb.close()
        return out
    finally:
        ea.close()
        eb.close()


def check_flow(want, la, lb, deltas, res, sg, re_, ch):
    assert la == lb
    assert sum("\t*\t" not in ln for ln in la) >= FLOW_READS // 2   # (they map: not a comparison of empty lines)
    rounds = len(deltas)
    assert rounds == len(want["prev_reads"]) == FLOW_CHUNKS
    assert sg["event_bytes_crossed"] == 0 and sg["rounds"] == rounds and res["fallback_rounds"] == 0 and res["resident_rounds"] == rounds
    assert 0 < ch["long_reads"] < want["pairs"] and ch["long_reads"] == want["above"][0]
    assert re_["reads_device"] == want["pairs"] and re_["reads_declined"] == 0
    for k, d in enumerate(deltas):   # every read that enters a round with chains takes them from the store, none from the host
        assert d == dict(NO_KEPT, reads_from_device=want["prev_reads"][k], seeds_from_device=want["prev_seeds"][k]), (k, d)
    assert res["seed_bytes_to_device"] == 0


def test_the_int16_flow_all_on_equals_all_off(flow, monkeypatch):  # noqa: F811
    """24 reads, 4 chunks, with a read that sits a round out, an empty window and an all-outlier one.  Under the default stop rule no read of this
    flow enters a round holding chains (tests/test_optins_cases_cpu.py): the store is reserved and written, and its counters of previous seeds
    stay 0 -- from either source.  The long path, the round end and the rounds from signal all run."""
    la, lb, deltas, res, sg, re_, ch = flow_pair(flow, StopOpt(), monkeypatch)
    print(deltas, res, sg, re_, ch)
    check_flow(oc.FLOW, la, lb, deltas, res, sg, re_, ch)
    assert not any(any(d.values()) for d in deltas)


def test_the_int16_flow_with_reads_that_go_on_takes_their_chains_from_the_store(flow, monkeypatch):  # noqa: F811
    """The same flow under a stop rule that asks for a sole primary chain of 100 anchors, read 0's second window cut to 300 samples: nothing is
    taken in round 1; from round 2 on reads are seeded from the device, as many and with as many seeds as the Python mirror counts; read 0 sits
    round 2 out and its 65 anchors of round 1 are among round 3's seeds from the device (the round's count is the mirror's, and none came from
    the host)."""
    la, lb, deltas, res, sg, re_, ch = flow_pair(oc.flow_with_a_sitter(flow), StopOpt(**oc.SIT_STOP), monkeypatch)
    print(deltas, res, sg, re_, ch)
    check_flow(oc.FLOW_SIT, la, lb, deltas, res, sg, re_, ch)
    assert not any(deltas[0].values()) and all(d["reads_from_device"] > 0 for d in deltas[1:])
    assert deltas[2]["seeds_from_device"] >= oc.SITTER_ANCHORS and deltas[2]["seeds_from_host"] == 0


# ---- C. a minimizer index, all on, from signal ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", mc.FORMS)
def test_a_minimizer_index_from_signal_with_every_optin_on_gives_the_host_sketchs_lines(ref, six5, raw_reads, form, monkeypatch):
    """Expected: a mapper with every opt-in off and the chaining on the host, fed the host's events of the same windows through
    rawdtw_mapper_round_seeded -- the host's sketch.  Under test: k_seed_min behind the detection, its hits laid down by the writer launch beside
    seeds from the store, lists on both sides of L_MIX5."""
    wr = mc.WholeReads(form, ref=ref)
    opt, copt = mc.whole_project_opts("default", form)
    src = oc.whole_chunks(six5, wr, raw_reads, form)
    e0 = ra.Engine(0)
    try:
        e0.upload_reference(ref.forward, ref.reverse)
        cm = mapper.CMapper(e0, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096, max_reads=wr.n_reads,
                            chain_opt=copt, output_chains=True, threads=3, carry=False, groups=1, device_chain=False)
        want, rounds0 = mapper.map_reads_c(src, list(range(wr.n_reads)), cm, seed_index=six5)
        assert cm.resident_stats() == dict(resident_rounds=0, fallback_rounds=0, hit_bytes_to_host=0, seed_bytes_to_device=0)
        assert cm.kept_stats() == NO_KEPT and cm.round_end_stats()["rounds"] == 0 and e0.chain_round_stats()["rounds"] == 0
        cm.close()
    finally:
        e0.close()
    monkeypatch.setenv(CAP, str(oc.L_MIX5))
    got, rounds, sg, res, re_, kp, ch = whole_reads_from_signal(ref, six5, wr, raw_reads, "default", form, seed_minimizer=1)
    print(form, rounds, sg, res, re_, kp, ch)
    assert got == want and rounds == rounds0
    assert sum("\t*\t" not in ln for ln in got) >= 1
    check_counters(oc.WHOLE5[form], rounds, sg, res, re_, kp, ch, 0)


# ---- D. a fall-back between resident rounds, with the store on ------------------------------------------------------------------------------
class _Watched:
    """a CMapper behind the interface tests/test_round_keep_gpu.py's drive asks for: every round's increase of the resident stats is noted; with
    `signal` a round's chunks are windows of samples and go through rawdtw_mapper_round_signal_resident"""

    def __init__(self, cm, signal):
        self.cm, self.signal, self.res = cm, signal, []

    def __getattr__(self, k):
        return getattr(self.cm, k)

    def round(self, ids, chunks, seed_index=None, resident=False):
        before = self.cm.resident_stats()
        if self.signal:
            self.cm.round_signal(ids, [c[0] for c in chunks], seed_index)
        else:
            self.cm.round(ids, chunks, seed_index=seed_index, resident=resident)
        self.res.append(delta(self.cm.resident_stats(), before))


class _Windows:
    """the whole reads' pA windows behind the interface drive asks of its reads"""

    def __init__(self, wr, raws):
        self.wr, self.sig, self.n_reads = wr, _Signal(wr, raws), wr.n_reads

    def n_chunks(self, r):
        return self.wr.n_chunks(r)

    def read_job(self, r):
        return self.wr.read_job(r)

    def chunk(self, r, c):
        return self.sig.window(r, c), []


def driven(ref, si, wr, reads, options, signal=False):
    """drive's rounds (all of them resident) on an engine of its own: (lines, per round (resident stats' increase, kept stats' increase), the totals)"""
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        for k, v in options.items():
            e.set_option(k, v)
        opt, copt = mc.whole_project_opts("default", 0)
        cm = _Watched(whole_mapper(e, wr, opt, copt, oc.never()), signal)
        lines, kept, _ = drive(cm, reads, si, lambda k: True)
        out = (lines, list(zip(cm.res, [d for _, d in kept])), cm.resident_stats(), cm.kept_stats(), e.chain_round_stats())
        cm.close()
        return out
    finally:
        e.close()


@pytest.mark.parametrize("signal", [False, True], ids=["events", "signal"])
def test_a_fall_back_between_resident_rounds_leaves_no_stale_half(ref, six, raw_reads, signal, monkeypatch):
    """The long path off and the cap at C_FB: rounds 1 and 2 stay resident, round 3 has a read above the cap and falls back at the begin, round 4
    is resident again.  In the round that fell back no counter of the store moves; in the round after it every read that holds chains sends them
    up from the host (no half survived the fall-back); the lines are those of the run with nothing on."""
    wr = mc.WholeReads(0, ref=ref)
    reads = _Windows(wr, raw_reads) if signal else wr
    off = driven(ref, six, wr, reads, {}, signal)
    assert off[2]["fallback_rounds"] == 0 and off[3] == NO_KEPT and off[4]["long_reads"] == 0
    monkeypatch.setenv(CAP, str(oc.C_FB))
    on = driven(ref, six, wr, reads, dict(device_round_end=1, resident_chains=4096), signal)
    print(on[1], on[2], on[3])
    assert on[0] == off[0]
    res, kp = on[2], on[3]
    assert res["fallback_rounds"] >= 1 and res["resident_rounds"] >= 2 and on[4]["long_reads"] == 0
    assert [d["fallback_rounds"] == 1 for d, _ in on[1]] == oc.FB_FALLS_BACK
    saw = set()
    for k, (d, kd) in enumerate(on[1]):
        n_prev, s_prev = oc.FB_PREVIOUS[k]
        assert d["fallback_rounds"] + d["resident_rounds"] == 1, k
        if d["fallback_rounds"]:
            assert kd == NO_KEPT and d["seed_bytes_to_device"] == 0 and d["hit_bytes_to_host"] > 0, k
            saw.add("fell back")
        elif k > 0 and on[1][k - 1][0]["fallback_rounds"]:
            assert kd == dict(NO_KEPT, reads_from_host=n_prev, seeds_from_host=s_prev) and n_prev > 0, (k, kd)
            saw.add("after a fall-back")
        else:
            assert kd == dict(NO_KEPT, reads_from_device=n_prev, seeds_from_device=s_prev), (k, kd)
            if k > 0:
                assert n_prev > 0
                saw.add("after a resident round")
    assert saw == {"fell back", "after a fall-back", "after a resident round"}
    assert res["seed_bytes_to_device"] == 12 * kp["seeds_from_host"] > 0


# ---- F. a round the chaining's end declines, with the store on -----------------------------------------------------------------------------------
def test_a_round_declined_at_the_chainings_end_leaves_no_stale_half():
    """A constructed read with 34 candidate chains in its second round (tests/optins_cases.py: decline_case): the round is begun resident --
    three reads laid down from the store -- and rawdtw_chain_round_end declines it, so it is chained on the host from the host's chains.  No
    counter of the store moves in it, the round after it takes every read's previous seeds from the host, the one after that from the device
    again; the lines are those of the run with nothing on, which declines the same round."""
    dref, chunks = oc.decline_case()
    si = SeedIndex.from_signals(dref.forward, dref.reverse, threads=4)
    src = oc.EventReads(si, chunks, [len(x) for x in dref.forward])
    off = driven(dref, si, src, src, {})
    on = driven(dref, si, src, src, dict(device_round_end=1, resident_chains=4096))
    print(on[1], on[2], on[3])
    assert on[0] == off[0] and sum("\tnc:i:0" not in ln for ln in on[0]) >= 3   # (the reads hold chains at the end)
    fell = [d["fallback_rounds"] == 1 for d, _ in on[1]]
    assert fell == [k == oc.DECLINED_ROUND for k in range(4)] == [d["fallback_rounds"] == 1 for d, _ in off[1]]
    for k, (d, kd) in enumerate(on[1]):
        n_prev, s_prev = oc.DECLINE_PREVIOUS[k]
        if fell[k]:
            assert kd == NO_KEPT and d["hit_bytes_to_host"] > 0 and n_prev > 0, (k, kd)
        elif k > 0 and fell[k - 1]:
            assert kd == dict(NO_KEPT, reads_from_host=n_prev, seeds_from_host=s_prev) and n_prev > 0, (k, kd)
        else:
            assert kd == dict(NO_KEPT, reads_from_device=n_prev, seeds_from_device=s_prev), (k, kd)
    assert on[1][3][1]["reads_from_device"] > 0
    # (the round that was declined had sent nothing up: its three reads with chains were laid down from the store)
    assert on[2]["seed_bytes_to_device"] == 12 * on[3]["seeds_from_host"] > 0 and on[1][oc.DECLINED_ROUND][0]["seed_bytes_to_device"] == 0


# ---- E. the plain device-chained mapper: the long path and the round end together ----------------------------------------------------------
def fixture_run(fx, name, form, stop, e, groups):
    opt, copt = mc.project_opts(name, form)
    cm = mapper.CMapper(e, opt, stop, ["seq%d" % s for s in range(len(fx.lens))], [int(x) for x in fx.lens], slot_events=2048, max_reads=fx.n_reads,
                        chain_opt=copt, output_chains=True, threads=3, groups=groups, carry=False, device_chain=True)
    lines, _ = mapper.map_reads_c(fx, list(range(fx.n_reads)), cm)
    st = cm.round_end_stats()
    cm.close()
    return lines, st


@pytest.mark.parametrize("name", ["default", "nofilter"])
def test_the_device_chained_mapper_ends_its_long_rounds_on_the_device(ref, name, monkeypatch):
    """tests/test_chain_long_mapper_gpu.py's cap of 300 with "device_round_end" on too, no resident rounds: the chains of k_chain_long go through the
    compaction into rawdtw_batch_submit_device and k_round_end; one group and two (the second context inherits "chain_long_seeds")."""
    monkeypatch.setenv(CAP, "300")
    fx = mc.Fixture(ref=ref)
    e = ra.Engine(0)
    try:
        e.upload_reference(fx.ref.forward, fx.ref.reverse)
        e.set_option("chain_long_seeds", 65536)
        e.set_option("device_round_end", 1)
        for groups in (1, 2):
            before = e.chain_round_stats()["long_reads"]
            lines, st = fixture_run(fx, name, 1, oc.never(), e, groups)
            check_lines_after_c_chunks(fx, name, 1, 99, lines, "device mapper, long path and round end")
            assert st["reads_device"] > 0 and st["rounds"] > 0, groups
            lines, st = fixture_run(fx, name, 1, StopOpt(), e, groups)
            check_lines_default_stop(fx, name, 1, lines, "device mapper, long path and round end")
            assert st["reads_device"] > 0 and st["rounds"] > 0, groups
            assert e.chain_round_stats()["long_reads"] > before, groups
            print(name, groups, st, e.chain_round_stats())
    finally:
        e.close()
