"""--dtw-output-cigar through the rounds from signal (the context's "signal_cigar" option): rawdtw_mapper_finish takes every mapped read's
events from its slot of the event arena (rawdtw_traceback_arena_steps), no event crosses PCIe, and the alns:f: / aln:s: tags are the
reference's recorded ones (pA input) or those of the parent's path -- host events, rawdtw_mapper_round_seeded_resident, flag 0x4 -- on the
same windows; rawdtw_mapper_read_events against the host's detection.  Helpers come from tests/test_signal_round_gpu.py,
tests/test_optins_together_gpu.py and tests/map_ref_cases.py.

The int16 case of the recorded-lines test compares with the parent's path, not with the recorded lines: the fixtures' pA reads are floats
that no int16 sample and channel reproduce (tests/test_seed_gpu.py says the same of them), so a DAC read detects other events than the
reference recorded -- on the CPU, all 26 chunks of the nine reads differ from the fixture in every event, at 8 192 and at 65 536 levels.
What it asks is as much: every whole line, CIGAR included, equal to an independent path's that uploads host events."""
import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from rawalign_amd import mapper
from rawalign_amd.mapping import StopOpt
from rawalign_amd.rawsig import CHANNEL_DTYPE, Channel, detect_events_raw_host
from rawalign_amd.rawsig import channels as chan_array
from rawalign_amd.seeding import SeedIndex, SeedParams
from tests import map_ref_cases as mc
from tests import optins_cases as oc
from tests.test_rawsig_host import raw_batch
from tests.test_signal_round_gpu import FLOW_CHUNKS, FLOW_READS, _Signal, _whole_mapper, flow  # noqa: F401  (flow: the fixture itself)

pytestmark = pytest.mark.gpu
CAP = "RAWDTW_CHAIN_MAX_SEEDS"
OPTION = "signal_cigar"
CIGAR_FLAGS = mc.EVAL | mc.CIGAR
DAC = Channel(8192.0, 1450.0, 3.0)
FLOW_CAP = 700   # the int16 flow's per-round maxima of seeds a read are 734, 649, 722, 494 (tests/optins_cases.py): rounds 1 and 3 fall back


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


def has_cigar(line):
    return "\talns:f:" in line and "\taln:s:(" in line


class _DacSignal:
    """the fixtures' reads as int16 DAC samples of one channel, cut as mc.raw_chunks cuts them"""

    def __init__(self, wr, raws):
        self.wr = wr
        self.raw = [np.round(sig * (DAC.digitisation / DAC.range) - DAC.offset).astype(np.int16) for sig in raws]
        self.chunks = [mc.raw_chunks(r) for r in self.raw]
        assert [len(c) for c in self.chunks] == [wr.n_chunks(r) for r in range(wr.n_reads)]
        self.channels = chan_array(DAC, wr.n_reads)
        assert self.channels.dtype == CHANNEL_DTYPE and len(self.channels) == wr.n_reads

    def read_job(self, r):
        return self.wr.read_job(r)

    def window(self, r, c):
        return self.chunks[r][c]


def from_signal(ref, si, wr, src, name, form, options, stop=None):
    """map_reads_c(..., signal=True) on an engine with `options` set: (lines, rounds, signal stats, timing, resident stats)"""
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        for k, v in options.items():
            e.set_option(k, v)
            assert e.get_option(k) == v, k
        opt, copt = mc.whole_project_opts(name, form)
        cm = mapper.CMapper(e, opt, stop or StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096,
                            max_reads=wr.n_reads, chain_opt=copt, output_chains=True, threads=3, carry=False, groups=1, device_chain=True)
        got, rounds = mapper.map_reads_c(src, list(range(wr.n_reads)), cm, seed_index=si, signal=True, event_opt=ra.EventOptions(contracted=bool(form)))
        out = (got, rounds, cm.signal_stats(), cm.timing(), cm.resident_stats())
        cm.close()
        return out
    finally:
        e.close()


def parents_path(ref, si, wr, src, name, form, device_chain=True, resident=True):
    """the same reads as host events (tests/optins_cases.py: HostChunks) through rawdtw_mapper_round_seeded(_resident) on an engine with nothing
    set; rawdtw_mapper_finish uploads the host's copy: (lines, rounds)"""
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        opt, copt = mc.whole_project_opts(name, form)
        cm = mapper.CMapper(e, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096,
                            max_reads=wr.n_reads, chain_opt=copt, output_chains=True, threads=3, carry=False, groups=1, device_chain=device_chain)
        got, rounds = mapper.map_reads_c(src, list(range(wr.n_reads)), cm, seed_index=si, resident=resident)
        assert cm.signal_stats()["rounds"] == 0 and cm.timing()["event_bytes"] > 0
        cm.close()
        return got, rounds
    finally:
        e.close()


# ---- 1. the recorded lines ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("kind", ["pa", "int16"])
def test_cigar_lines_from_signal_with_no_event_crossing(ref, six, raw_reads, kind, form):
    wr = mc.WholeReads(form, ref=ref)
    if kind == "pa":
        src = _Signal(wr, raw_reads)
        want = [wr.expected_line("cigar", r) for r in range(wr.n_reads)]
    else:
        src = _DacSignal(wr, raw_reads)
        jobs = [wr.read_job(r) for r in range(wr.n_reads)]
        host = oc.HostChunks(six, src.chunks, wr.lens, jobs, ra.EventOptions(contracted=bool(form)), chan=DAC)
        want, _ = parents_path(ref, six, wr, host, "cigar", form)
    got, rounds, sg, tm, res = from_signal(ref, six, wr, src, "cigar", form, {OPTION: 1})
    print(kind, form, rounds, sg, res)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, (kind, form, r)
    assert sum(has_cigar(ln) for ln in got) >= 3      # (not a comparison of lines without the tags)
    assert sg["event_bytes_crossed"] == 0 and tm["event_bytes"] == 0
    assert sg["rounds"] == rounds > 0 and res["resident_rounds"] + res["fallback_rounds"] == rounds


def test_the_option_is_0_or_1_and_off_by_default(ref):
    e = ra.Engine(0)
    try:
        assert e.get_option(OPTION) == 0
        for bad in (2, -1, 1 << 40):
            with pytest.raises(ra.RawDTWError) as err:
                e.set_option(OPTION, bad)
            assert err.value.status == 1 and e.get_option(OPTION) == 0
        e.set_option(OPTION, 1)
        assert e.get_option(OPTION) == 1
        e.set_option(OPTION, 0)
        assert e.get_option(OPTION) == 0
    finally:
        e.close()


def test_the_option_through_the_environment(monkeypatch):
    monkeypatch.setenv("RAWDTW_OPTS", "signal_cigar=1")
    e = ra.Engine(0)
    try:
        assert e.get_option(OPTION) == 1
    finally:
        e.close()


# ---- 2. the five opt-ins on -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", mc.FORMS)
def test_cigar_lines_with_the_five_optins_on_equal_the_all_off_mappers(ref, six5, raw_reads, form, monkeypatch):
    """Expected: a mapper on an engine with nothing set, the chaining on the host, fed the host's events of the same windows through
    rawdtw_mapper_round_seeded against the w = 5 index (the host's sketch), its finish uploading the host's copy.  Under test: rounds from signal
    with "chain_long_seeds", "chain_max_chains", "seed_minimizer", "device_round_end" and "resident_chains" on, lists on both sides of the cap."""
    wr = mc.WholeReads(form, ref=ref)
    want, rounds0 = parents_path(ref, six5, wr, oc.whole_chunks(six5, wr, raw_reads, form), "cigar", form, device_chain=False, resident=False)
    monkeypatch.setenv(CAP, str(oc.L_MIX5))
    options = dict(oc.ALL_ON, seed_minimizer=1, chain_max_chains=64, **{OPTION: 1})
    got, rounds, sg, tm, res = from_signal(ref, six5, wr, _Signal(wr, raw_reads), "cigar", form, options)
    print(form, rounds, sg, res)
    assert got == want and rounds == rounds0
    assert sum(has_cigar(ln) for ln in got) >= 1
    assert sg["event_bytes_crossed"] == 0 and tm["event_bytes"] == 0 and res["fallback_rounds"] == 0


# ---- 3. the int16 flow: disturbed rounds, mixed round kinds, read_events ------------------------------------------------------------------
def cigar_flow(flw, monkeypatch, cap=None, first_cap=0, host_fed=()):
    """tests/test_signal_round_gpu.py's flow with flag 0x4 on both mappers.  A: the parent's path on an engine with nothing set (created before
    the cap is).  B: "signal_cigar" on, every round from int16 signal -- except that in round 2 the reads of `host_fed` get their chunk as host
    events through rawdtw_mapper_round_seeded_resident, in a call of their own.  Before the first round and after the last, B's read_events
    against the host's detection of what each read was fed.  -> (lines A, lines B, per round B's resident stats' increase, B's signal stats,
    B's timing)"""
    sref, si, chan, window, _ = flw
    n = FLOW_READS
    names, lens = ["synth_0"], [len(sref.forward[0])]
    opt = ra.MapOpt(flag=CIGAR_FLAGS)
    ea = ra.Engine(0)
    if cap:
        monkeypatch.setenv(CAP, str(cap))
    eb = ra.Engine(0)
    try:
        for e in (ea, eb):
            e.upload_reference(sref.forward, sref.reverse)
        eb.set_option(OPTION, 1)
        if first_cap:
            eb.set_option("signal_events_cap", first_cap)
        ca, cb = (mapper.CMapper(e, opt, StopOpt(), names, lens, slot_events=4096, max_reads=n, threads=3, carry=False, groups=1, device_chain=True)
                  for e in (ea, eb))
        ids = [ca.add_read("read_%d" % r, 4000 * FLOW_CHUNKS, FLOW_CHUNKS) for r in range(n)]
        assert ids == [cb.add_read("read_%d" % r, 4000 * FLOW_CHUNKS, FLOW_CHUNKS) for r in range(n)]
        assert all(len(cb.read_events(i)) == 0 for i in ids)   # no round yet
        fed, deltas = {r: [] for r in range(n)}, []
        for c in range(FLOW_CHUNKS):
            sa, sb = [ca.state(i) for i in ids], [cb.state(i) for i in ids]
            assert sa == sb, c
            act = [r for r in range(n) if not sa[r][0]]
            if not act:
                break
            wins = [window(r, c) for r in act]
            raw, off = raw_batch(wins)
            _, eoff, ev = ea.detect_events_raw(raw, off, chan)
            evs = [ev[int(eoff[k]):int(eoff[k + 1])] for k in range(len(act))]
            ca.round([ids[r] for r in act], [(x, []) for x in evs], seed_index=si, resident=True)
            before = cb.resident_stats()
            host_k = [k for k, r in enumerate(act) if c == 1 and r in host_fed]
            sig_k = [k for k in range(len(act)) if k not in host_k]
            if host_k:
                cb.round([ids[act[k]] for k in host_k], [(evs[k], []) for k in host_k], seed_index=si, resident=True)
            if sig_k:
                cb.round_signal([ids[act[k]] for k in sig_k], [wins[k] for k in sig_k], si, channels=chan)
            after = cb.resident_stats()
            deltas.append({k: after[k] - before[k] for k in after})
            for r, w in zip(act, wins):
                fed[r].append(w)
        assert [ca.state(i) for i in ids] == [cb.state(i) for i in ids]
        crossed = cb.signal_stats()["event_bytes_crossed"]
        want_ev = []   # what the host detects in the windows a read was fed, chunk behind chunk
        for r in range(n):
            raw, off = raw_batch(fed[r])
            want_ev.append(detect_events_raw_host(raw, off, chan, threads=4)[2])

        def check_read_events(cm, when):
            for r in range(n):
                got = cm.read_events(ids[r])
                assert len(got) == len(want_ev[r]) and np.array_equal(got.view(np.uint32), want_ev[r].view(np.uint32)), (when, r)

        check_read_events(ca, "A, out of the arena")
        check_read_events(cb, "B, out of the arena")
        assert ca.finish() == 0 and cb.finish() == 0
        assert cb.signal_stats()["event_bytes_crossed"] == crossed and cb.timing()["event_bytes"] == crossed   # the finish sent none up
        check_read_events(cb, "B after its finish: the arena is what it was")
        check_read_events(ca, "A after its finish: the host's copy")
        out = ([ca.paf(i) for i in ids], [cb.paf(i) for i in ids], deltas, cb.signal_stats(), cb.timing())
        ca.close()
        cb.close()
        return out
    finally:
        ea.close()
        eb.close()


@pytest.fixture(scope="module")
def undisturbed(flow):  # noqa: F811
    """the flow with nothing forced: computed once"""
    mp = pytest.MonkeyPatch()
    try:
        return cigar_flow(flow, mp)
    finally:
        mp.undo()


def test_the_int16_flow_with_cigar_equals_the_parents_path_and_read_events_the_hosts_detection(undisturbed):
    la, lb, deltas, sg, tm = undisturbed
    print(deltas, sg)
    assert la == lb
    assert sum(has_cigar(ln) for ln in lb) >= FLOW_READS // 2
    assert sg["event_bytes_crossed"] == 0 and tm["event_bytes"] == 0 and sg["retried_rounds"] == 0
    assert all(d["fallback_rounds"] == 0 for d in deltas)


def test_a_fall_back_between_resident_rounds_changes_no_line(flow, undisturbed, monkeypatch):  # noqa: F811
    la, lb, deltas, sg, tm = cigar_flow(flow, monkeypatch, cap=FLOW_CAP)
    fell = [d["fallback_rounds"] == 1 for d in deltas]
    print(fell, sg)
    assert any(fell[k] and not fell[k - 1] and not fell[k + 1] for k in range(1, len(fell) - 1)), fell
    assert la == lb == undisturbed[1]
    assert sg["event_bytes_crossed"] == 0 and tm["event_bytes"] == 0   # (a fall-back fetches hits, not events)


def test_a_retried_round_changes_no_line(flow, undisturbed, monkeypatch):  # noqa: F811
    la, lb, deltas, sg, tm = cigar_flow(flow, monkeypatch, first_cap=1)
    assert sg["retried_rounds"] > 0
    assert la == lb == undisturbed[1]
    assert sg["event_bytes_crossed"] == 0 and tm["event_bytes"] == 0


def test_reads_fed_a_chunk_of_host_events_between_rounds_from_signal(flow, undisturbed, monkeypatch):  # noqa: F811
    """a third of round 2's reads take their chunk as host events (rawdtw_mapper_round_seeded_resident), every other chunk comes from signal: the
    finish reads all of them in the arena, and the lines are the all-host-events mapper's"""
    host_fed = set(range(0, FLOW_READS, 3)) | {1, 5}
    la, lb, deltas, sg, tm = cigar_flow(flow, monkeypatch, host_fed=host_fed)
    assert la == lb == undisturbed[1]
    assert sg["event_bytes_crossed"] > 0 and sg["event_bytes_crossed"] == tm["event_bytes"]   # (that one chunk of those reads, nothing else)
    assert sg["rounds"] >= 2


# ---- 4. what stays refused -------------------------------------------------------------------------------------------------------------------
def test_an_external_scorer_is_still_refused_with_no_read_changed(ref, six, raw_reads):
    wr = mc.WholeReads(0, ref=ref)
    src = _Signal(wr, raw_reads)

    def scorer(*a):
        raise AssertionError("never called")

    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        e.set_option(OPTION, 1)
        opt, copt = mc.whole_project_opts("cigar", 0)
        # set before the first round: the round from signal is refused
        cm = _whole_mapper(e, wr, opt, copt)
        ids = [cm.add_read("read_%d" % r, src.read_job(r).qlen, wr.n_chunks(r)) for r in range(wr.n_reads)]
        cm.set_scorer(scorer)
        with pytest.raises(RuntimeError, match="status 5"):
            cm.round_signal(ids, [src.window(r, 0) for r in range(wr.n_reads)], six)
        assert all(cm.state(i) == (False, 0) for i in ids) and cm.stats()[0] == 0 and cm.signal_stats()["rounds"] == 0
        assert all(len(cm.read_events(i)) == 0 for i in ids)
        cm.close()
        # set after a round from signal: the scorer is refused, reads and lines stay
        cm = _whole_mapper(e, wr, opt, copt)
        ids = [cm.add_read("read_%d" % r, src.read_job(r).qlen, wr.n_chunks(r)) for r in range(wr.n_reads)]
        cm.round_signal(ids, [src.window(r, 0) for r in range(wr.n_reads)], six)
        states, lines, events = [cm.state(i) for i in ids], [cm.paf(i) for i in ids], [cm.read_events(i) for i in ids]
        with pytest.raises(RuntimeError, match="status 1.*before the first round"):
            cm.set_scorer(scorer)
        assert [cm.state(i) for i in ids] == states and [cm.paf(i) for i in ids] == lines and cm.signal_stats()["rounds"] == 1
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(events, [cm.read_events(i) for i in ids]))
        cm.close()
    finally:
        e.close()
