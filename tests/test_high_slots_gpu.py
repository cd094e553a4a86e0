"""The mapper at slot bases past 2^30 and 2^31 floats of its event arena: a metamorphic test.  A mapper of 65 536 events a slot and
2^15 + 16 reads (two groups: 2^16 + 32) owns an arena of 2^31 + 2^20 floats a group; slot_of's base, read_base, seg_dst, dst_start and
ev_start are uint32_t element offsets into it.  Fillers registered through rawdtw_mapper_add_read that never enter a round push the
reads under test into the slots on both sides of 2^30 and of 2^31 and into the top ones.  Every flow then has to give, byte for byte,
what an identical mapper without fillers gives -- PAF lines, log lines, CIGARs, rawdtw_mapper_read_events and the counters -- while
the existing suite pins those lines at low slots to the reference (tests/test_signal_round_gpu.py and its neighbours, whose reads and
helpers this uses)."""
import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from rawalign_amd import mapper
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex
from tests import map_ref_cases as mc
from tests import optins_cases as oc
from tests.test_signal_cigar_gpu import _DacSignal, has_cigar
from tests.test_signal_round_gpu import _Signal

pytestmark = pytest.mark.gpu
SLOT = 65536
MAX_READS = {1: (1 << 15) + 16, 2: (1 << 16) + 32}
AT_30, AT_31 = (1 << 30) // SLOT, (1 << 31) // SLOT   # the first slot whose base is 2^30, 2^31
# where the nine reads' events go, as places (slot base / SLOT) inside a group's arena: the first slot, the slots on both sides of the
# two marks -- one ends at the mark, the next begins there --, and the two at the very top
PLACES = (0, AT_30 - 1, AT_30, AT_30 + 1, AT_31 - 1, AT_31, AT_31 + 1, MAX_READS[1] - 2, MAX_READS[1] - 1)


def slots(groups):
    """the reads' slot numbers: group = slot % groups, place = slot / groups (slot_of); with two groups read k is in group k % 2, as it
    is without fillers (a context's own counters then see the same reads)"""
    return [p if groups == 1 else 2 * p + (k & 1) for k, p in enumerate(PLACES)]


def test_the_slots_are_where_they_should_be():
    for groups in (1, 2):
        s = slots(groups)
        assert s == sorted(s) and len(set(s)) == 9 and s[-1] // groups == MAX_READS[1] - 1 and s[-2] // groups == MAX_READS[1] - 2
        assert [x % groups for x in s] == [k % groups for k in range(9)]
        base = [(x // groups) * SLOT for x in s]
        assert base[1] + SLOT == 1 << 30 == base[2] and base[4] + SLOT == 1 << 31 == base[5] and base[-1] + SLOT == (MAX_READS[1]) * SLOT < 1 << 32
        assert {x % groups for x in s} == set(range(groups))


class Padded:
    """a CMapper whose k-th added read lands in slot targets[k]: fillers (one chunk promised, none ever given) take the slots between"""

    def __init__(self, cm, targets):
        self.cm, self.targets, self.ids, self.next_slot = cm, list(targets), [], 0

    def __getattr__(self, k):
        return getattr(self.cm, k)

    def add_read(self, name, qlen, n_chunks):
        want = self.targets[len(self.ids)]
        while self.next_slot < want:
            self.cm.add_read("filler_%d" % self.next_slot, 4000, 1)
            self.next_slot += 1
        self.ids.append(self.cm.add_read(name, qlen, n_chunks))
        self.next_slot += 1
        return self.ids[-1]


@pytest.fixture(scope="module")
def ref():
    return mc.make_reference()


@pytest.fixture(scope="module")
def six(ref):
    return SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)


@pytest.fixture(scope="module")
def raw_reads():
    return mc.make_raw_reads()


def run(ref, wr, src, targets, name="default", groups=1, device_chain=True, options=None, local=False, opt_kw=None, **map_kw):
    """one mapper of the high-slot shape on an engine of its own; targets None: no fillers, the reads in slots 0 .. 8
    -> dict(lines, log, events, counters)"""
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        for k, v in (options or {}).items():
            e.set_option(k, v)
            assert e.get_option(k) == v, k
        if local:
            e.set_border_local(True)
        opt, copt = mc.whole_project_opts(name, wr.form)
        for k, v in (opt_kw or {}).items():
            setattr(opt, k, v)
        cm = mapper.CMapper(e, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=SLOT,
                            max_reads=MAX_READS[groups], chain_opt=copt, output_chains=True, threads=3, carry=False, groups=groups,
                            device_chain=device_chain)
        pm = Padded(cm, targets if targets is not None else range(wr.n_reads))
        lines, rounds = mapper.map_reads_c(src, list(range(wr.n_reads)), pm, **map_kw)
        assert len(pm.ids) == wr.n_reads and (targets is None) == (pm.ids == list(range(wr.n_reads)))
        out = dict(lines=lines, rounds=rounds, log=[ln for ln in cm.log().splitlines() if "filler_" not in ln],
                   events=[cm.read_events(i).view(np.uint32).tolist() for i in pm.ids], states=[cm.state(i) for i in pm.ids],
                   counters=(cm.stats(), cm.resident_stats(), cm.round_end_stats(), cm.kept_stats(), cm.decline_stats(), cm.signal_stats(),
                             e.chain_round_stats()))
        cm.close()
        return out
    finally:
        e.close()


def same(high, low, what):
    for r, (g, w) in enumerate(zip(high["lines"], low["lines"])):
        assert g == w, (what, r)
    assert high["rounds"] == low["rounds"] and high["states"] == low["states"], what
    assert high["log"] == low["log"], what
    for r, (g, w) in enumerate(zip(high["events"], low["events"])):
        assert g == w, (what, "events of read", r)
    assert sum(len(x) for x in low["events"]) > 5000 and sum("\t*\t" not in ln for ln in low["lines"]) >= 5   # (reads with events that map)
    assert high["counters"] == low["counters"], what


def both(ref, wr, src, groups=1, **kw):
    low = run(ref, wr, src, None, groups=groups, **kw)
    high = run(ref, wr, src, slots(groups), groups=groups, **kw)
    return high, low


# ---- the flows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("device_chain", [False, True], ids=["host_chaining", "device_chaining"])
def test_plain_rounds_with_host_hits(ref, groups, device_chain):
    """rawdtw_mapper_round: events appended into the slots (seg_dst), batches with read_base there; chained on the host, or on the device
    (read_base in rawdtw_chain_round_begin, the batch from device arrays)"""
    wr = mc.WholeReads(1, ref=ref)
    high, low = both(ref, wr, wr, groups=groups, device_chain=device_chain)
    same(high, low, "plain rounds")
    assert high["lines"] == [wr.expected_line("default", r) for r in range(wr.n_reads)]


def test_seeded_resident_rounds_with_the_device_round_end_and_kept_chains(ref, six):
    """rawdtw_mapper_round_seeded_resident with "device_round_end" and "resident_chains": seeding reads the slots (ev_start), the round end and
    the keep store address by slot"""
    wr = mc.WholeReads(0, ref=ref)
    high, low = both(ref, wr, wr, options=dict(device_round_end=1, resident_chains=4096), seed_index=six, resident=True)
    same(high, low, "seeded resident rounds")
    _, res, re_, kp = low["counters"][:4]
    assert res["resident_rounds"] > 0 and re_["reads_device"] > 0 and kp["seeds_from_device"] > 0
    assert high["lines"] == [wr.expected_line("default", r) for r in range(wr.n_reads)]


@pytest.mark.parametrize("kind", ["pa", "int16"])
def test_rounds_from_signal_with_every_optin_on(ref, six, raw_reads, kind):
    """rawdtw_mapper_round_signal_resident / _raw_resident: detection writes into the slots (dst_start), seeding and chaining read them"""
    wr = mc.WholeReads(0, ref=ref)
    src = _Signal(wr, raw_reads) if kind == "pa" else _DacSignal(wr, raw_reads)
    high, low = both(ref, wr, src, options=dict(oc.ALL_ON), seed_index=six, signal=True, event_opt=ra.EventOptions(contracted=False))
    same(high, low, "rounds from signal")
    assert low["counters"][5]["event_bytes_crossed"] == 0 and low["counters"][5]["rounds"] == low["rounds"]
    if kind == "pa":
        assert high["lines"] == [wr.expected_line("default", r) for r in range(wr.n_reads)]


def test_cigar_from_the_arena(ref, six, raw_reads):
    """--dtw-output-cigar with "signal_cigar": the finish's traceback reads the events in their slots (rawdtw_traceback_arena_steps)"""
    wr = mc.WholeReads(0, ref=ref)
    high, low = both(ref, wr, _Signal(wr, raw_reads), name="cigar", options=dict(signal_cigar=1), seed_index=six, signal=True,
                     event_opt=ra.EventOptions(contracted=False))
    same(high, low, "cigar from the arena")
    assert sum(has_cigar(ln) for ln in low["lines"]) >= 3
    assert high["lines"] == [wr.expected_line("cigar", r) for r in range(wr.n_reads)]


def test_banded_cigar_from_the_arena(ref, six, raw_reads):
    """global + banded with rawdtw_mapper_set_banded_cigar: the banded traceback over the slots"""
    wr = mc.WholeReads(0, ref=ref)
    high, low = both(ref, wr, _Signal(wr, raw_reads), name="cigar", options=dict(signal_cigar=1), opt_kw=dict(dtw_border_constraint=0, dtw_fill_method=1),
                     seed_index=six, signal=True, event_opt=ra.EventOptions(contracted=False), banded_cigar=True)
    same(high, low, "banded cigar from the arena")
    assert sum(has_cigar(ln) for ln in low["lines"]) >= 3


@pytest.mark.parametrize("cigar", [False, True], ids=["scores", "cigar"])
def test_a_local_mapper(ref, six, raw_reads, cigar):
    """the local border constraint: k_local_jobs takes read_base from the device arrays, the semiglobal kernels read the slots; with
    --dtw-output-cigar the semiglobal traceback does"""
    wr = mc.WholeReads(0, ref=ref)
    kw = (dict(name="cigar", options=dict(signal_cigar=1), signal=True, event_opt=ra.EventOptions(contracted=False)) if cigar
          else dict(options=dict(device_round_end=1, resident_chains=4096), resident=True))
    high, low = both(ref, wr, _Signal(wr, raw_reads) if cigar else wr, local=True, opt_kw=dict(dtw_border_constraint=2), seed_index=six, **kw)
    same(high, low, "local mapper")
    if cigar:
        assert sum(has_cigar(ln) for ln in low["lines"]) >= 3
