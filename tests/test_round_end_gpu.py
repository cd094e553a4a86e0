"""A round's end on the device (rawdtw_round_end, rawdtw_batch_round_end_begin / _fetch: rawalign_amd/csrc/rawdtw_round_end.hip) against
the host restatement rawdtw_round_end_host -- which tests/test_round_end_host.py ties to the reference's own answers -- bit for bit:
primaries in order, mapq, the stop rule's answer.  Declined reads are excepted: their flag must be set exactly where one of the four
stated conditions holds (tests/round_end_cases.py: must_decline, from the host's results alone).  Then the forms on a batch's arrays in
device memory, a batch the device-planned path declined, and the mapper with the context's "device_round_end" on: the same lines and
log as with it off."""
import ctypes as C

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from rawalign_amd import mapper, synth
from rawalign_amd import mapping as M
from rawalign_amd.align import CandidateBatch
from rawalign_amd.dtw import ANCHOR_DTYPE, CHAIN_REC_DTYPE
from rawalign_amd.mapping import StopOpt
from tests import map_ref_cases as K
from tests import round_end_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = ra.Engine(0)
    yield e
    e.close()


def device(eng, rd):
    return eng.round_end(rd.opt, rd.chain_off, rd.recs, rd.score, rd.keep)


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("name", list(K.OPTION_SETS))
def test_fixture_rounds(eng, name, form):
    rd, want = R.fixture_round(name, form)
    got = device(eng, rd)
    assert not (got[0]["flags"] & R.ROUND_DECLINED).any()   # nothing of the fixture may decline
    R.assert_equal_except_declined(rd, got, rd.host(), (name, form))
    R.check_fixture_round(rd, want, got[0], got[1], ("device", name, form))


@pytest.mark.parametrize("case", [c[0] for c in R.random_rounds()])
def test_random_rounds(eng, case):
    rd = dict(R.random_rounds())[case]
    decl = R.assert_equal_except_declined(rd, device(eng, rd), rd.host(), case)
    assert (~decl).sum() >= 0.95 * rd.n_reads


@pytest.mark.parametrize("group", R.edge_groups())
def test_constructed_edges(eng, group):
    rd, es = R.edges_round(group)
    got = device(eng, rd)
    assert not (got[0]["flags"] & R.ROUND_DECLINED).any(), [n for n, o in zip(rd.names, got[0]) if o["flags"] & R.ROUND_DECLINED]
    R.assert_equal_except_declined(rd, got, rd.host(), group)


@pytest.mark.parametrize("evaluate", (0, 1))
def test_constructed_declines(eng, evaluate):
    rd = R.declines_round(evaluate)
    got = device(eng, rd)
    decl = R.assert_equal_except_declined(rd, got, rd.host(), evaluate)
    assert [bool(x) for x in decl] == [n is not None for n in rd.names]
    d = got[0][decl]   # a declined read's other outputs are void: zeroed, no primary listed
    assert (d["n_primary"] == 0).all() and (d["mapq"] == 0).all() and (d["flags"] == R.ROUND_DECLINED).all()
    owner = np.repeat(np.arange(rd.n_reads), np.diff(rd.chain_off).astype(np.int64))
    assert (got[1][decl[owner]] == R.NO_PRIMARY).all()


def test_no_chain_at_all_and_arguments(eng):
    so = R.select_opt(1)
    out, prim = eng.round_end(so, np.zeros(6, np.uint64), np.zeros(0, CHAIN_REC_DTYPE), np.zeros(0, np.float32), np.zeros(0, np.uint8))
    assert len(out) == 5 and not out["n_primary"].any() and not out["flags"].any() and len(prim) == 0
    out, prim = eng.round_end(so, np.zeros(1, np.uint64), np.zeros(0, CHAIN_REC_DTYPE), np.zeros(0, np.float32), None)   # no read: as the host form
    assert len(out) == 0 and len(prim) == 0 and len(ra.round_end_host(so, np.zeros(1, np.uint64), np.zeros(0, CHAIN_REC_DTYPE), np.zeros(0, np.float32))[0]) == 0
    with pytest.raises(ra.RawDTWError):   # offsets that do not ascend
        eng.round_end(so, np.array([0, 2, 1], np.uint64), np.zeros(2, CHAIN_REC_DTYPE), np.zeros(2, np.float32), np.zeros(2, np.uint8))
    with pytest.raises(ra.RawDTWError):   # EVALUATE_CHAINS without keep flags
        eng.round_end(so, np.array([0, 2], np.uint64), np.zeros(2, CHAIN_REC_DTYPE), np.zeros(2, np.float32), None)
    rd = dict(R.random_rounds())["n63-eval0-sel1"]   # without EVALUATE_CHAINS the keep flags are not read
    a, b = eng.round_end(rd.opt, rd.chain_off, rd.recs, rd.score, None), rd.host()
    R.assert_equal_except_declined(rd, a, b, "no keep")


# ---- a batch's arrays where they lie ---------------------------------------------------------------------------------------------
def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def recs_of(cb, rng):
    """records for a CandidateBatch's chains: positions from the anchors, a key per strand array, chaining scores descending a read"""
    recs = np.zeros(cb.n_chains, CHAIN_REC_DTYPE)
    keys = {int(b): k for k, b in enumerate(sorted(set(int(x) for x in cb.ref_base)))}
    for r in range(cb.n_reads):
        c0, c1 = int(cb.chain_off[r]), int(cb.chain_off[r + 1])
        recs["chaining_score"][c0:c1] = np.sort(rng.integers(10, 200, c1 - c0).astype(np.float32))[::-1]
    for c in range(cb.n_chains):
        a = cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])]
        recs[c]["key"], recs[c]["n_anchors"] = keys[int(cb.ref_base[c])], len(a)
        recs[c]["start_position"], recs[c]["end_position"] = a[-1]["target_position"], a[0]["target_position"]
    return recs


def test_a_batchs_round_end_through_the_python_face(eng):
    """Batch.round_end_begin / round_end_fetch behind Batch.run, the records copied up from the host: equal to the host restatement on the
    batch's fetched score and keep, under both evaluate_chains values; one round end at a time a context"""
    rng = np.random.default_rng(3)
    sref = synth.make_reference([60_000], seed=11)
    e2 = ra.Engine(0)
    e2.upload_reference(sref.forward, sref.reverse)
    offs = {(0, st): e2.reference_offset(0, st) for st in (0, 1)}
    cb, _ = synth.make_candidate_batch(sref, offs, synth.SynthParams(n_reads=200, max_chunks=3), seed=12)
    e2.upload_events(cb.events)
    recs = recs_of(cb, rng)
    b = ra.Batch(e2, ra.MapOpt(), cb)   # a batch destroyed with its round end begun takes it along: the context is free for the next
    b.run()
    b.round_end_begin(R.select_opt(1), recs)
    b.close()
    for evaluate in (1, 0):
        so = R.select_opt(evaluate)
        b = ra.Batch(e2, ra.MapOpt(), cb)
        b.run()
        b.round_end_begin(so, recs)
        with pytest.raises(ra.RawDTWError):
            b.round_end_begin(so, recs)
        score, keep = b.fetch()
        got = b.round_end_fetch()
        with pytest.raises(ra.RawDTWError):
            b.round_end_fetch()
        b.close()
        want = ra.round_end_host(so, cb.chain_off, recs, score, keep)
        rd = R.Round([], evaluate)
        rd.chain_off, rd.recs, rd.score, rd.keep = np.asarray(cb.chain_off, np.uint64), recs, score, keep
        decl = R.assert_equal_except_declined(rd, got, want, evaluate)
        assert not decl.any() and (want[0]["n_primary"] > 0).sum() > cb.n_reads // 2
    e2.close()


def test_a_batch_the_device_planned_path_declines(eng):
    """A batch that runs out of pass slots is scored again through the job list when it is fetched: its round end, enqueued behind the
    first run, runs again on those scores -- whether the batch is fetched first or the round end"""
    from tests.test_stream_path import _chains, _medium

    rng = np.random.default_rng(77)
    ref = [rng.normal(size=60000).astype(np.float32), rng.normal(size=60000).astype(np.float32)]
    e2 = ra.Engine(0)
    e2.set_option("tile_lds_floats", 2048)
    e2.set_option("pass_pool", 1)
    e2.upload_reference([ref[0]], [ref[1]])
    events, chain_off, anchor_off, anchors, slot, read_base = _chains(rng, 300, 60000, _medium, (1, 30))
    ref_base = np.array([e2.reference_offset(0, 1 if s == 0 else 0) for s in slot], np.uint64)
    cb = CandidateBatch(events, chain_off, anchor_off, anchors, ref_base, read_base)
    e2.upload_events(events)
    recs = recs_of(cb, rng)
    so = R.select_opt(0)   # (random events against a random reference: hardly a chain is kept; without EVALUATE_CHAINS every one takes part)
    opt = ra.MapOpt(dtw_min_score=5.0)
    outs = []
    for fetch_first in (True, False):
        b = ra.Batch(e2, opt, cb)
        assert b.verify_plan() is False   # declined: more passes than slots
        b.run()
        b.round_end_begin(so, recs)
        if fetch_first:
            score, keep = b.fetch()
            got = b.round_end_fetch()
        else:
            got = b.round_end_fetch()
            score, keep = b.fetch()
        b.close()
        want = ra.round_end_host(so, cb.chain_off, recs, score, keep)
        rd = R.Round([], 0)
        rd.chain_off, rd.recs, rd.score, rd.keep = np.asarray(cb.chain_off, np.uint64), recs, score, keep
        decl = R.assert_equal_except_declined(rd, got, want, fetch_first)
        assert not decl.any() and (want[0]["n_primary"] > 0).sum() > 250 and (score != np.float32(-1e10)).sum() > 20
        outs.append(got)
    assert outs[0][0].tobytes() == outs[1][0].tobytes()
    e2.close()


def test_a_device_chained_batch_with_the_records_in_device_memory():
    """rawdtw_chain_round -> rawdtw_batch_submit_device -> rawdtw_batch_round_end_begin on rawdtw_chain_round_recs' array -> fetch: equal to
    rawdtw_round_end_host on that batch's fetched score and keep and the records the chaining sent home"""
    from tests.test_device_chain import REC_DTYPE, SEED_DTYPE

    ref = synth.make_reference([150_000], seed=31)
    n = 300
    seeds = mapper.SyntheticSeeds(ref, n, seed=9, max_chunks=2)
    e2 = ra.Engine(0)
    lib = e2.lib
    e2.upload_reference(ref.forward, ref.reverse)
    copt = M.default_chain_opt(6)
    evs, per_read, read_base = [], [], np.zeros(n, np.uint32)
    at = 0
    for r in range(n):
        ev, hits = seeds.chunk(r, 0)
        read_base[r] = at
        at += len(ev)
        evs.append(np.asarray(ev, np.float32))
        s = np.zeros(len(hits), SEED_DTYPE)
        for k, (sq, st, t, q) in enumerate(hits):
            s[k] = (sq * 2 + (1 if st else 0), t, q)
        per_read.append(s)
    e2.upload_events(np.concatenate(evs))
    key_base = np.array([e2.reference_offset(0, 0), e2.reference_offset(0, 1)], np.uint64)
    seed_off = np.zeros(n + 1, np.uint64)
    seed_off[1:] = np.cumsum([len(s) for s in per_read])
    allseeds = np.concatenate(per_read + [np.zeros(1, SEED_DTYPE)])
    cap = n * 32
    chain_off, anchor_off, recs = np.zeros(n + 1, np.uint64), np.zeros(cap + 1, np.uint64), np.zeros(cap, REC_DTYPE)
    anchors = np.zeros(int(seed_off[-1]) + 1, ANCHOR_DTYPE)
    d_a, d_rb, d_qb = C.c_void_p(), C.c_void_p(), C.c_void_p()
    with pytest.raises(ra.RawDTWError):
        e2.chain_round_recs()   # no chaining round yet
    assert lib.rawdtw_chain_round(e2._ctx, C.byref(copt), n, vp(seed_off), vp(allseeds), vp(read_base), 2, vp(key_base), vp(chain_off), vp(anchor_off), vp(recs), cap,
                                  vp(anchors), C.byref(d_a), C.byref(d_rb), C.byref(d_qb)) == 0
    nc = int(chain_off[-1])
    assert nc > n // 2
    d_recs = e2.chain_round_recs()
    assert d_recs
    for evaluate in (1, 0):
        so = R.select_opt(evaluate)
        co = ra.MapOpt().c_struct()
        h = C.c_void_p()
        assert lib.rawdtw_batch_submit_device(e2._ctx, C.byref(co), n, vp(chain_off), vp(anchor_off), d_a, d_rb, d_qb, C.byref(h)) == 0, lib.rawdtw_last_error(e2._ctx)
        assert lib.rawdtw_batch_round_end_begin(e2._ctx, h, C.byref(so), C.c_void_p(d_recs), 1) == 0, lib.rawdtw_last_error(e2._ctx)
        score, keep = np.zeros(nc + 1, np.float32), np.zeros(nc + 1, np.uint8)
        assert lib.rawdtw_batch_fetch(e2._ctx, h, vp(score), vp(keep), None) == 0
        out, prim = np.zeros(n, ra.ROUND_OUT_DTYPE), np.zeros(nc + 1, np.uint32)
        assert lib.rawdtw_batch_round_end_fetch(e2._ctx, h, vp(out), vp(prim)) == 0, lib.rawdtw_last_error(e2._ctx)
        assert lib.rawdtw_batch_destroy(h) == 0
        want = ra.round_end_host(so, chain_off, recs[:nc], score[:nc], keep[:nc])
        rd = R.Round([], evaluate)
        rd.chain_off, rd.recs, rd.score, rd.keep = chain_off, recs[:nc].astype(CHAIN_REC_DTYPE), score[:nc], keep[:nc]
        decl = R.assert_equal_except_declined(rd, (out, prim[:nc]), want, evaluate)
        assert not decl.any() and (out["flags"] & R.ROUND_HIGH).sum() > 20 and (out["n_primary"] >= 1).sum() > n // 2
    e2.close()


# ---- the mapper --------------------------------------------------------------------------------------------------------------------
NEVER = dict(min_bestmap_ratio=1e9, min_meanmap_ratio=1e9, min_chain_anchor=10 ** 6)


class WithTwin:
    """`seeds`, and one more read whose single chunk makes two identical chains: the same twenty targets hit from two stretches of the
    read that hold the same events, 500 apart -- equal chaining scores, positions, anchor counts and (the DTW sees the same numbers)
    alignment scores.  The device declines that read; the host ends it.  (Under global DTW: with sparse borders the second of two such
    chains is cut by the first one's score -- align_chain's attainable score counts a part's shared end event once, its final score
    twice -- and -1e10 is not the first one's score.)"""

    def __init__(self, seeds, ref, n):
        self.seeds, self.lens, self.n = seeds, seeds.lens, n
        rng = np.random.default_rng(8)
        half = rng.normal(0, 1, 500)
        half[20:231] = ref.forward[2][1000 + np.round(np.arange(211) * 1.1).astype(int)] + rng.normal(0, 0.05, 211)
        self.ev = np.concatenate([half, half]).astype(np.float32)
        self.hits = [(2, 1, 1000 + 11 * k, q0 + 20 + 10 * k) for q0 in (0, 500) for k in range(20)]

    def read_job(self, r):
        return self.seeds.read_job(r) if r < self.n else mapper.ReadJob("twin", qlen=4000, n_chunks_available=1)

    def chunk(self, r, c):
        return self.seeds.chunk(r, c) if r < self.n else (self.ev, self.hits)


@pytest.fixture(scope="module")
def seven():
    """the seven-sequence index of tests/test_mapper.py, 300 reads"""
    ref = synth.make_reference([20000, 35000, 12000, 8000, 26000, 15000, 30000], seed=20231005 + 9)
    n = 300
    return ref, n, mapper.SyntheticSeeds(ref, n, seed=13, max_chunks=4)


def run_mapper(ref, seeds, ids, opt, stop, groups, on):
    slot = max(max(rd["n_ev"] for rd in getattr(seeds, "seeds", seeds).reads), 1000) + 8
    e = ra.Engine(0)
    e.upload_reference(ref.forward, ref.reverse)
    e.set_option("device_round_end", int(on))
    assert e.get_option("device_round_end") == int(on)
    names, lens = [f"seq{s}" for s in range(ref.n_seq)], [len(x) for x in ref.forward]
    cm = mapper.CMapper(e, opt, stop, names, lens, slot_events=slot, max_reads=len(ids), carry=False, threads=4, groups=groups, device_chain=True)
    lines, rounds = mapper.map_reads_c(seeds, ids, cm)
    out = (lines, cm.log(), cm.round_end_stats(), rounds)
    cm.close()
    e.close()
    return out


@pytest.mark.parametrize("groups,stop,flag", [(1, StopOpt(), 0x2), (2, StopOpt(**NEVER), 0x2 | 0x8), (2, StopOpt(), 0x8), (1, StopOpt(**NEVER), 0x2)],
                         ids=["one-group-stop-rule", "two-groups-all-chunks-log-scores", "two-groups-log-scores-alone", "one-group-all-chunks"])
def test_mapper_lines_and_log_do_not_depend_on_the_option(seven, groups, stop, flag):
    ref, n, seeds = seven
    opt = ra.MapOpt(flag=flag)
    off = run_mapper(ref, seeds, list(range(n)), opt, stop, groups, False)
    on = run_mapper(ref, seeds, list(range(n)), opt, stop, groups, True)
    assert on[0] == off[0] and on[1] == off[1] and on[3] == off[3]
    assert bool(on[1]) == bool(flag & 0x8)
    if stop.min_chain_anchor == 2:   # (the stop rule: reads leave the rounds at different times)
        assert sum(1 for l in on[0] if l.split("\t")[4] in "+-") > n // 4
    assert off[2] == dict(rounds=0, reads_device=0, reads_declined=0)
    assert 0 < on[2]["rounds"] <= on[3] and on[2]["reads_device"] > n // 2 and on[3] >= 2


@pytest.mark.parametrize("flag", [0x8, 0x2 | 0x8])
def test_mapper_ends_a_declined_read_on_the_host(seven, flag):
    ref, n, seeds = seven
    n = 60
    tw = WithTwin(seeds, ref, n)
    ids = list(range(n + 1))
    opt = ra.MapOpt(dtw_border_constraint=0, flag=flag)
    off = run_mapper(ref, tw, ids, opt, StopOpt(), 2, False)
    on = run_mapper(ref, tw, ids, opt, StopOpt(), 2, True)
    assert on[0] == off[0] and on[1] == off[1]
    assert on[0][n].startswith("twin\t") and "\tnc:i:1\t" in on[0][n]   # two candidates on one stretch: one primary chain
    assert on[2]["reads_declined"] >= 1 and on[2]["reads_device"] > 0
