"""The device paths against the REFERENCE's own compiled rmap.cpp, through the fixture tests/golden/map_ref_*.npz alone (see
tests/test_map_ref.py and scripts/make_golden_map.py): the library's mapper with the chaining kernels of rawdtw_chain.hip and
the device DTW, the Python mirror with the device scorers, rawdtw_chain_round on every stored round's seed lists, and the
batch path (k_plan .. k_fold_select) on the stored candidate lists at the non-default --dtw-* options.  Bits and integers only."""
import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapper
from rawalign_amd.align import CandidateBatch
from rawalign_amd.mapping import StopOpt
from tests import map_ref_cases as K
from tests.test_map_ref import check_lines_after_c_chunks, check_lines_default_stop, check_round, replay, run_c_mapper, whole_read_lines_c
from tests.util import planner_options

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def fx():
    return K.Fixture()


@pytest.fixture(scope="module")
def eng(fx):
    e = ra.Engine(0)
    e.upload_reference(fx.ref.forward, fx.ref.reverse)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_rounds(fx):
    e = ra.Engine(0)   # (RoundScorer keeps the reads' events in slots of the context's event arena: a context of its own)
    e.upload_reference(fx.ref.forward, fx.ref.reverse)
    yield e
    e.close()


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("k,name", list(enumerate(K.OPTION_SETS)))
def test_device_mapper_against_the_reference(fx, eng, k, name, form):
    """CMapper with device_chain = 1: the anchor sort, chaining DP, traceback and evaluation order of rawdtw_chain.hip, the DTW,
    fold and selection on the device, the rest on the host -- the PAF fields the fixture holds, alns / aln of the cigar set
    included; groups 1 and 2; for the fused form also round by round (max_num_chunk = c, a stop rule that never fires)"""
    kw = dict(threads=4, groups=1 + (k + form) % 2, carry=False, device_chain=True)
    n = check_lines_default_stop(fx, name, form, run_c_mapper(fx, name, form, StopOpt(), engine=eng, **kw), "device mapper")
    assert n >= fx.n_reads // 2
    if form == 1:
        for c in range(1, max(fx.n_chunks(r) for r in range(fx.n_reads)) + 1):
            lines = run_c_mapper(fx, name, form, StopOpt(max_num_chunk=c, **K.NEVER), engine=eng, **kw)
            check_lines_after_c_chunks(fx, name, form, c, lines, "device mapper")


@pytest.mark.parametrize("name", ["default", "nofilter", "global_full"])
def test_device_mapper_with_rounds_the_device_declines(fx, name, monkeypatch):
    """RAWDTW_CHAIN_MAX_SEEDS lowered to 300: a read's first round (a chunk's hits) stays below it, later rounds (the chains'
    anchors on top) go over it and the round is chained on the host in the middle of a read"""
    monkeypatch.setenv("RAWDTW_CHAIN_MAX_SEEDS", "300")
    e = ra.Engine(0)
    e.upload_reference(fx.ref.forward, fx.ref.reverse)
    try:
        for groups in (1, 2):
            lines = run_c_mapper(fx, name, 1, StopOpt(**K.NEVER), engine=e, threads=3, groups=groups, carry=False, device_chain=True)
            check_lines_after_c_chunks(fx, name, 1, 99, lines, "device mapper, declined rounds")
            check_lines_default_stop(fx, name, 1, run_c_mapper(fx, name, 1, StopOpt(), engine=e, threads=3, groups=groups, carry=False, device_chain=True),
                                     "device mapper, declined rounds")
    finally:
        e.close()


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("name", list(K.OPTION_SETS))
def test_python_mirror_with_the_device_scorers_against_the_reference(fx, eng, eng_rounds, name, form):
    """mapper.map_reads with DeviceScorer (a batch a round) and RoundScorer (part costs carried from round to round on the
    device): every round's chains in full, the stop rule"""
    opt, copt = K.project_opts(name, form)
    if opt.flag & K.CIGAR:
        opt.flag &= ~K.CIGAR   # (the rounds are the default set's; the final alignment is the device mapper test's)
    reads = list(range(fx.n_reads))
    for what in ("DeviceScorer", "RoundScorer"):
        sc = mapper.DeviceScorer(eng) if what == "DeviceScorer" else mapper.RoundScorer(eng_rounds, 2048, fx.n_reads)
        seen = []

        def on_round(rnd, chains):
            for r, cs in chains.items():
                check_round(fx, name, form, r, rnd - 1, cs, opt, what)
                seen.append(r)
        mapper.map_reads(fx, reads, sc, opt, StopOpt(**K.NEVER), chain_opt=copt, on_round=on_round)
        assert len(seen) == sum(fx.n_chunks(r) for r in reads)
        if what == "RoundScorer":
            sc.close()


@pytest.mark.parametrize("name", ["default", "nbest5", "minanch3", "skips3", "band20", "nofilter"])
def test_chain_round_on_the_stored_seed_lists(fx, eng, name):
    """rawdtw_chain_round directly: per round every read's seeds -- the anchors of the chains the fixture holds for the round
    before, then the chunk's hits, as the mapper adds them -- against the fixture's candidate records in evaluation order
    (chaining score bits, sequence, strand, anchors), the survivors among them being the reference's own chains"""
    from tests.test_device_chain import SEED_DTYPE, device_round

    opt, copt = K.project_opts(name, 1)
    per_round = {}
    gen = replay(fx, name, 1, lists := [])
    for r, rnd, cands, _ in gen:
        if cands is None:
            continue
        seeds = np.zeros(sum(len(a) for _, _, a in lists), SEED_DTYPE)
        at = 0
        for s, st, a in lists:   # (any order: the device sorts)
            seeds["key"][at:at + len(a)] = s * 2 + st
            seeds["target_position"][at:at + len(a)], seeds["query_position"][at:at + len(a)] = a["target_position"], a["query_position"]
            at += len(a)
        per_round.setdefault(rnd, []).append((r, seeds[np.random.default_rng(r).permutation(len(seeds))]))
    checked = 0
    for rnd, items in sorted(per_round.items()):
        st, chain_off, anchor_off, recs, anchors, _, _, _ = device_round(eng, copt, [s for _, s in items], n_keys=2 * len(fx.lens))
        assert st == 0, (name, rnd, st)
        for i, (r, _) in enumerate(items):
            want = fx.candidates(name, 1, r, rnd)
            c0, c1 = int(chain_off[i]), int(chain_off[i + 1])
            assert c1 - c0 == len(want), (name, r, rnd, c1 - c0, len(want))
            for j, k in enumerate(want):
                rec = recs[c0 + j]
                assert int(K.bits(rec["chaining_score"])) == int(k["chaining"]) and int(rec["key"]) == int(k["seq"]) * 2 + int(k["strand"]), (name, r, rnd, j)
                got = anchors[int(anchor_off[c0 + j]):int(anchor_off[c0 + j + 1])]
                assert len(got) == int(k["n_anchors"]) == int(rec["n_anchors"]) and bytes(K.anchors_digest(got)) == bytes(k["digest"]), (name, r, rnd, j)
                checked += 1
    assert checked > 100


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("name", ["default", "frac025", "frac004", "bonus06", "min5", "min60"])
def test_batch_path_on_the_stored_candidate_lists(fx, eng, oracle, name, form):
    """ra.Batch, device-planned (verify_plan() is True) and host-planned, on every (read, round)'s candidate list as one batch
    (a batch read per pair, its events those of the rounds so far): per-chain scores and keeps against the reference's
    align_chain record -- cut chains (-1e10) and ties included -- and per-part costs against the DTW oracle (the reference's
    compiled dtw.cpp where oracle/_ref holds it, the C restatement elsewhere)"""
    from oracle.loader import RefDTW

    dtw = RefDTW() if RefDTW.available() else oracle
    opt, copt = K.project_opts(name, form)
    ev_parts, chain_off, anchor_off, anchors, ref_base, read_base, want, owner = [], [0], [0], [], [], [], [], []
    at = 0
    for r, rnd, cands, events in replay(fx, name, form):
        if not cands:
            continue
        rec = fx.candidates(name, form, r, rnd)
        assert len(rec) == len(cands)
        for c, k in zip(cands, rec):
            assert bytes(K.anchors_digest(c.anchors)) == bytes(k["digest"])
            anchors.append(np.ascontiguousarray(c.anchors, ra.ANCHOR_DTYPE))
            anchor_off.append(anchor_off[-1] + len(c.anchors))
            ref_base.append(eng.reference_offset(c.reference_sequence_index, c.strand))
            read_base.append(at)
            want.append(int(k["score"]))
            owner.append((c, events))
        chain_off.append(len(want))
        ev_parts.append(events)
        at += len(events)
    cb = CandidateBatch(np.concatenate(ev_parts), np.array(chain_off, np.uint64), np.array(anchor_off, np.uint64), np.concatenate(anchors),
                        np.array(ref_base, np.uint64), np.array(read_base, np.uint32))
    eng.upload_events(cb.events)
    want = np.array(want, np.uint32)
    keep_want = want.view(np.float32) >= f32(opt.dtw_min_score)
    frac = f32(opt.dtw_band_radius_frac)
    for planned in (True, False):
        with planner_options(eng, **({} if planned else {"device_plan": 0})):
            b = ra.Batch(eng, opt, cb)
            assert b.verify_plan() is planned
            b.run()
            score, keep, jc = b.fetch(with_job_costs=True)
            b.close()
        bad = np.nonzero(score.view(np.uint32) != want)[0]
        assert len(bad) == 0, (name, form, planned, len(bad), bad[:5], score[bad[:5]], want.view(np.float32)[bad[:5]])
        assert np.array_equal(keep.astype(bool), keep_want)
        j = 0
        for ci, (c, events) in enumerate(owner):   # (the jobs are laid out chain by chain, a chain's parts in align_chain's order)
            a = c.anchors
            parts = len(a) - 1
            arr = fx.ref.forward[c.reference_sequence_index] if c.strand == 1 else fx.ref.reverse[c.reference_sequence_index]
            for p in range(parts):
                s, e = a[parts - p], a[parts - p - 1]
                n = int(e["query_position"]) - int(s["query_position"]) + 1
                m = int(e["target_position"]) - int(s["target_position"]) + 1
                R0 = max(1, int(f32(n) * frac))   # rmap.cpp:276
                w = dtw.dtw_banded(events[int(s["query_position"]):int(s["query_position"]) + n],
                                   arr[int(s["target_position"]):int(s["target_position"]) + m], R0, p != parts - 1)
                assert int(K.bits(jc[j + p])) == int(K.bits(w)), (name, form, planned, ci, p, n, m, R0)
            j += parts
        assert j == len(jc)


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("name", list(K.WHOLE_SETS))
def test_whole_reads_on_the_device_against_what_the_reference_printed(eng, name, form):
    """The whole-read record of tests/golden/map_ref_reads.npz (what the reference's map_worker_for printed for raw reads) against
    the device mapper fed the stored events and hits: chaining on the device and on the host, groups 1 and 2; every line whole,
    alns / aln of the cigar set (the device's traceback) included."""
    wr = K.WholeReads(form)
    want = [wr.expected_line(name, r) for r in range(wr.n_reads)]
    for dev, groups in ((True, 1), (True, 2), (False, 1)):
        got = whole_read_lines_c(wr, name, form, engine=eng, threads=3, groups=groups, carry=False, device_chain=dev)
        for r, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, form, dev, groups, r)


@pytest.mark.parametrize("form", K.FORMS)
def test_device_event_detection_on_the_raw_reads_against_the_reference(form):
    """Engine.detect_events (rawdtw_events.hip), plain and contracted, on every chunk of the raw reads against the events the
    reference's detect_events gave for them: bit for bit"""
    from rawalign_amd import events as E

    wr = K.WholeReads(form)
    chunks = [c for sig in K.make_raw_reads() for c in K.raw_chunks(sig)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint64)
    e = ra.Engine(0)
    try:
        eoff, ev = e.detect_events(np.concatenate(chunks), off, E.EventOptions(contracted=bool(form)))[:2]
        assert np.array_equal(np.asarray(eoff).astype(np.int64), wr.ev_off) and np.array_equal(np.asarray(ev, np.float32).view(np.uint32), wr.events.view(np.uint32))
    finally:
        e.close()
