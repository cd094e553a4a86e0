"""The local border constraint on the device (include/rawdtw.h, "local border"; border_constraint == 2, opt-in by rawdtw_set_border_local):
the refusals with the setter off, batches from every hand-over against the numpy restatement (tests/local_cases.py) and the reference's
recorded answers (tests/golden/local_ref.npz), k_local_jobs' edges, every scoring class of the semiglobal launches in one batch, the
property local <= global, and the mapper's flows against mapper.map_reads with LocalScorer.  The premise of the property test is fixed on
the CPU (tests/test_local_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from rawalign_amd import mapper
from rawalign_amd.align import Batch, CandidateBatch, pack_anchors
from rawalign_amd.dtw import ANCHOR_DTYPE, CHAIN_REC_DTYPE, round_end_host
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex
from tests import local_cases as lc
from tests import map_ref_cases as mc
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu
INVALID, RANGE = 1, 4
KIND_FOLD, KIND_SELECT, KIND_SEMI = 6, 7, 11   # rawdtw_launches.h: kKindChainFold, kKindReadSelect, kKindSemiWave
HOOK = "RAWDTW_LOCAL_JOBS"                     # read when a context is created: "host" brings the anchors home instead of k_local_jobs
LOCAL_OPT = dict(dtw_border_constraint=2)


def vp(x):
    return C.c_void_p(x.ctypes.data)


class OnDevice:
    """device copies of a batch's anchors, ref_base and read_base, alive as long as this is"""

    def __init__(self, cb):
        arrs = (np.ascontiguousarray(cb.anchors, ANCHOR_DTYPE), np.ascontiguousarray(cb.ref_base, np.uint64), np.ascontiguousarray(cb.read_base, np.uint32))
        self.t = [torch.from_numpy(np.concatenate([a.view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])).to("cuda:0") for a in arrs]
        torch.cuda.synchronize()
        self.ptrs = [t.data_ptr() for t in self.t]


@pytest.fixture(scope="module")
def case():
    return lc.make_case()


@pytest.fixture(scope="module")
def fx(case):
    f = lc.Fixture()
    assert f.same_inputs(case), "rawalign_amd/synth.py or tests/local_cases.py drifted: regenerate with scripts/make_golden_local.py"
    return f


@pytest.fixture(scope="module")
def want(case, fx):
    """the case's job costs (the restatement's, which are the fixture's) and its scores and keeps under the default options"""
    costs = lc.job_costs(case.cb, case.arena)
    assert_bits_equal(costs, fx.z["slow"].view(np.float32), "restatement against the fixture")
    score, keep = lc.fold(case.cb, costs, ra.MapOpt(**LOCAL_OPT))
    assert 0 < keep.sum() < case.cb.n_chains
    return costs, score, keep


def engine_for(case, local=True):
    e = ra.Engine(0)
    e.upload_reference(case.ref.forward, case.ref.reverse)
    assert e.get_border_local() is False
    if local:
        e.set_border_local(True)
        assert e.get_border_local() is True
    cb, arena = case.rebased(e)
    e.upload_events(cb.events)
    return e, cb, arena


def check(got, want, what):
    costs, score, keep = want
    assert_bits_equal(got[0], score, what + ": scores")
    assert np.array_equal(got[1], keep), what
    assert_bits_equal(got[2], costs, what + ": job costs")


def sparse_still_scores(e, cb, arena, oracle):
    """a sparse + banded batch of the same chains on the context, against the oracle's sequential align_chain loop"""
    from oracle.loader import OrcOpt

    opt = ra.MapOpt()
    b = Batch(e, opt, cb)
    b.run()
    score, keep = b.fetch()
    b.close()
    oopt = OrcOpt(1, 1, opt.dtw_band_radius_frac, opt.dtw_match_bonus, opt.dtw_min_score, 1)
    for r in range(cb.n_reads):
        best = np.float32(0.0)
        for c in range(int(cb.chain_off[r]), int(cb.chain_off[r + 1])):
            a = cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])]
            s = np.float32(oracle.align_chain(a, arena[int(cb.ref_base[c])], cb.events[int(cb.read_base[c]):], oopt, float(best)))
            assert score[c].view(np.uint32) == s.view(np.uint32), (r, c, score[c], s)
            k = s >= np.float32(opt.dtw_min_score)
            assert bool(keep[c]) == bool(k)
            if k and s > best:
                best = s


# ---- off -------------------------------------------------------------------------------------------------------------------------------
def test_off_every_entry_point_refuses_2_and_the_context_goes_on(case, oracle):
    e, cb, arena = engine_for(case, local=False)
    lib, copt = e.lib, ra.MapOpt(**LOCAL_OPT).c_struct()
    host = [np.ascontiguousarray(x) for x in (cb.chain_off, cb.anchor_off, cb.anchors, cb.ref_base, cb.read_base)]
    dev, ca = OnDevice(cb), pack_anchors(lib, host[1], host[2])
    calls = {
        "create": lambda h: lib.rawdtw_batch_create(e._ctx, C.byref(copt), cb.n_reads, *(vp(x) for x in host), C.byref(h)),
        "submit": lambda h: lib.rawdtw_batch_submit(e._ctx, C.byref(copt), cb.n_reads, *(vp(x) for x in host), C.byref(h)),
        "submit_device": lambda h: lib.rawdtw_batch_submit_device(e._ctx, C.byref(copt), cb.n_reads, vp(host[0]), vp(host[1]),
                                                                  *(C.c_void_p(p) for p in dev.ptrs), C.byref(h)),
        "submit_compact": lambda h: lib.rawdtw_batch_submit_compact(e._ctx, C.byref(copt), cb.n_reads, vp(host[0]), vp(host[1]), vp(ca.heads), vp(ca.unit_abs),
                                                                    vp(ca.steps), vp(ca.wide), len(ca.wide), vp(host[3]), vp(host[4]), C.byref(h)),
    }
    for name, call in calls.items():
        h = C.c_void_p()
        assert call(h) == INVALID and not h.value, name
        assert b"invalid border constraint" in lib.rawdtw_last_error(e._ctx), name
        sparse_still_scores(e, cb, arena, oracle)
    with pytest.raises(RuntimeError, match="rawdtw_mapper_create -> 1"):
        mapper.CMapper(e, ra.MapOpt(**LOCAL_OPT), StopOpt(), ["seq0"], [len(case.ref.forward[0])], slot_events=512, max_reads=4)
    sparse_still_scores(e, cb, arena, oracle)
    e.set_border_local(True)   # ... and off again: the refusal is back
    e.set_border_local(False)
    h = C.c_void_p()
    assert calls["submit"](h) == INVALID and not h.value
    for bad in (3, -1):   # any other value is refused as before, on or off
        e.set_border_local(bad == 3)
        copt.border_constraint = bad
        assert calls["create"](h) == INVALID and not h.value
    e.close()


# ---- on: results from every hand-over --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["create", "submit", "compact"])
def test_on_batches_from_host_arrays_and_compact_lists(case, want, how):
    e, cb, _ = engine_for(case)
    b = Batch(e, ra.MapOpt(**LOCAL_OPT), cb, compact=how == "compact", submit=how == "submit")
    b.run()
    check(b.fetch(with_job_costs=True), want, how)
    assert b.hand_over_stats() == dict(records_on_device=0, bytes_to_device=0, bytes_to_host=0)
    e.close()


@pytest.mark.parametrize("path", ["device", "host"])
def test_on_batches_from_device_arrays(case, want, path, monkeypatch):
    """rawdtw_batch_submit_device: k_local_jobs writes the records (two anchors a chain are read, 32 bytes a chain come home), or -- the hook
    set when the context is created -- every anchor comes home as for any other batch off the device-planned path"""
    if path == "host":
        monkeypatch.setenv(HOOK, "host")
    e, cb, _ = engine_for(case)
    monkeypatch.delenv(HOOK, raising=False)
    dev = OnDevice(cb)
    b = Batch(e, ra.MapOpt(**LOCAL_OPT), cb, device_ptrs=dev.ptrs)
    check(b.fetch(with_job_costs=True), want, path)
    nc, na = cb.n_chains, len(cb.anchors)
    assert b.hand_over_stats() == (dict(records_on_device=nc, bytes_to_device=8 * (nc + 1), bytes_to_host=32 * nc) if path == "device"
                                   else dict(records_on_device=0, bytes_to_device=0, bytes_to_host=8 * na + 12 * nc))
    b.run()   # a second run of the same batch
    check(b.fetch(with_job_costs=True), want, path + ", run again")
    b.close()
    # "resident_arrays": rawdtw_batch_create on the same device arrays
    e.set_option("resident_arrays", 1)
    h = C.c_void_p()
    copt = ra.MapOpt(**LOCAL_OPT).c_struct()
    host = [np.ascontiguousarray(cb.chain_off, np.uint64), np.ascontiguousarray(cb.anchor_off, np.uint64)]
    e._check(e.lib.rawdtw_batch_create(e._ctx, C.byref(copt), cb.n_reads, vp(host[0]), vp(host[1]), *(C.c_void_p(p) for p in dev.ptrs), C.byref(h)))
    e._check(e.lib.rawdtw_batch_run(e._ctx, h))
    got = (np.zeros(nc, np.float32), np.zeros(nc, np.uint8), np.zeros(nc, np.float32))
    e._check(e.lib.rawdtw_batch_fetch(e._ctx, h, *(vp(x) for x in got)))
    check(got, want, path + ", resident_arrays")
    e.set_option("resident_arrays", 0)
    e.lib.rawdtw_batch_destroy(h)
    e.close()


def test_on_every_batch_entry_point_works_on_a_local_batch(case, want):
    """info, run_timed, run_reps, enqueue / collect, launch_stats, verify_plan, fetch with job costs, the round end, destroy in any order and
    the context destroyed first"""
    e, cb, _ = engine_for(case)
    opt = ra.MapOpt(**LOCAL_OPT)
    b = Batch(e, opt, cb)
    jobs, job_off = b.build_jobs()
    wj, wo = lc.jobs(cb)
    assert jobs.tobytes() == wj.tobytes() and np.array_equal(job_off, wo)
    info = b.info()
    cells = int((jobs["n"].astype(np.int64) * jobs["m"]).sum())
    assert info["n_jobs"] == cb.n_chains == info["n_full_jobs"] and info["cells"] == cells and info["n_lane_jobs"] == 0
    assert b.verify_plan() is False   # (checked against the job list; not planned on the device)
    timed = b.run_timed()
    kinds = [k for k, _, _ in timed]
    assert kinds[-2:] == [KIND_FOLD, KIND_SELECT] and len(kinds) >= 3 and set(kinds[:-2]) == {KIND_SEMI}
    assert all(np.isfinite(ms) and ms >= 0 for _, _, ms in timed)
    check(b.fetch(with_job_costs=True), want, "run_timed")
    assert [(k, p) for k, p, _ in b.run_reps(3)] == [(k, p) for k, p, _ in timed]
    b.enqueue(True)
    b.enqueue(True)
    got, runs = b.collect()
    assert runs == 2 and [(k, p) for k, p, _ in got] == [(k, p) for k, p, _ in timed]
    st = b.launch_stats()
    assert [s["kind"] for s in st] == kinds and sum(s["n_jobs"] for s in st[:-2]) == cb.n_chains and sum(s["cells"] for s in st[:-2]) == cells
    assert {s["param"] for s in st[:-2]} <= {1, 2, 4, 8, 8 + 256}
    check(b.fetch(with_job_costs=True), want, "after the timed runs")
    # the round end on the batch's scores where they lie, against the host's
    recs = np.zeros(cb.n_chains, CHAIN_REC_DTYPE)
    for c in range(cb.n_chains):
        a = cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])]
        recs[c] = (np.float32(10 + 3 * len(a) + 0.25 * c), 0 if cb.ref_base[c] == cb.ref_base.min() else 1, a[-1]["target_position"], a[0]["target_position"], len(a))
    sel = StopOpt().c_struct(opt)
    b.round_end_begin(sel, recs)
    out, primary = b.round_end_fetch()
    w_out, w_primary = round_end_host(sel, cb.chain_off, recs, want[1], want[2])
    assert out.tobytes() == w_out.tobytes() and np.array_equal(primary, w_primary)
    # destroy in any order, and the context first
    b2, b3 = Batch(e, opt, cb, submit=True), Batch(e, opt, cb)
    check(b2.fetch(with_job_costs=True), want, "a second batch")
    b.close()
    h2, b2._h = b2._h, None   # (a batch that ran and one that never did outlive their context)
    h3, b3._h = b3._h, None
    ctx, e._ctx = e._ctx, None
    e.lib.rawdtw_destroy(ctx)
    assert e.lib.rawdtw_batch_destroy(h3) == 0 and e.lib.rawdtw_batch_destroy(h2) == 0


# ---- on: k_local_jobs' edges -----------------------------------------------------------------------------------------------------------
def edge_batch(nc, ref_len, n_events):
    """nc chains over one event array, eight to a read: three-anchor, one-anchor (n = m = 1), equal-query (n = 1), equal-target (m = 1) and
    two-anchor chains in turn; from three chains on, chains 0, nc // 2 and nc - 1 are empty -- the start anchor of chain nc - 2 (of the
    only chain when nc == 1) is then the anchor array's last element"""
    rng = np.random.default_rng(nc)
    anchors, aoff = [], [0]
    for c in range(nc):
        t0, q0 = int(rng.integers(0, ref_len - 80)), int(rng.integers(0, n_events - 60))
        n, m = int(rng.integers(2, 50)), int(rng.integers(2, 70))
        kind = c % 5
        if nc >= 3 and c in (0, nc // 2, nc - 1):
            lst = []
        elif kind == 0:
            lst = [(t0 + m - 1, q0 + n - 1), (t0 + m // 2, q0 + n // 2), (t0, q0)]
        elif kind == 1:
            lst = [(t0, q0)]
        elif kind == 2:
            lst = [(t0 + m - 1, q0), (t0, q0)]
        elif kind == 3:
            lst = [(t0, q0 + n - 1), (t0, q0)]
        else:
            lst = [(t0 + m - 1, q0 + n - 1), (t0, q0)]
        anchors.extend(lst)
        aoff.append(len(anchors))
    coff = list(range(0, nc, 8)) + [nc]
    return (np.array(coff, np.uint64), np.array(aoff, np.uint64), np.array(anchors, ANCHOR_DTYPE) if anchors else np.zeros(0, ANCHOR_DTYPE))


@pytest.mark.parametrize("path", ["device", "host"])
@pytest.mark.parametrize("nc", [1, 255, 256, 257])
def test_local_job_records_at_the_workgroups_edges(case, nc, path, monkeypatch):
    if path == "host":
        monkeypatch.setenv(HOOK, "host")
    e = ra.Engine(0)
    monkeypatch.delenv(HOOK, raising=False)
    e.upload_reference(case.ref.forward, case.ref.reverse)
    e.set_border_local(True)
    events = np.random.default_rng(5).normal(size=400).astype(np.float32)
    e.upload_events(events)
    L = len(case.ref.forward[0])
    coff, aoff, anchors = edge_batch(nc, L, len(events))
    strand = (np.arange(nc) % 2).astype(np.int64)
    offs = {s: e.reference_offset(0, s) for s in (0, 1)}
    cb = CandidateBatch(events, coff, aoff, anchors, np.array([offs[int(s)] for s in strand], np.uint64), np.zeros(nc, np.uint32))
    arena = {offs[1]: case.ref.forward[0], offs[0]: case.ref.reverse[0]}
    opt = ra.MapOpt(dtw_border_constraint=2, dtw_min_score=-4.0)   # (random events on a reference: scores lie around 0)
    costs = lc.job_costs(cb, arena)
    score, keep = lc.fold(cb, costs, opt)
    dev = OnDevice(cb)
    b = Batch(e, opt, cb, device_ptrs=dev.ptrs)
    check(b.fetch(with_job_costs=True), (costs, score, keep), "%d chains, %s" % (nc, path))
    jobs, _ = b.build_jobs()
    assert len(jobs) == len(costs) == nc - (3 if nc >= 3 else 0) and (jobs["n"] == 1).sum() >= len(jobs) // 5 and (jobs["m"] == 1).sum() >= len(jobs) // 5
    assert b.verify_plan() is False
    assert b.hand_over_stats()["records_on_device"] == (nc if path == "device" else 0)
    assert 0 < keep.sum() < nc or nc == 1
    e.close()


@pytest.mark.parametrize("path", ["device", "host"])
def test_a_reference_base_beyond_32_bits_is_out_of_range_on_both_paths(case, path, monkeypatch):
    """ref_base = 2^32 + 7 against an arena of a few thousand signals: a sum wrapped to 32 bits would lie inside it"""
    if path == "host":
        monkeypatch.setenv(HOOK, "host")
    e, cb, _ = engine_for(case)
    monkeypatch.delenv(HOOK, raising=False)
    far = CandidateBatch(cb.events, cb.chain_off, cb.anchor_off, cb.anchors, np.full(cb.n_chains, (1 << 32) + 7, np.uint64), cb.read_base)
    dev = OnDevice(far)
    h = C.c_void_p()
    copt = ra.MapOpt(**LOCAL_OPT).c_struct()
    host = [np.ascontiguousarray(far.chain_off, np.uint64), np.ascontiguousarray(far.anchor_off, np.uint64)]
    st = e.lib.rawdtw_batch_submit_device(e._ctx, C.byref(copt), far.n_reads, vp(host[0]), vp(host[1]), *(C.c_void_p(p) for p in dev.ptrs), C.byref(h))
    assert st == RANGE and not h.value, e.lib.rawdtw_last_error(e._ctx)
    near = CandidateBatch(cb.events, cb.chain_off, cb.anchor_off, cb.anchors, cb.ref_base, np.full(cb.n_chains, len(cb.events), np.uint32))   # (the events too)
    with pytest.raises(ra.RawDTWError) as err:
        Batch(e, ra.MapOpt(**LOCAL_OPT), near)
    assert err.value.status == RANGE
    e.close()


# ---- on: every scoring class in one batch ------------------------------------------------------------------------------------------------
CLASS_N = (1, 64, 65, 128, 129, 256, 257, 512, 513, 1025, 1537)


def class_batch(e, ref_len):
    """a chain of two anchors for every n of CLASS_N and every m of 1, 63, 64, 65, about n / 2 and about 2 n; a read a chain"""
    anchors, t0 = [], 3
    for n in CLASS_N:
        for m in (1, 63, 64, 65, max(1, n // 2), 2 * n):
            anchors.extend([(t0 + m - 1, n - 1), (t0, 0)])
            t0 = (t0 + 17) % 90
    nc = len(anchors) // 2
    assert max(a[0] for a in anchors) < ref_len
    off = np.arange(nc + 1, dtype=np.uint64)
    return off.copy(), off * np.uint64(2), np.array(anchors, ANCHOR_DTYPE), np.full(nc, e.reference_offset(0, 1), np.uint64), np.zeros(nc, np.uint32)


@pytest.mark.parametrize("full_wg", [1, 0])
def test_every_scoring_class_in_one_batch(full_wg):
    rng = np.random.default_rng(31)
    fwd, rev = rng.normal(size=3300).astype(np.float32), rng.normal(size=3300).astype(np.float32)
    ev_a, ev_b = rng.normal(size=1600).astype(np.float32), rng.normal(size=1600).astype(np.float32)
    e = ra.Engine(0)
    e.upload_reference([fwd], [rev])
    e.set_border_local(True)
    e.set_option("full_wg", full_wg)
    arrs = class_batch(e, len(fwd))
    opt = ra.MapOpt(dtw_border_constraint=2, dtw_fill_method=0, dtw_min_score=-1e9)
    arena = {int(arrs[3][0]): fwd}
    e.upload_events(ev_a)
    b = Batch(e, opt, CandidateBatch(ev_a, *arrs))
    params = {s["param"] for s in b.launch_stats(with_cells=False)[:-2]}
    assert params == ({1, 2, 4, 8, 8 + 256} if full_wg else {1, 2, 4, 8}), params
    e.upload_events(ev_b)   # other events between create and run: a run reads the arenas as they are then
    for events, what in ((ev_b, "other events before the run"), (ev_b, "run again"), (ev_a, "the first events back")):
        e.upload_events(events)
        b.run()
        cb = CandidateBatch(events, *arrs)
        costs = lc.job_costs(cb, arena)
        score, keep = lc.fold(cb, costs, opt)
        check(b.fetch(with_job_costs=True), (costs, score, keep), "full_wg %d, %s" % (full_wg, what))
    assert not np.array_equal(lc.job_costs(CandidateBatch(ev_a, *arrs), arena), lc.job_costs(CandidateBatch(ev_b, *arrs), arena))
    e.close()


# ---- the property ------------------------------------------------------------------------------------------------------------------------
def test_local_costs_are_at_most_the_global_full_matrix_costs(case, want):
    """one candidate batch scored as local and as global + full: every job cost at most the global one as floats, strictly below for at least
    the quarter of the chains that tests/test_local_cpu.py fixed on this case"""
    e, cb, _ = engine_for(case)
    loc = Batch(e, ra.MapOpt(**LOCAL_OPT), cb, submit=True).fetch(with_job_costs=True)[2]
    glo = Batch(e, ra.MapOpt(dtw_border_constraint=0, dtw_fill_method=0), cb, submit=True).fetch(with_job_costs=True)[2]
    print("local", loc, "global", glo)
    assert_bits_equal(loc, want[0], "local job costs")
    assert len(loc) == len(glo) == cb.n_chains and np.isfinite(glo).all()
    assert (loc <= glo).all()
    assert (loc < glo).sum() * 4 >= cb.n_chains
    e.close()


# ---- the mapper ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref():
    return mc.make_reference()


@pytest.fixture(scope="module")
def six(ref):
    return SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)


@pytest.fixture(scope="module")
def wr(ref):
    return mc.WholeReads(0, ref=ref)


@pytest.fixture(scope="module")
def mirror(ref, wr):
    """{flag set: (lines, rounds)} of mapper.map_reads with LocalScorer on the recorded events and hits of the whole reads"""
    out = {}
    for name in ("default", "cigar"):
        opt, copt = mc.whole_project_opts(name, 0)
        opt.dtw_border_constraint = 2
        out[name] = mapper.map_reads(wr, list(range(wr.n_reads)), lc.LocalScorer(ref), opt, StopOpt(), chain_opt=copt, output_chains=True)
    assert sum(ln.split("\t")[4] in "+-" for ln in out["default"][0]) >= 5 and sum("\taln:s:(" in ln for ln in out["cigar"][0]) >= 3
    assert out["default"][1] >= 2
    return out


def local_mapper(ref, wr, name, options=None, **kw):
    e = ra.Engine(0)
    e.upload_reference(ref.forward, ref.reverse)
    e.set_border_local(True)
    for k, v in (options or {}).items():
        e.set_option(k, v)
        assert e.get_option(k) == v, k
    opt, copt = mc.whole_project_opts(name, 0)
    opt.dtw_border_constraint = 2
    cm = mapper.CMapper(e, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096, max_reads=wr.n_reads,
                        chain_opt=copt, output_chains=True, threads=3, carry=kw.pop("carry", False), **kw)
    return e, cm


def same_lines(got, want, what):
    for r, (g, w) in enumerate(zip(got[0], want[0])):
        assert g == w, (what, r)
    assert got[1] == want[1], what


@pytest.mark.parametrize("flow", ["plain", "plain_carry_2groups", "device_chain_1group", "device_chain_2groups"])
def test_mapper_rounds_give_the_mirrors_lines(ref, wr, mirror, flow):
    kw = {"plain": dict(groups=1), "plain_carry_2groups": dict(groups=2, carry=True), "device_chain_1group": dict(groups=1, device_chain=True),
          "device_chain_2groups": dict(groups=2, device_chain=True)}[flow]
    e, cm = local_mapper(ref, wr, "default", **kw)
    got = mapper.map_reads_c(wr, list(range(wr.n_reads)), cm)
    cm.set_banded_cigar(True)   # (does not touch a local mapper)
    cm.close()
    e.close()
    same_lines(got, mirror["default"], flow)


def test_mapper_seeded_resident_rounds_with_the_round_end_and_the_chains_on_the_device(ref, wr, six, mirror):
    e, cm = local_mapper(ref, wr, "default", options=dict(device_round_end=1, resident_chains=4096), groups=1, device_chain=True)
    got = mapper.map_reads_c(wr, list(range(wr.n_reads)), cm, seed_index=six, resident=True)
    res, re_, kp = cm.resident_stats(), cm.round_end_stats(), cm.kept_stats()
    print(res, re_, kp)
    cm.close()
    e.close()
    same_lines(got, mirror["default"], "seeded-resident")
    assert res["fallback_rounds"] == 0 and res["resident_rounds"] == got[1] and re_["reads_device"] > 0


def test_mapper_cigar_from_host_events(ref, wr, mirror):
    e, cm = local_mapper(ref, wr, "cigar", groups=1)
    got = mapper.map_reads_c(wr, list(range(wr.n_reads)), cm, banded_cigar=True)   # (the banded path's switch does not touch a local mapper)
    cm.close()
    e.close()
    same_lines(got, mirror["cigar"], "flag 0x4 from host events")


class ShiftedHits:
    """the whole reads with every seed hit D columns further left on the reference: the chains are the same (chaining sees differences
    only), a chain's window starts D columns early, and its path starts at column j0 = D"""
    D = 7

    def __init__(self, wr):
        self.wr, self.n_reads, self.lens, self.ref = wr, wr.n_reads, wr.lens, wr.ref

    def n_chunks(self, r):
        return self.wr.n_chunks(r)

    def read_job(self, r):
        return self.wr.read_job(r)

    def chunk(self, r, c):
        ev, hits = self.wr.chunk(r, c)
        return ev, [(s, st, t - self.D if t >= self.D else t, q) for s, st, t, q in hits]


def test_mapper_cigar_of_paths_that_start_past_column_0(ref, wr, monkeypatch):
    """the local finish seeds j with j0 and formats through the host formatter: against mapper.map_reads with LocalScorer, whose paths
    are rawdtw_semiglobal_tb_host's"""
    shifted, j0s, cigar = ShiftedHits(wr), [], lc.cigar

    def spy(a, b, s):
        out = cigar(a, b, s)
        j0s.append(out[4])
        return out

    monkeypatch.setattr(lc, "cigar", spy)
    opt, copt = mc.whole_project_opts("cigar", 0)
    opt.dtw_border_constraint = 2
    want = mapper.map_reads(shifted, list(range(wr.n_reads)), lc.LocalScorer(ref), opt, StopOpt(), chain_opt=copt, output_chains=True)
    assert len(j0s) >= 3 and min(j0s) > 0, j0s
    e, cm = local_mapper(ref, wr, "cigar", groups=1)
    got = mapper.map_reads_c(shifted, list(range(wr.n_reads)), cm)
    cm.close()
    e.close()
    same_lines(got, want, "flag 0x4 with j0 > 0")
    assert sum("\taln:s:(" in ln for ln in got[0]) >= 3


def test_mapper_cigar_from_the_arena_in_rounds_from_signal(ref, wr, six, mirror):
    from tests.test_signal_round_gpu import _Signal

    raws = mc.make_raw_reads()
    e, cm = local_mapper(ref, wr, "cigar", options=dict(signal_cigar=1), groups=1, device_chain=True)
    got = mapper.map_reads_c(_Signal(wr, raws), list(range(wr.n_reads)), cm, seed_index=six, signal=True, event_opt=ra.EventOptions(contracted=False))
    sg = cm.signal_stats()
    cm.close()
    e.close()
    same_lines(got, mirror["cigar"], "flag 0x4 from the arena")
    assert sg["event_bytes_crossed"] == 0 and sg["rounds"] == got[1]
