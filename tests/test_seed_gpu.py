"""Seeding on the device (include/rawdtw.h: rawdtw_seed_index_upload, rawdtw_seed_begin / rawdtw_seed_end, rawdtw_seed.hip, and
rawdtw_mapper_round_seeded on a device mapper) against the reference's recorded answers (tests/golden/) and against the host
path, hit for hit and in order: exact equality of integers everywhere.  Nothing here reads the reference itself."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapper, seeding, synth
from rawalign_amd._lib import RawDTWError
from rawalign_amd.events import PinnedArray
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import HIT_DTYPE, SeedIndex, SeedParams
from tests import map_ref_cases as mc
from tests import seed_cases as sc

pytestmark = pytest.mark.gpu
INVALID, RANGE, UNSUPPORTED = 1, 4, 5


@pytest.fixture(scope="module")
def ref():
    return mc.make_reference()


@pytest.fixture(scope="module")
def six(ref):
    return SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)


@pytest.fixture(scope="module")
def eng(six):
    e = ra.Engine(0)
    e.upload_seed_index(six)
    yield e
    e.close()


def same_hits(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in HIT_DTYPE.names:
        assert np.array_equal(got[f], want[f]), (what, f)


def check_against_host(eng, si, chunks, what, **kw):
    ev, off = sc.flat(chunks)
    want_off, want = seeding.seed_hits_host(si, ev, off, threads=16)
    got_off, got = eng.seed_hits(ev, off, **kw)
    assert np.array_equal(got_off, want_off), what
    same_hits(got, want, what)
    return want_off, want


# ---- 1. device = host = fixture ----------------------------------------------------------------------------------------------------
def test_device_equals_the_mapping_fixtures(eng, six):
    fx = mc.Fixture()
    hoff, hits = eng.seed_hits(fx.events, fx.ev_off)
    assert np.array_equal(hoff.astype(np.int64), fx.hit_off) and len(hits) == 10860
    same_hits(hits, fx.hits, "map_ref_inputs")
    for form in mc.FORMS:
        w = mc.WholeReads(form)
        hoff, hits = eng.seed_hits(w.events, w.ev_off)
        assert np.array_equal(hoff.astype(np.int64), w.hit_off)
        assert [tuple(int(v) for v in r) for r in sc.hit_rows(hits)] == [tuple(h) for h in w.hits]


@pytest.mark.parametrize("name", sc.DEVICE_CASES)
def test_device_equals_the_seeding_fixture(name):
    sfx = sc.Fixture()
    fwd, rev, p, chunks = sc.build_case(name)
    assert sc.case_sha256(fwd, rev, chunks) == sfx.sha(name)
    si = SeedIndex.from_signals(fwd, rev, p, threads=4)
    e = ra.Engine(0)
    try:
        e.upload_seed_index(si)
        for pinned in (True, False):
            ev, off = sc.flat(chunks)
            hoff, hits = e.seed_hits(ev, off, pinned=pinned)
            assert np.array_equal(hoff, sfx.hit_off(name)) and np.array_equal(sc.hit_rows(hits), sfx.hits(name)), (name, pinned)
        check_against_host(e, si, chunks, name)
        if name == "motif":   # the long-list path: one element's list above 1 024 positions
            assert np.unique(sc.hit_rows(hits)[:int(hoff[1]), 3], return_counts=True)[1].max() > 1024
    finally:
        e.close()


# ---- 2. a realistic batch ----------------------------------------------------------------------------------------------------------
REAL_BP, REAL_SEED, REAL_READS = 300_000, 777, 2048


def realistic_raw_reads(n=REAL_READS):
    """one 4 000-sample chunk a read, drawn from both strands of the genome behind synth.make_reference([REAL_BP], REAL_SEED)"""
    rng = np.random.default_rng(REAL_SEED + 1)
    g = synth.make_genome(REAL_BP, REAL_SEED)
    starts = rng.integers(0, REAL_BP - 800, n)
    raws = synth.make_genome_raw_reads(g, starts, [700] * n, rng.integers(0, 2, n), seed=REAL_SEED + 2)
    return [r[:4000] for r in raws]


def test_device_equals_host_on_a_realistic_batch():
    sref = synth.make_reference([REAL_BP], seed=REAL_SEED)
    si = SeedIndex.from_signals(sref.forward, sref.reverse, threads=16)
    raws = realistic_raw_reads()
    assert len(raws) >= 2048 and all(len(r) == 4000 for r in raws)
    e = ra.Engine(0)
    try:
        e.upload_seed_index(si)
        sig = np.concatenate(raws)
        eoff, ev = e.detect_events(sig, np.arange(len(raws) + 1, dtype=np.uint64) * 4000)
        chunks = [ev[int(eoff[k]):int(eoff[k + 1])] for k in range(len(raws))]
        want_off, want = check_against_host(e, si, chunks, "realistic")
        with_hits = int(np.count_nonzero(np.diff(want_off.astype(np.int64)) > 0))
        assert with_hits > 0.9 * len(raws), with_hits   # (the host's own count: the test cannot pass on empty output)
        # right hits among them: most chunks have a hit on their own strand
        assert len(want) > 4 * len(raws)
    finally:
        e.close()


# ---- 3. pinned and pageable, empty and short chunks inside a batch --------------------------------------------------------------------
def test_page_locked_and_pageable_results_and_empty_chunks(eng, six, ref):
    rng = np.random.default_rng(5)
    chunks = []
    for k in range(300):
        arr = (ref.forward, ref.reverse)[k % 2][k % 3]
        lo = int(rng.integers(0, len(arr) - 500))
        n = (0, 1, 5, 6, 7)[k % 5] if k % 4 == 0 else int(rng.integers(1, 500))
        chunks.append((arr[lo:lo + n] + np.float32(rng.normal(0, 0.04))).astype(np.float32))
    chunks[0], chunks[-1] = chunks[0][:0], chunks[-1][:0]   # (the batch's first and last chunk are empty)
    want_off, want = check_against_host(eng, six, chunks, "pinned", pinned=True)
    check_against_host(eng, six, chunks, "pageable", pinned=False)
    assert len(want) > 1000
    lib = ra.load_library()
    assert lib.rawdtw_host_is_page_locked(C.c_void_p(eng._seed_stage["hits"].ptr)) == 1
    ev, off = sc.flat(chunks)
    a = eng.seed_hits(ev, off, pinned=True, kernel_ms=True)
    assert a[2] > 0
    # no chunk at all, and chunks that are all empty
    hoff, hits = eng.seed_hits(np.zeros(0, np.float32), np.zeros(1, np.uint64))
    assert hoff.tolist() == [0] and len(hits) == 0
    hoff, hits = eng.seed_hits(np.zeros(0, np.float32), np.zeros(4, np.uint64))
    assert hoff.tolist() == [0, 0, 0, 0] and len(hits) == 0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_range_second_begin_unsupported_and_no_table(eng, six, ref):
    lib = ra.load_library()
    fx = mc.Fixture()
    n = 20
    ev, off = np.ascontiguousarray(fx.events[:int(fx.ev_off[n])]), np.ascontiguousarray(fx.ev_off[:n + 1], np.uint64)
    want_off, want = seeding.seed_hits_host(six, ev, off)
    total = int(want_off[-1])
    assert total > 100
    vp = lambda a: a.ctypes.data  # noqa: E731
    for pinned in (True, False):   # a cap one too small: RANGE from _end, hit_off filled, not one hit written
        if pinned:
            keep = [PinnedArray(n + 1, np.uint64), PinnedArray(total, HIT_DTYPE)]
            hoff, hits = keep[0].array, keep[1].array
        else:
            hoff, hits = np.zeros(n + 1, np.uint64), np.zeros(total, HIT_DTYPE)
        hits.view(np.uint8)[:] = 0xAB
        canary = hits.copy()
        assert lib.rawdtw_seed_begin(eng._ctx, n, vp(off), vp(ev), vp(hoff), vp(hits), total - 1) == 0
        assert lib.rawdtw_seed_end(eng._ctx, None) == RANGE
        assert np.array_equal(hoff, want_off) and np.array_equal(hits, canary), pinned
        assert lib.rawdtw_seed_begin(eng._ctx, n, vp(off), vp(ev), vp(hoff), vp(hits), total) == 0   # exactly enough
        assert lib.rawdtw_seed_end(eng._ctx, None) == 0
        same_hits(hits[:total], want, "exact cap")
    with pytest.raises(RawDTWError) as ei:
        eng.seed_hits(ev, off, hits_cap=7)
    assert ei.value.status == RANGE and np.array_equal(ei.value.hit_off, want_off)
    # a second begin is refused and the first seeding stays right
    hoff, hits = np.zeros(n + 1, np.uint64), np.zeros(total, HIT_DTYPE)
    hoff2, hits2 = np.zeros(n + 1, np.uint64), np.zeros(total, HIT_DTYPE)
    assert lib.rawdtw_seed_end(eng._ctx, None) == INVALID   # nothing begun
    assert lib.rawdtw_seed_begin(eng._ctx, n, vp(off), vp(ev), vp(hoff), vp(hits), total) == 0
    assert lib.rawdtw_seed_begin(eng._ctx, n, vp(off), vp(ev), vp(hoff2), vp(hits2), total) == INVALID
    assert lib.rawdtw_seed_index_upload(eng._ctx, six._h) == INVALID   # (nor is the table replaced under a seeding)
    assert lib.rawdtw_seed_end(eng._ctx, None) == 0
    assert np.array_equal(hoff, want_off) and not hoff2.any() and not hits2.view(np.uint8).any()
    same_hits(hits, want, "first seeding")
    # refusals of begin, nothing enqueued: null arguments, offsets that descend
    bad = off.copy()
    bad[5] = bad[4] - 1
    assert lib.rawdtw_seed_begin(eng._ctx, n, vp(bad), vp(ev), vp(hoff2), vp(hits2), total) == INVALID
    assert lib.rawdtw_seed_begin(eng._ctx, n, None, vp(ev), vp(hoff2), vp(hits2), total) == INVALID
    assert lib.rawdtw_seed_begin(eng._ctx, n, vp(off), None, vp(hoff2), vp(hits2), total) == INVALID
    assert lib.rawdtw_seed_begin(eng._ctx, n, vp(off), vp(ev), None, vp(hits2), total) == INVALID
    assert lib.rawdtw_seed_begin(eng._ctx, n, vp(off), vp(ev), vp(hoff2), None, total) == INVALID
    assert lib.rawdtw_seed_end(eng._ctx, None) == INVALID   # (none of them began anything)
    assert not hoff2.any()
    # w > 0 is the host's; a context without a table seeds nothing
    e2 = ra.Engine(0)
    try:
        assert lib.rawdtw_seed_begin(e2._ctx, n, vp(off), vp(ev), vp(hoff2), vp(hits2), total) == INVALID
        assert b"rawdtw_seed_index_upload" in lib.rawdtw_last_error(e2._ctx)
        e2.upload_seed_index(SeedIndex.from_signals(ref.forward, ref.reverse, SeedParams(w=5)))
        assert lib.rawdtw_seed_begin(e2._ctx, n, vp(off), vp(ev), vp(hoff2), vp(hits2), total) == UNSUPPORTED
        assert lib.rawdtw_seed_end(e2._ctx, None) == INVALID and not hoff2.any() and not hits2.view(np.uint8).any()
        e2.upload_seed_index(six)   # an upload replaces the table
        assert lib.rawdtw_seed_begin(e2._ctx, n, vp(off), vp(ev), vp(hoff2), vp(hits2), total) == 0
        assert lib.rawdtw_seed_end(e2._ctx, None) == 0
        same_hits(hits2, want, "after a second upload")
    finally:
        e2.close()


# ---- 5. beside other work on the same context ------------------------------------------------------------------------------------------
def test_detection_seeding_and_a_batch_on_one_context_change_nothing_of_each_other(six, ref):
    lib = ra.load_library()
    e = ra.Engine(0)
    try:
        e.upload_seed_index(six)
        e.upload_reference(ref.forward, ref.reverse)
        offs = {(s, st): e.reference_offset(s, st) for s in range(ref.n_seq) for st in (0, 1)}
        cb, _ = synth.make_candidate_batch(ref, offs, synth.SynthParams(n_reads=128, max_chunks=2), seed=52)
        e.upload_events(cb.events)
        co = ra.MapOpt().c_struct()
        vp = lambda a: np.ascontiguousarray(a).ctypes.data  # noqa: E731
        arrs = [np.ascontiguousarray(x) for x in (cb.chain_off, cb.anchor_off, cb.anchors, cb.ref_base, cb.read_base)]
        raws = synth.make_raw_reads(256, 4000, seed=53)
        sig, soff = np.concatenate(raws), np.arange(257, dtype=np.uint64) * 4000
        fx = mc.Fixture()

        def run(beside):
            h = C.c_void_p()
            assert lib.rawdtw_batch_submit(e._ctx, C.byref(co), cb.n_reads, *[vp(a) for a in arrs], C.byref(h)) == 0
            det = e.detect_events(sig, soff) if beside else None
            sd = e.seed_hits(fx.events, fx.ev_off) if beside else None
            score, keep = np.zeros(cb.n_chains + 1, np.float32), np.zeros(cb.n_chains + 1, np.uint8)
            assert lib.rawdtw_batch_fetch_destroy(e._ctx, h, vp(score), vp(keep)) == 0
            return score[:cb.n_chains].copy(), keep[:cb.n_chains].copy(), det, sd

        s0, k0, _, _ = run(False)
        s1, k1, (eoff, ev), (hoff, hits) = run(True)
        assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)) and np.array_equal(k0, k1)
        want_off, want = ra.detect_events_host(sig, soff, threads=16)
        assert np.array_equal(eoff, want_off) and np.array_equal(ev.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(hoff.astype(np.int64), fx.hit_off)
        same_hits(hits, fx.hits, "beside a batch and a detection")
    finally:
        e.close()


# ---- 6. whole reads through the library alone ------------------------------------------------------------------------------------------
class _DetectedReads:
    """the raw reads of tests/golden/map_ref_reads.npz with the events the DEVICE detected for them, behind mapper.SyntheticSeeds'
    interface; the hits are left to rawdtw_mapper_round_seeded"""

    def __init__(self, wr, eng, form):
        self.wr, self.lens, self.n_reads = wr, wr.lens, wr.n_reads
        chunks = [c for sig in mc.make_raw_reads() for c in mc.raw_chunks(sig)]
        off = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint64)
        self.eoff, self.ev = eng.detect_events(np.concatenate(chunks), off, ra.EventOptions(contracted=bool(form)))[:2]

    def read_job(self, r):
        return self.wr.read_job(r)

    def chunk(self, r, c):
        ci = int(self.wr.chunk_first[r]) + c
        return self.ev[int(self.eoff[ci]):int(self.eoff[ci + 1])], []


@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("name", list(mc.WHOLE_SETS))
def test_whole_reads_detected_seeded_and_mapped_by_the_library(six, ref, name, form):
    """Raw pA chunks in, PAF lines out, every stage the library's: rawdtw_detect_begin, rawdtw_mapper_round_seeded (seeding on the
    device, then the unchanged round) and rawdtw_mapper_finish, against the record and tags the reference's map_worker_for left in
    the fixture -- with one group and two, chaining on the host and on the device.  (The fixture's raw reads are fp32 pA, which no
    int16 sample and channel reproduce bit for bit: they go in through the pA entry, rawdtw_detect_begin, not the int16 one.)"""
    wr = mc.WholeReads(form)
    want = [wr.expected_line(name, r) for r in range(wr.n_reads)]
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        seeds = _DetectedReads(wr, e, form)
        assert np.array_equal(seeds.ev.view(np.uint32), wr.events.view(np.uint32))
        opt, copt = mc.whole_project_opts(name, form)
        for dev, groups in ((True, 1), (True, 2), (False, 1), (False, 2)):
            cm = mapper.CMapper(e, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096,
                                max_reads=wr.n_reads, chain_opt=copt, output_chains=True, threads=3, groups=groups, carry=False, device_chain=dev)
            got, _ = mapper.map_reads_c(seeds, list(range(wr.n_reads)), cm, seed_index=six)
            cm.close()
            for r, (g, w) in enumerate(zip(got, want)):
                assert g == w, (name, form, dev, groups, r)
    finally:
        e.close()


# ---- 7. the int16 entry, seeding and mapping on one context ----------------------------------------------------------------------------
def test_int16_windows_detected_seeded_and_mapped_on_one_context():
    """Raw int16 windows in, PAF lines out, on ONE context: rawdtw_detect_raw_begin, then rawdtw_mapper_round_seeded (device
    seeding, device chaining) and finish -- against the host path fed the same windows (rawdtw_detect_raw_host,
    rawdtw_seed_hits_host) through the plain rawdtw_mapper_round on a context of its own: the same lines, round by round the
    same reads still active."""
    from rawalign_amd.rawsig import Channel, detect_events_raw_host

    n, n_chunks = 48, 3
    sref = synth.make_reference([REAL_BP], seed=REAL_SEED)
    si = SeedIndex.from_signals(sref.forward, sref.reverse, threads=8)
    rng = np.random.default_rng(REAL_SEED + 5)
    g = synth.make_genome(REAL_BP, REAL_SEED)
    pa = synth.make_genome_raw_reads(g, rng.integers(0, REAL_BP - 2200, n), [2000] * n, rng.integers(0, 2, n), seed=REAL_SEED + 6)
    chan = Channel(8192.0, 1450.0, 3.0)
    raws = [np.round(r[:4000 * n_chunks] * (chan.digitisation / chan.range) - chan.offset).astype(np.int16) for r in pa]
    assert all(len(r) == 4000 * n_chunks for r in raws)
    opt, stop = ra.MapOpt(), StopOpt()
    names, lens = ["synth_0"], [len(sref.forward[0])]
    ea, eb = ra.Engine(0), ra.Engine(0)
    try:
        for e in (ea, eb):
            e.upload_reference(sref.forward, sref.reverse)
        ca = mapper.CMapper(ea, opt, stop, names, lens, slot_events=4096, max_reads=n, threads=3, carry=False, device_chain=True)
        cb = mapper.CMapper(eb, opt, stop, names, lens, slot_events=4096, max_reads=n, threads=3, carry=False, device_chain=True)
        ids = [ca.add_read("read_%d" % r, 4000 * n_chunks, n_chunks) for r in range(n)]
        assert ids == [cb.add_read("read_%d" % r, 4000 * n_chunks, n_chunks) for r in range(n)]
        for c in range(n_chunks):
            act = [r for r in range(n) if not ca.state(ids[r])[0]]
            assert act == [r for r in range(n) if not cb.state(ids[r])[0]], c
            if not act:
                break
            raw = np.concatenate([raws[r][4000 * c:4000 * (c + 1)] for r in act])
            off = np.arange(len(act) + 1, dtype=np.uint64) * 4000
            _, eoff, ev = ea.detect_events_raw(raw, off, chan)
            ca.round([ids[r] for r in act], [(ev[int(eoff[k]):int(eoff[k + 1])], []) for k in range(len(act))], seed_index=si)
            _, hoff_e, hev = detect_events_raw_host(raw, off, chan, threads=8)
            assert np.array_equal(hoff_e, eoff) and np.array_equal(hev.view(np.uint32), ev.view(np.uint32))
            hoff, hits = seeding.seed_hits_host(si, hev, hoff_e, threads=8)
            rows = sc.hit_rows(hits).tolist()
            cb.round([ids[r] for r in act], [(hev[int(hoff_e[k]):int(hoff_e[k + 1])], [tuple(x) for x in rows[int(hoff[k]):int(hoff[k + 1])]])
                                             for k in range(len(act))])
        assert ca.finish() == 0 and cb.finish() == 0
        la, lb = [ca.paf(i) for i in ids], [cb.paf(i) for i in ids]
        assert la == lb
        assert sum("\t*\t" not in ln for ln in la) >= n // 2   # (they map: the test is not one of empty lines)
        ca.close()
        cb.close()
    finally:
        ea.close()
        eb.close()


# ---- 8. plain, resident and detected seedings in turn on one context ------------------------------------------------------------------
@pytest.mark.parametrize("w", [0, 5])
def test_the_three_seedings_share_one_workspace(ref, w):
    """The three begins (rawdtw_seed_begin, rawdtw_seed_resident_begin, rawdtw_seed_detected_begin) carve one grow-only workspace,
    each its own way; here they follow one another on one context, growing and re-using it, every seeding against
    rawdtw_seed_hits_host hit for hit -- and the rules between the kinds: a later seeding of any kind ends what an ended resident
    one left readable, a begin refused by its own argument checks does not."""
    from rawalign_amd.seeding import SeedParams

    lib = ra.load_library()
    si = SeedIndex.from_signals(ref.forward, ref.reverse, SeedParams(w=w), threads=4)
    wins = [np.ascontiguousarray(sig[i:i + 1000], np.float32) for sig in mc.make_raw_reads() for i in range(0, len(sig) - 999, 1000)][:65]
    evs = [ra.detect_events(x) for x in wins]   # (the host's detection: bit for bit what the device leaves in the arena)
    slot = 1024
    assert len(evs) == 65 and all(6 <= len(x) <= slot for x in evs)
    starts = np.arange(65, dtype=np.uint64) * slot
    vp = lambda a: a.ctypes.data  # noqa: E731

    def host(chunks):
        return seeding.seed_hits_host(si, *sc.flat(chunks), threads=8)

    def fetch_fails(rs):
        with pytest.raises(RawDTWError) as ei:
            rs.fetch()
        return ei.value.status

    e = ra.Engine(0)
    try:
        if w:
            e.set_option("seed_minimizer", 1)
        e.upload_seed_index(si)
        e.reserve_events(66 * slot)
        # 1. plain, one chunk
        off1, hits1 = host(evs[3:4])
        assert len(hits1) > 0
        got_off, got = e.seed_hits(*sc.flat(evs[3:4]))
        assert np.array_equal(got_off, off1)
        same_hits(got, hits1, "1 plain")
        # 2. resident, 65 chunks of which one is empty: both blocks grow
        chunks = list(evs)
        chunks[7] = chunks[7][:0]
        ev, off = sc.flat(chunks)
        e.append_events(ev, off, starts.astype(np.uint32))
        want_off, want = host(chunks)
        rs = e.seed_resident(starts, np.array([len(c) for c in chunks], np.uint32))
        assert np.array_equal(rs.hit_off, want_off) and len(want) > 65
        same_hits(rs.fetch(), want, "2 resident")
        # 3. detected, 64 windows behind a resident detection
        sig = np.concatenate(wins[:64])
        det = e.detect_resident(sig, np.arange(65, dtype=np.uint64) * 1000, starts[:64], np.full(64, slot, np.uint32), wait=False)
        sd = e.seed_detected(det, wait=False)
        ev_len, _, total = det.end()
        assert ev_len.tolist() == [len(x) for x in evs[:64]] and total == sum(len(x) for x in evs[:64])
        rs3 = sd.end()
        want_off, want = host(evs[:64])
        assert np.array_equal(rs3.hit_off, want_off)
        same_hits(rs3.fetch(), want, "3 detected")
        # 4. plain, three chunks without an event: nothing is enqueued, and step 3's hits are gone all the same
        got_off, got = e.seed_hits(np.zeros(0, np.float32), np.zeros(4, np.uint64))
        want_off, want = host([evs[0][:0]] * 3)
        assert got_off.tolist() == want_off.tolist() == [0, 0, 0, 0] and len(got) == len(want) == 0
        assert fetch_fails(rs3) == INVALID
        # 5. resident, one chunk: what the detection left in slot 3 of the arena
        rs5 = e.seed_resident(starts[3:4], np.array([len(evs[3])], np.uint32))
        assert np.array_equal(rs5.hit_off, off1)
        same_hits(rs5.fetch(), hits1, "5 resident")
        # two begins refused by their own argument checks leave it readable
        hoff = np.zeros(3, np.uint64)
        outside, some = np.array([70 * slot], np.uint64), np.array([8], np.uint32)
        assert lib.rawdtw_seed_resident_begin(e._ctx, 1, vp(outside), vp(some), vp(hoff)) == RANGE
        descending, few, room = np.array([0, 5, 3], np.uint64), np.zeros(8, np.float32), np.zeros(8, HIT_DTYPE)
        assert lib.rawdtw_seed_begin(e._ctx, 2, vp(descending), vp(few), vp(hoff), vp(room), 8) == INVALID
        assert not hoff.any()
        same_hits(rs5.fetch(), hits1, "5 after the refusals")
        same_hits(rs5.fetch(pinned=False), hits1, "5 after the refusals, pageable")
    finally:
        e.close()
