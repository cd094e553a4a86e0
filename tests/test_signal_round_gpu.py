"""Chunk rounds from raw signal with the events left on the device (include/rawdtw.h: rawdtw_detect_resident_begin /
rawdtw_detect_raw_resident_begin / rawdtw_detect_resident_end, rawdtw_seed_detected_begin, rawdtw_mapper_round_signal_resident /
rawdtw_mapper_round_raw_resident) against the host restatements, the reference's recorded lines and the parent's path
(rawdtw_detect_raw_begin + rawdtw_mapper_round_seeded_resident): integers and float bits compared exactly (any NaN equals any NaN).
Nothing here reads the reference itself."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapper, seeding, synth
from rawalign_amd.mapping import StopOpt
from rawalign_amd.rawsig import CHANNEL_DTYPE, Channel, detect_events_raw_host
from rawalign_amd.seeding import HIT_DTYPE, SeedIndex, SeedParams
from rawalign_amd.synth import make_dac_reads
from tests import map_ref_cases as mc
from tests.test_rawsig_host import expect_from_old_path, raw_batch

pytestmark = pytest.mark.gpu
INVALID, RANGE, UNSUPPORTED = 1, 4, 5
SENTINEL = 0x5EA7BEEF   # the arena's fill: no event has these bits (3.4e18 is no normalised event)
QNAN = 0x7FC00000
KINDS = ["raw", "pa"]
LONG = 120   # the 250 000-sample window's place: behind the 0 / 1 / 64 / 65-chunk prefixes


def vp(a):
    return C.c_void_p(a.ctypes.data)


def canon(x):
    """float bits with every NaN made one NaN"""
    x = np.ascontiguousarray(x, np.float32)
    b = x.view(np.uint32).copy()
    b[np.isnan(x)] = QNAN
    return b


# ---- the windows of tests 1 and 2 -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def windows():
    """about 200 int16 windows: lengths 1 .. 4 000 at outlier rates 0 and 0.02, an empty, an all-outlier and a constant window, and
    one of 250 000 samples (more than 2 048 events: k_ev_events sums them from global memory)"""
    rng = np.random.default_rng(8)
    lens = [1, 2, 3, 5, 6, 7, 11, 12, 13, 63, 64, 65, 4000, 3999] + [int(x) for x in rng.integers(1, 4001, 182)]
    half = len(lens) // 2
    r0, c0 = make_dac_reads(half, lens[:half], seed=101, outlier_rate=0.0)
    r1, c1 = make_dac_reads(len(lens) - half, lens[half:], seed=102, outlier_rate=0.02)
    raws, chan = [], []
    for k in range(half):   # (the two rates interleaved)
        raws += [r0[k], r1[k]]
        chan += [c0[k], c1[k]]
    chan = np.array(chan, CHANNEL_DTYPE)
    raws[9] = np.zeros(0, np.int16)                 # empty
    raws[30] = np.full(4000, -30000, np.int16)      # all outliers
    raws[31], chan[31] = np.full(4000, 88, np.int16), (8192.0, 8192.0, 0.0)   # constant, and exactly 88 pA (every fp32 sum is exact): no peak, no events
    long_raw, long_ch = make_dac_reads(1, 250000, seed=103, outlier_rate=0.001)
    raws[LONG], chan[LONG] = long_raw[0], long_ch[0]
    return raws, chan


@pytest.fixture(scope="module")
def host(windows):
    """{contracted: (s_len, event_off, events)} of rawdtw_detect_raw_host, computed once -- and, for the pA input, the windows converted
    on the host (an all-outlier window becomes an empty one) with rawdtw_detect_events_host's answer on them, which must be the same"""
    raws, chan = windows
    raw, off = raw_batch(raws)
    out = {}
    for contracted in (False, True):
        opt = ra.EventOptions(contracted=contracted)
        s_len, eoff, ev = detect_events_raw_host(raw, off, chan, opt, threads=16)
        o_len, o_off, o_ev = expect_from_old_path(raws, chan, opt)
        assert np.array_equal(s_len, o_len) and np.array_equal(eoff, o_off) and np.array_equal(canon(ev), canon(o_ev))
        out[contracted] = (np.asarray(s_len).copy(), np.asarray(eoff).copy(), ev)
    pa = [ra.to_pa(r, c) for r, c in zip(raws, chan)]
    cnt = np.diff(out[False][1].astype(np.int64))
    assert np.diff(out[True][1].astype(np.int64))[31] == 0
    assert cnt[9] == 0 and cnt[30] == 0 and cnt[31] == 0 and cnt[LONG] > 2048 and len(pa[30]) == 0 and len(pa[31]) == 4000
    out["pa"] = pa
    return out


class Arena:
    """a torch tensor filled with the sentinel, set as the engine's event arena"""

    def __init__(self, eng, n):
        import torch

        self.t = torch.full((max(int(n), 4),), SENTINEL, dtype=torch.int32, device="cuda:0")
        eng.set_events_device(self.t.data_ptr(), self.t.numel(), keepalive=self.t)

    def bits(self):
        import torch

        torch.cuda.synchronize()
        return self.t.cpu().numpy().view(np.uint32)


def layout(counts, seed):
    """dst_start scattered in a permuted order at odd offsets; room exactly the count for every third chunk, larger elsewhere"""
    n = len(counts)
    rng = np.random.default_rng(seed)
    room = np.array([c if k % 3 == 0 else c + 1 + k % 5 for k, c in enumerate(counts)], np.uint32)
    dst = np.zeros(n, np.uint64)
    pos = 1
    for k in rng.permutation(n):
        dst[k] = pos
        pos += int(room[k]) + 1
        pos += 1 - pos % 2   # (the next start is odd)
    return dst, room, pos + 7


def inputs(kind, windows, host, n=None):
    raws, chan = windows
    n = len(raws) if n is None else n
    if kind == "raw":
        data, off = raw_batch(raws[:n])
        return data, off, chan[:n]
    pa = host["pa"][:n]
    off = np.concatenate([[0], np.cumsum([len(x) for x in pa])]).astype(np.uint64)
    return (np.concatenate(pa) if n else np.zeros(0, np.float32)).astype(np.float32), off, None


def expected_arena(size, dst, eoff, ev):
    want = np.full(size, SENTINEL, np.uint32)
    bits = canon(ev)
    for k in range(len(dst)):
        a, b = int(eoff[k]), int(eoff[k + 1])
        want[int(dst[k]):int(dst[k]) + b - a] = bits[a:b]
    return want


def arena_bits(ar):
    b = ar.bits().copy()
    f = b.view(np.float32)
    b[np.isnan(f)] = QNAN
    return b


# ---- 1. placement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("contracted", [False, True])
def test_events_land_at_their_places_and_nowhere_else(windows, host, kind, contracted):
    s_len, eoff, ev = host[contracted]
    opt = ra.EventOptions(contracted=contracted)
    eng = ra.Engine(0)
    try:
        for n in (len(windows[0]), 0, 1, 64, 65):
            counts = np.diff(eoff[:n + 1].astype(np.int64))
            dst, room, size = layout(counts, seed=n)
            assert n < 3 or (len(set(int(d) % 2 for d in dst)) == 1 and int(dst[0]) % 2 == 1 and not np.array_equal(np.argsort(dst), np.arange(n)))
            ar = Arena(eng, size)
            data, off, ch = inputs(kind, windows, host, n)
            ev_len, got_len, total = eng.detect_resident(data, off, dst, room, chan=ch, opt=opt)
            assert np.array_equal(ev_len, counts) and total == int(eoff[n]), (n, kind)
            assert np.array_equal(got_len, s_len[:n]), (n, kind)
            want = expected_arena(size, dst, eoff[:n + 1], ev)
            got = arena_bits(ar)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (n, kind, contracted, bad[:8], got[bad[:8]], want[bad[:8]])
    finally:
        eng.close()


# ---- 2. all or nothing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_round_that_does_not_fit_writes_nothing(windows, host, kind):
    s_len, eoff, ev = host[False]
    n = len(windows[0])
    counts = np.diff(eoff.astype(np.int64))
    dst, room, size = layout(counts, seed=7)
    data, off, ch = inputs(kind, windows, host)
    untouched = np.full(size, SENTINEL, np.uint32)
    eng = ra.Engine(0)
    try:
        ar = Arena(eng, size)
        mid = n // 2 - (n // 2) % 3   # (a chunk whose room is exactly its count)
        assert counts[mid] > 0 and room[mid] == counts[mid]
        short = room.copy()
        short[mid] -= 1
        with pytest.raises(ra.RawDTWError) as e:
            eng.detect_resident(data, off, dst, short, chan=ch)
        assert e.value.status == RANGE and "room" in str(e.value)
        assert np.array_equal(e.value.ev_len, counts) and e.value.total == int(eoff[-1])
        assert np.array_equal(ar.bits(), untouched)
        with pytest.raises(ra.RawDTWError) as e:
            eng.detect_resident(data, off, dst, room, chan=ch, events_cap=int(eoff[-1]) - 1)
        assert e.value.status == RANGE and "events_cap" in str(e.value)
        assert np.array_equal(e.value.ev_len, counts) and e.value.total == int(eoff[-1])
        assert np.array_equal(ar.bits(), untouched)
        ev_len, got_len, total = eng.detect_resident(data, off, dst, room, chan=ch, events_cap=int(eoff[-1]))
        assert np.array_equal(ev_len, counts) and np.array_equal(got_len, s_len) and total == int(eoff[-1])
        assert np.array_equal(arena_bits(ar), expected_arena(size, dst, eoff, ev))
    finally:
        eng.close()


def test_begin_refusals_enqueue_nothing(windows, host):
    s_len, eoff, ev = host[False]
    n = 65
    counts = np.diff(eoff[:n + 1].astype(np.int64))
    dst, room, size = layout(counts, seed=3)
    raw, off, ch = inputs("raw", windows, host, n)
    sig, soff, _ = inputs("pa", windows, host, n)
    lib = ra.load_library()
    eng, bare = ra.Engine(0), ra.Engine(0)
    try:
        # no arena on the context
        for call in (lambda: bare.detect_resident(raw, off, dst, room, chan=ch), lambda: bare.detect_resident(sig, soff, dst, room)):
            with pytest.raises(ra.RawDTWError) as e:
                call()
            assert e.value.status == INVALID and "arena" in str(e.value)
        ar = Arena(eng, size)
        # null arguments
        c = eng._ctx
        assert lib.rawdtw_detect_raw_resident_begin(c, None, n, vp(off), vp(raw), vp(ch), None, vp(room), 1 << 20) == INVALID
        assert lib.rawdtw_detect_raw_resident_begin(c, None, n, vp(off), vp(raw), vp(ch), vp(dst), None, 1 << 20) == INVALID
        assert lib.rawdtw_detect_raw_resident_begin(c, None, n, vp(off), vp(raw), None, vp(dst), vp(room), 1 << 20) == INVALID
        assert lib.rawdtw_detect_raw_resident_begin(c, None, n, None, vp(raw), vp(ch), vp(dst), vp(room), 1 << 20) == INVALID
        assert lib.rawdtw_detect_resident_begin(c, None, n, vp(soff), None, vp(dst), vp(room), 1 << 20) == INVALID
        assert lib.rawdtw_detect_resident_begin(c, None, n, vp(soff), vp(sig), None, vp(room), 1 << 20) == INVALID
        # a stretch beyond the arena
        far = dst.copy()
        far[n - 1] = size - int(room[n - 1]) + 1
        for call in (lambda: eng.detect_resident(raw, off, far, room, chan=ch), lambda: eng.detect_resident(sig, soff, far, room)):
            with pytest.raises(ra.RawDTWError) as e:
                call()
            assert e.value.status == RANGE and "beyond" in str(e.value)
        # nothing is begun: neither end has anything to end
        tot = C.c_uint64()
        evl = np.zeros(n, np.uint32)
        assert lib.rawdtw_detect_resident_end(c, None, vp(evl), C.byref(tot), None) == INVALID
        assert lib.rawdtw_detect_end(c, None) == INVALID
        # a detection begun: a second begin of any of the four kinds is refused, and the plain end does not end it
        det = eng.detect_resident(raw, off, dst, room, chan=ch, wait=False)
        for call in (lambda: eng.detect_resident(raw, off, dst, room, chan=ch), lambda: eng.detect_resident(sig, soff, dst, room),
                     lambda: eng.detect_events_raw(raw, off, ch), lambda: eng.detect_events(sig[:int(soff[1])], soff[:2])):
            with pytest.raises(ra.RawDTWError) as e:
                call()
            assert e.value.status == INVALID and "begun" in str(e.value)
        assert lib.rawdtw_detect_end(c, None) == INVALID
        assert lib.rawdtw_detect_resident_end(c, None, vp(evl), None, None) == INVALID   # (a null total: refused, still begun)
        ev_len, got_len, total = det.end()
        assert np.array_equal(ev_len, counts) and np.array_equal(got_len, s_len[:n]) and total == int(eoff[n])
        assert np.array_equal(arena_bits(ar), expected_arena(size, dst, eoff[:n + 1], ev))
        # and a plain detection begun is not ended by the resident end
        assert lib.rawdtw_detect_resident_end(c, None, vp(evl), C.byref(tot), None) == INVALID
        got = eng.detect_events_raw(raw, off, ch)
        assert np.array_equal(got[1], eoff[:n + 1]) and np.array_equal(canon(got[2]), canon(ev[:int(eoff[n])]))
    finally:
        eng.close()
        bare.close()


def test_the_four_detections_share_one_workspace(windows, host):
    """Float and raw, plain and resident, one after another on one context: every kind follows one of the other family (a plain end reads
    what a resident begin laid out before it, and the reverse), the blocks grow after a smaller detection, and n crosses the 64-chunk
    wave both ways.  Each against the host's answer, bit for bit."""
    s_len, eoff, ev = host[False]
    every = len(windows[0])
    eng = ra.Engine(0)

    def plain(kind, n):
        if kind == "raw":
            data, off, ch = inputs(kind, windows, host, n)
            got_len, got_off, got = eng.detect_events_raw(data, off, ch)
            assert np.array_equal(got_len, s_len[:n]) and np.array_equal(got_off, eoff[:n + 1]), (kind, n)
            assert np.array_equal(canon(got), canon(ev[:int(eoff[n])])), (kind, n)
            return
        keep = [k for k in range(n) if len(host["pa"][k])]   # (the plain float entry refuses an empty chunk)
        assert len(keep) == n - sum(1 for k in (9, 30) if k < n)
        pa = [host["pa"][k] for k in keep]
        off = np.concatenate([[0], np.cumsum([len(x) for x in pa])]).astype(np.uint64)
        want = [ev[int(eoff[k]):int(eoff[k + 1])] for k in keep]
        got_off, got = eng.detect_events(np.concatenate(pa), off)
        assert np.array_equal(got_off, np.concatenate([[0], np.cumsum([len(x) for x in want])]).astype(np.uint64)), (kind, n)
        assert np.array_equal(canon(got), canon(np.concatenate(want))), (kind, n)

    def resident(kind, n):
        counts = np.diff(eoff[:n + 1].astype(np.int64))
        dst, room, size = layout(counts, seed=40 + n)
        ar = Arena(eng, size)
        data, off, ch = inputs(kind, windows, host, n)
        ev_len, got_len, total = eng.detect_resident(data, off, dst, room, chan=ch)
        assert np.array_equal(ev_len, counts) and np.array_equal(got_len, s_len[:n]) and total == int(eoff[n]), (kind, n)
        got, want = arena_bits(ar), expected_arena(size, dst, eoff[:n + 1], ev)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (kind, n, bad[:8], got[bad[:8]], want[bad[:8]])

    try:
        plain("pa", 65)
        resident("raw", 1)
        plain("raw", 64)
        resident("pa", every)
        plain("pa", 1)
        resident("raw", every)
    finally:
        eng.close()


# ---- 3. seeding behind the detection ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref():
    return mc.make_reference()


@pytest.fixture(scope="module")
def seed_windows():
    """pA windows of 1 000 samples cut from the fixtures' raw reads (they seed: the reads come from the reference's genomes), with a
    constant window (0 events) and a 30-sample one (fewer than e = 6 events) to put at a batch's ends"""
    wins = [np.ascontiguousarray(sig[i:i + 1000], np.float32) for sig in mc.make_raw_reads() for i in range(0, len(sig) - 999, 1000)]
    assert len(wins) >= 70
    none, few = np.full(1000, 88.0, np.float32), wins[0][:30].copy()
    assert len(ra.detect_events(none)) == 0 and 0 < len(ra.detect_events(few)) < 6
    return wins, none, few


def host_seeding(si, wins, opt=None):
    evs = [ra.detect_events(w, opt) if len(w) else np.zeros(0, np.float32) for w in wins]
    eoff = np.concatenate([[0], np.cumsum([len(e) for e in evs])]).astype(np.uint64)
    ev = np.concatenate(evs + [np.zeros(0, np.float32)]).astype(np.float32)
    hoff, hits = seeding.seed_hits_host(si, ev, eoff, threads=8)
    return np.diff(eoff.astype(np.int64)), ev, hoff, hits


def same_hits(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in HIT_DTYPE.names:
        assert np.array_equal(got[f], want[f]), (what, f)


def detect_and_seed(eng, wins, slot=1024, events_cap=None, order="detect first"):
    sig = np.concatenate(list(wins) + [np.zeros(0, np.float32)]).astype(np.float32)
    off = np.concatenate([[0], np.cumsum([len(w) for w in wins])]).astype(np.uint64)
    dst, room = np.arange(len(wins), dtype=np.uint64) * slot, np.full(len(wins), slot, np.uint32)
    det = eng.detect_resident(sig, off, dst, room, events_cap=events_cap, wait=False)
    sd = eng.seed_detected(det, wait=False)
    if order == "detect first":
        got = det.end()
        return got, sd.end(), dst
    rs = sd.end()
    return det.end(), rs, dst


@pytest.mark.parametrize("w", [0, 5])
def test_seeding_enqueued_behind_the_detection_equals_the_host(ref, seed_windows, w):
    wins, none, few = seed_windows
    si = SeedIndex.from_signals(ref.forward, ref.reverse, SeedParams(w=w), threads=4)
    eng = ra.Engine(0)
    try:
        if w:
            eng.set_option("seed_minimizer", 1)
        eng.upload_seed_index(si)
        eng.reserve_events(66 * 1024)
        batches = [("1", [wins[3]]), ("64", [none] + wins[:62] + [few]), ("65", [few] + wins[5:68] + [none]), ("no samples", [wins[0][:0]] * 3)]
        for i, (what, batch) in enumerate(batches):
            counts, ev, hoff, hits = host_seeding(si, batch)
            assert what in ("1", "no samples") or (counts[0] in (0, 2) and 0 <= counts[-1] < 6 and len(hits) > len(batch))
            (ev_len, _, total), rs, dst = detect_and_seed(eng, batch, order="detect first" if i % 2 == 0 else "seed first")
            assert np.array_equal(ev_len, counts) and total == len(ev), what
            assert np.array_equal(rs.hit_off, hoff), what
            same_hits(rs.fetch(pinned=True), hits, what)
            same_hits(rs.fetch(pinned=False), hits, what)
        # a declined detection: the seeding's launches did nothing, its end says so
        batch = batches[1][1]
        counts, ev, hoff, hits = host_seeding(si, batch)
        sig = np.concatenate(batch).astype(np.float32)
        off = np.concatenate([[0], np.cumsum([len(x) for x in batch])]).astype(np.uint64)
        dst, room = np.arange(len(batch), dtype=np.uint64) * 1024, np.full(len(batch), 1024, np.uint32)
        det = eng.detect_resident(sig, off, dst, room, events_cap=len(ev) - 1, wait=False)
        sd = eng.seed_detected(det, wait=False)
        with pytest.raises(ra.RawDTWError) as e:
            sd.end()
        assert e.value.status == RANGE and "declined" in str(e.value)
        with pytest.raises(ra.RawDTWError) as e:
            det.end()
        assert e.value.status == RANGE and e.value.total == len(ev) and np.array_equal(e.value.ev_len, counts)
        with pytest.raises(ra.RawDTWError) as e:   # (nothing of it can be fetched)
            ra.dtw.ResidentSeeding(eng, hoff, 0.0).fetch()
        assert e.value.status == INVALID
        # behind it: a resident detection + seeding, and an ordinary resident seeding of the events that detection left in the arena
        (ev_len, _, total), rs, dst = detect_and_seed(eng, batch)
        assert np.array_equal(ev_len, counts) and np.array_equal(rs.hit_off, hoff)
        same_hits(rs.fetch(), hits, "after a declined one")
        rs = eng.seed_resident(dst, ev_len)
        assert np.array_equal(rs.hit_off, hoff)
        same_hits(rs.fetch(), hits, "ordinary resident seeding")
        # without a resident detection begun there is nothing to seed behind
        with pytest.raises(ra.RawDTWError) as e:
            eng.seed_detected(ra.dtw.ResidentDetection(eng, len(batch), None))
        assert e.value.status == INVALID
    finally:
        eng.close()


# ---- 4. the reference's own lines ---------------------------------------------------------------------------------------------------------
class _Signal:
    """the fixtures' pA reads cut with mc.raw_chunks, behind the interface map_reads_c(..., signal=True) asks for"""

    channels = None

    def __init__(self, wr, raws):
        self.wr, self.chunks = wr, [mc.raw_chunks(sig) for sig in raws]
        assert [len(c) for c in self.chunks] == [wr.n_chunks(r) for r in range(wr.n_reads)]

    def read_job(self, r):
        return self.wr.read_job(r)

    def window(self, r, c):
        return self.chunks[r][c]


@pytest.fixture(scope="module")
def six(ref):
    return SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)


@pytest.fixture(scope="module")
def raw_reads():
    raws = mc.make_raw_reads()
    assert mc.raw_sha256(raws) == np.load(mc.READS)["raw_sha256"].tobytes(), "synth.make_genome_raw_reads or tests/map_ref_cases.py drifted"
    return raws


def _whole_mapper(e, wr, opt, copt):
    return mapper.CMapper(e, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096,
                          max_reads=wr.n_reads, chain_opt=copt, output_chains=True, threads=3, carry=False, groups=1, device_chain=True)


@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("name", ["default", "noeval", "global_full", "frac025"])
def test_signal_in_gives_the_references_lines(ref, six, raw_reads, name, form):
    """The mapper is handed nothing but the reads' pA samples, chunk by chunk: every line is the one the reference's map_worker_for left
    in the fixture, and no event crossed PCIe."""
    wr = mc.WholeReads(form, ref=ref)
    want = [wr.expected_line(name, r) for r in range(wr.n_reads)]
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        opt, copt = mc.whole_project_opts(name, form)
        cm = _whole_mapper(e, wr, opt, copt)
        got, rounds = mapper.map_reads_c(_Signal(wr, raw_reads), list(range(wr.n_reads)), cm, seed_index=six, signal=True,
                                         event_opt=ra.EventOptions(contracted=bool(form)))
        st, rs, tm = cm.signal_stats(), cm.resident_stats(), cm.timing()
        cm.close()
        print(name, form, rounds, st, rs)
        for r, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, form, r)
        assert st["event_bytes_crossed"] == 0 and tm["event_bytes"] == 0
        assert st["rounds"] == rounds and st["sample_bytes_to_device"] > 0
        assert rs["resident_rounds"] + rs["fallback_rounds"] == rounds
    finally:
        e.close()


def test_a_cigar_mapper_is_refused_with_no_read_changed(ref, six, raw_reads):
    wr = mc.WholeReads(0, ref=ref)
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        opt, copt = mc.whole_project_opts("cigar", 0)
        cm = _whole_mapper(e, wr, opt, copt)
        src = _Signal(wr, raw_reads)
        ids = [cm.add_read("read_%d" % r, src.read_job(r).qlen, wr.n_chunks(r)) for r in range(wr.n_reads)]
        with pytest.raises(RuntimeError, match="status 5") as err:
            cm.round_signal(ids, [src.window(r, 0) for r in range(wr.n_reads)], six)
        assert "rawdtw_detect_raw_begin" in str(err.value) and "rawdtw_mapper_round_seeded_resident" in str(err.value)
        assert all(cm.state(i) == (False, 0) for i in ids) and cm.stats()[0] == 0 and cm.signal_stats()["rounds"] == 0
        # ... and the same mapper still maps the reads through the parent's path, CIGAR included
        got, _ = mapper.map_reads_c(wr, list(range(wr.n_reads)), _Readded(cm, ids), seed_index=six, resident=True)
        assert got == [wr.expected_line("cigar", r) for r in range(wr.n_reads)]
        cm.close()
    finally:
        e.close()


class _Readded:
    """map_reads_c's view of a mapper whose reads were added already"""

    def __init__(self, cm, ids):
        self.cm, self.ids, self.sequence_until = cm, list(ids), cm.sequence_until

    def __getattr__(self, k):
        return getattr(self.cm, k)

    def add_read(self, name, qlen, n_chunks):
        return self.ids.pop(0)


# ---- 5. the int16 flow against the parent's path ------------------------------------------------------------------------------------------
FLOW_BP, FLOW_SEED, FLOW_READS, FLOW_CHUNKS = 300_000, 777, 24, 4


@pytest.fixture(scope="module")
def flow():
    sref = synth.make_reference([FLOW_BP], seed=FLOW_SEED)
    si = SeedIndex.from_signals(sref.forward, sref.reverse, threads=8)
    rng = np.random.default_rng(FLOW_SEED + 5)
    g = synth.make_genome(FLOW_BP, FLOW_SEED)
    n = FLOW_READS
    pa = synth.make_genome_raw_reads(g, rng.integers(0, FLOW_BP - 3000, n), [2800] * n, rng.integers(0, 2, n), seed=FLOW_SEED + 6)
    chan = Channel(8192.0, 1450.0, 3.0)
    raws = [np.round(r[:4000 * FLOW_CHUNKS] * (chan.digitisation / chan.range) - chan.offset).astype(np.int16) for r in pa]
    assert all(len(r) == 4000 * FLOW_CHUNKS for r in raws)

    to_dac = lambda x: np.round(x * (chan.digitisation / chan.range) - chan.offset).astype(np.int16)  # noqa: E731
    jrng = np.random.default_rng(FLOW_SEED + 7)
    junk = {(r, c): to_dac(90.0 + 12.0 * np.repeat(jrng.normal(0, 1, 500), 8) + jrng.normal(0, 1.2, 4000))
            for r in range(1, n, 2) for c in range(2 if r % 4 == 1 else 1)}

    def window(r, c):
        """read r's chunk c.  The even reads are drawn from the genome throughout (they map in the first round); the odd ones start with
        one chunk from nowhere, or two (r % 4 == 1), so that the later rounds still have reads"""
        if (r, c) in junk:
            return junk[(r, c)]
        if (r, c) == (3, 1):
            return raws[r][4000:4300]                      # about 30 events: below min_events, the read sits the round out
        if (r, c) == (5, 2):
            return raws[r][:0]                             # an empty window
        if (r, c) == (7, 1):
            return np.full(4000, -30000, np.int16)         # all outliers
        return raws[r][4000 * c:4000 * (c + 1)]

    # the host's event counts, read by round: what a slot must hold
    counts = np.zeros((n, FLOW_CHUNKS), np.int64)
    for c in range(FLOW_CHUNKS):
        raw, off = raw_batch([window(r, c) for r in range(n)])
        counts[:, c] = np.diff(detect_events_raw_host(raw, off, chan, threads=8)[1].astype(np.int64))
    assert 0 < counts[3, 1] < 50 and counts[5, 2] == 0 and counts[7, 1] == 0
    return sref, si, chan, window, counts


def run_flow(flow, slot_events=4096, cap_first_try=0, fail_round=None):
    """mapper A: the parent's path (rawdtw_detect_raw_begin + rawdtw_mapper_round_seeded_resident); mapper B: rawdtw_mapper_round_raw_resident.
    Per round the same active reads and states; returns (lines A, lines B, A's resident stats, B's, B's signal stats)."""
    sref, si, chan, window, counts = flow
    n = FLOW_READS
    names, lens = ["synth_0"], [len(sref.forward[0])]
    ea, eb = ra.Engine(0), ra.Engine(0)
    try:
        for e in (ea, eb):
            e.upload_reference(sref.forward, sref.reverse)
        if cap_first_try:
            eb.set_option("signal_events_cap", cap_first_try)
        ca, cb = (mapper.CMapper(e, ra.MapOpt(), StopOpt(), names, lens, slot_events=slot_events, max_reads=n, threads=3, carry=False, device_chain=True)
                  for e in (ea, eb))
        ids = [ca.add_read("read_%d" % r, 4000 * FLOW_CHUNKS, FLOW_CHUNKS) for r in range(n)]
        assert ids == [cb.add_read("read_%d" % r, 4000 * FLOW_CHUNKS, FLOW_CHUNKS) for r in range(n)]
        failed = False
        for c in range(FLOW_CHUNKS):
            sa, sb = [ca.state(i) for i in ids], [cb.state(i) for i in ids]
            assert sa == sb, c
            act = [r for r in range(n) if not sa[r][0]]
            if not act:
                break
            wins = [window(r, c) for r in act]
            raw, off = raw_batch(wins)
            if c == fail_round:
                assert any(counts[r, :c + 1].sum() > slot_events for r in act)
                lines = [cb.paf(i) for i in ids]
                _, eoff, ev = ea.detect_events_raw(raw, off, chan)
                with pytest.raises(RuntimeError, match="status 4"):
                    ca.round([ids[r] for r in act], [(ev[int(eoff[k]):int(eoff[k + 1])], []) for k in range(len(act))], seed_index=si, resident=True)
                with pytest.raises(RuntimeError, match="status 4.*outgrew its slot"):
                    cb.round_signal([ids[r] for r in act], wins, si, channels=chan)
                assert [cb.state(i) for i in ids] == sb and [cb.paf(i) for i in ids] == lines and cb.stats()[0] == c
                assert [cb.paf(i) for i in ids] == [ca.paf(i) for i in ids]
                failed = True
                break
            _, eoff, ev = ea.detect_events_raw(raw, off, chan)
            ca.round([ids[r] for r in act], [(ev[int(eoff[k]):int(eoff[k + 1])], []) for k in range(len(act))], seed_index=si, resident=True)
            cb.round_signal([ids[r] for r in act], wins, si, channels=chan)
        assert failed == (fail_round is not None)
        assert [ca.state(i) for i in ids] == [cb.state(i) for i in ids]
        assert ca.finish() == 0 and cb.finish() == 0
        out = ([ca.paf(i) for i in ids], [cb.paf(i) for i in ids], ca.resident_stats(), cb.resident_stats(), cb.signal_stats())
        ca.close()
        cb.close()
        return out
    finally:
        ea.close()
        eb.close()


def test_int16_rounds_from_signal_equal_the_parents_path(flow):
    la, lb, ra_st, rb_st, sg = run_flow(flow)
    print(ra_st, rb_st, sg)
    assert la == lb and ra_st == rb_st
    assert sum("\t*\t" not in ln for ln in la) >= FLOW_READS // 2   # (they map: the test is not one of empty lines)
    assert sg["event_bytes_crossed"] == 0 and sg["retried_rounds"] == 0
    assert sg["rounds"] == rb_st["resident_rounds"] + rb_st["fallback_rounds"] and sg["rounds"] >= 2
    assert sg["sample_bytes_to_device"] > 0 and sg["sample_bytes_to_device"] % 2 == 0


def test_a_round_from_signal_that_falls_back_fetches_hits_not_events(flow, monkeypatch):
    monkeypatch.setenv("RAWDTW_CHAIN_MAX_SEEDS", "60")
    la, lb, ra_st, rb_st, sg = run_flow(flow)
    print(ra_st, rb_st, sg)
    assert rb_st["fallback_rounds"] > 0 and rb_st["hit_bytes_to_host"] > 0
    assert la == lb and ra_st == rb_st
    assert sg["event_bytes_crossed"] == 0


def test_a_first_try_whose_cap_is_too_small_runs_the_round_twice(flow):
    la, lb, ra_st, rb_st, sg = run_flow(flow, cap_first_try=1)
    print(ra_st, rb_st, sg)
    assert sg["retried_rounds"] > 0 and sg["retried_rounds"] <= sg["rounds"]
    assert la == lb and ra_st == rb_st and sg["event_bytes_crossed"] == 0


def test_a_slot_too_small_for_the_third_round_fails_it_and_changes_nothing(flow):
    counts = flow[4]
    slot = int(counts[:, :2].sum(axis=1).max()) + 10   # (two rounds fit every read; a third chunk of more than 10 events does not)
    la, lb, ra_st, rb_st, sg = run_flow(flow, slot_events=slot, fail_round=2)
    assert la == lb and sg["rounds"] == 2 and sg["event_bytes_crossed"] == 0
