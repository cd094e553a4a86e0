"""Raw signal in, on the device (include/rawdtw.h: rawdtw_detect_raw_begin / rawdtw_detect_end; k_raw_count and k_raw_compact in
rawdtw_events.hip) against the host restatement rawdtw_detect_raw_host, bit for bit (s_len, event_off, events; any NaN equals
any NaN), and against the float entry on host-converted chunks -- which tests/test_events_gpu.py ties to the reference's own
answers.  The vector loads' heads and tails, empty and all-outlier windows, degenerate channels, both forms, page-locked and
pageable results, the shared workspace, the refusals, and a raw detection while a DTW batch is in flight."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd.rawsig import CHANNEL_DTYPE, channels
from rawalign_amd.synth import make_dac_reads, make_raw_reads
from tests.test_events_host import assert_same_events
from tests.test_rawsig_host import DEGENERATE, expect_from_old_path, host_converted, np_to_pa, raw_batch

F32 = np.float32
FORMS = [False, True]
RATES = [0.0, 0.001, 0.3]


@pytest.fixture(scope="module")
def eng():
    e = ra.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def realistic():
    """{rate: (raws, chan)}: 4 096 windows of about 4 000 samples, a channel of its own a read"""
    rng = np.random.default_rng(50)
    lens = [int(x) for x in rng.integers(3900, 4101, 4096)]
    return {rate: make_dac_reads(4096, lens, seed=51 + i, outlier_rate=rate) for i, rate in enumerate(RATES)}


def n_dropped(raws, chan):
    return sum(int((~np_to_pa(r, c)[1]).sum()) for r, c in zip(raws, chan))


def check_against_host(eng, raws, chan, opt, what, lead=0, **kw):
    """the batch through the device and through rawdtw_detect_raw_host; `lead` samples in front of the first window"""
    raw, off = raw_batch(raws)
    if lead:
        raw, off = np.concatenate([np.full(lead, 77, np.int16), raw]), off + np.uint64(lead)
    chan = channels(chan, len(raws))
    want_len, want_off, want = ra.detect_events_raw_host(raw, off, chan, opt, threads=16)
    s_len, eoff, ev = eng.detect_events_raw(raw, off, chan, opt, **kw)
    assert np.array_equal(s_len, want_len), what
    assert np.array_equal(eoff, want_off), what
    assert_same_events(ev, want, what)
    return s_len, eoff, ev


@pytest.mark.gpu
@pytest.mark.parametrize("contracted", FORMS)
@pytest.mark.parametrize("rate", RATES)
def test_device_equals_host_on_realistic_windows(eng, realistic, rate, contracted):
    raws, chan = realistic[rate]
    dropped = n_dropped(raws, chan)
    assert (dropped == 0) if rate == 0 else (dropped > 0.5 * rate * 4096 * 4000)
    s_len, eoff, _ = check_against_host(eng, raws, chan, ra.EventOptions(contracted=contracted), (rate, contracted))
    assert int(s_len.sum()) == sum(len(r) for r in raws) - dropped
    assert eoff[-1] > 4096 * 200


@pytest.mark.gpu
@pytest.mark.parametrize("contracted", FORMS)
def test_two_entry_points_agree(eng, realistic, contracted):
    """the same batch through the OLD path: to_pa on the host, then Engine.detect_events"""
    opt = ra.EventOptions(contracted=contracted)
    for rate in RATES:
        raws, chan = realistic[rate]
        raws, chan = raws[:1024], chan[:1024]
        raw, off = raw_batch(raws)
        s_len, eoff, ev = eng.detect_events_raw(raw, off, chan, opt)
        lens, sig, sig_off = host_converted(raws, chan)
        assert np.all(lens > 0) and np.array_equal(s_len, lens)
        old_off, old = eng.detect_events(sig, sig_off, opt)
        assert np.array_equal(eoff, old_off), rate
        assert_same_events(ev, old, rate)


def edge_lengths():
    lens = list(range(1, 71))
    for m in range(8, 513, 8):  # every multiple of 8 (and so of 64) up to 512, one either side
        lens += [m - 1, m, m + 1]
    return lens


@pytest.mark.gpu
@pytest.mark.parametrize("contracted", FORMS)
def test_heads_and_tails_of_the_vector_loads(eng, contracted):
    opt = ra.EventOptions(contracted=contracted)
    lens = edge_lengths()
    rng = np.random.default_rng(60)
    for lead, rate in ((0, 0.0), (1, 0.05), (4, 0.3), (7, 0.05)):
        order = [lens[i] for i in rng.permutation(len(lens))]
        raws, chan = make_dac_reads(len(order), order, seed=61 + lead, outlier_rate=rate)
        starts = lead + np.concatenate([[0], np.cumsum(order)[:-1]])
        assert set(starts % 8) == set(range(8))  # odd and even 2-byte positions, every place in a 16-byte group
        assert (n_dropped(raws, chan) > 0) == (rate > 0)
        s_len, eoff, _ = check_against_host(eng, raws, chan, opt, (lead, rate), lead=lead)
        assert eoff[-1] > 1000
    # each length at an odd and at an even start, explicitly: the batch twice, the second copy an odd distance behind the first
    raws, chan = make_dac_reads(len(lens), lens, seed=70, outlier_rate=0.02)
    sep = np.full(1 if sum(lens) % 2 == 0 else 2, 500, np.int16)
    twice = raws + [sep] + raws
    ch2 = np.concatenate([chan, chan[:1], chan])
    starts = np.concatenate([[0], np.cumsum([len(r) for r in twice])[:-1]])
    half = len(raws)
    assert all((starts[k] + starts[half + 1 + k]) % 2 == 1 for k in range(half))
    check_against_host(eng, twice, ch2, opt, "both parities")


@pytest.mark.gpu
@pytest.mark.parametrize("contracted", FORMS)
def test_empty_all_outlier_long_and_degenerate_windows(eng, contracted):
    opt = ra.EventOptions(contracted=contracted)
    raws, chan = make_dac_reads(200, 4000, seed=80, outlier_rate=0.001)
    chan = chan.copy()
    for k in (0, 17, 18, 100, 199):
        raws[k] = np.zeros(0, np.int16)              # empty, the batch's first and last among them
    for k in (5, 50, 51):
        raws[k] = np.full(4000, -30000, np.int16)    # all outliers
    raws[60] = np.full(1, 32000, np.int16)
    s_len, eoff, _ = check_against_host(eng, raws, chan, opt, "empty and all-outlier")
    for k in (0, 17, 18, 100, 199, 5, 50, 51, 60):
        assert s_len[k] == 0 and eoff[k + 1] == eoff[k]
    assert eoff[-1] > 190 * 300
    # one 250 000-sample window among short ones
    long_raw, long_ch = make_dac_reads(1, 250000, seed=81, outlier_rate=0.001)
    mixed = raws[:100] + long_raw + raws[100:]
    s_len, eoff, _ = check_against_host(eng, mixed, np.concatenate([chan[:100], long_ch, chan[100:]]), opt, "long")
    assert 240000 < s_len[100] < 250000 and eoff[101] - eoff[100] > 20000
    # the degenerate channels: IEEE arithmetic decides, the same on both sides
    rng = np.random.default_rng(82)
    for j, d in enumerate(DEGENERATE):
        ch, base = chan.copy(), list(raws)
        for k in range(10 + j, 200, len(DEGENERATE)):  # a tenth of the batch on this channel
            ch[k] = d
            base[k] = rng.integers(-1200, 1200, 4000).astype(np.int16)
        s_len, _, _ = check_against_host(eng, base, ch, opt, d)
        want = [len(np_to_pa(r, c)[0]) for r, c in zip(base, ch)]
        assert list(s_len) == want, d
    # nothing but empty windows, and no window at all
    s_len, eoff, ev = eng.detect_events_raw(np.zeros(9, np.int16), np.full(6, 4, np.uint64), chan[:5], opt)
    assert not s_len.any() and not eoff.any() and len(ev) == 0
    s_len, eoff, ev = eng.detect_events_raw(np.zeros(0, np.int16), np.zeros(1, np.uint64), np.zeros(0, CHANNEL_DTYPE), opt)
    assert len(s_len) == 0 and list(eoff) == [0] and len(ev) == 0


@pytest.mark.gpu
def test_page_locked_and_pageable_results_are_identical(eng):
    rng = np.random.default_rng(4)
    raws, chan = make_dac_reads(300, [int(x) for x in rng.integers(1, 4000, 300)], seed=90, outlier_rate=0.01)
    raw, off = raw_batch(raws)
    a_len, a_off, a, ms = eng.detect_events_raw(raw, off, chan, pinned=True, kernel_ms=True)
    b_len, b_off, b, ms2 = eng.detect_events_raw(raw, off, chan, pinned=False, kernel_ms=True)
    assert np.array_equal(a_len, b_len) and np.array_equal(a_off, b_off)
    assert_same_events(a, b, "pinned vs pageable")
    assert ms > 0 and ms2 > 0
    lib = ra.load_library()
    for name in ("raw", "slen", "eoff", "ev"):
        assert lib.rawdtw_host_is_page_locked(C.c_void_p(eng._raw_stage[name].ptr)) == 1
    check_against_host(eng, raws, chan, None, "pageable", pinned=False)
    # events_cap: one short is RAWDTW_ERR_RANGE with event_off and s_len filled; exactly enough passes
    want_len, want_off, _ = ra.detect_events_raw_host(raw, off, chan)
    for pinned in (False, True):
        with pytest.raises(ra.RawDTWError) as e:
            eng.detect_events_raw(raw, off, chan, pinned=pinned, events_cap=int(want_off[-1]) - 1)
        assert e.value.status == 4
        assert np.array_equal(e.value.event_off, want_off) and np.array_equal(e.value.s_len, want_len)
        got = eng.detect_events_raw(raw, off, chan, pinned=pinned, events_cap=int(want_off[-1]))
        assert np.array_equal(got[1], want_off)


@pytest.mark.gpu
def test_float_and_raw_detections_share_the_workspace(eng):
    raws, chan = make_dac_reads(500, 4000, seed=91, outlier_rate=0.01)
    reads = make_raw_reads(700, 3000, seed=92)
    sig = np.concatenate(reads)
    sig_off = (np.arange(701) * 3000).astype(np.uint64)
    want_off, want = ra.detect_events_host(sig, sig_off, threads=16)
    for _ in range(2):  # raw, float, raw, float: each after the other kind
        check_against_host(eng, raws, chan, None, "raw after float")
        got_off, got = eng.detect_events(sig, sig_off)
        assert np.array_equal(got_off, want_off)
        assert_same_events(got, want, "float after raw")
    fresh = ra.Engine(0)  # a float detection first on a context, then a larger raw one (the workspace grows)
    try:
        got_off, got = fresh.detect_events(sig[:30000], sig_off[:11])
        assert np.array_equal(got_off, want_off[:11])
        check_against_host(fresh, raws, chan, None, "raw after a smaller float")
    finally:
        fresh.close()


@pytest.mark.gpu
def test_second_begin_of_either_kind_is_refused_and_refusals_enqueue_nothing(eng):
    lib = ra.load_library()
    raws, chan = make_dac_reads(64, 4000, seed=93, outlier_rate=0.01)
    raw, off = raw_batch(raws)
    N = int(off[-1])
    want_len, want_off, want = ra.detect_events_raw_host(raw, off, chan, threads=8)
    sig = np.concatenate(make_raw_reads(64, 4000, seed=94))
    sig_off = (np.arange(65) * 4000).astype(np.uint64)
    fwant_off, fwant = ra.detect_events_host(sig, sig_off, threads=8)
    vp = lambda a: a.ctypes.data  # noqa: E731
    new = lambda: (np.zeros(64, np.uint32), np.zeros(65, np.uint64), np.zeros(N, F32))  # noqa: E731
    ctx = eng._ctx
    raw_begin = lambda o, n, ro, r, ch, sl, eo, ev, cap: lib.rawdtw_detect_raw_begin(  # noqa: E731
        ctx, o, n, None if ro is None else vp(ro), None if r is None else vp(r), None if ch is None else vp(ch),
        None if sl is None else vp(sl), None if eo is None else vp(eo), None if ev is None else vp(ev), cap)
    assert lib.rawdtw_detect_end(ctx, None) == 1  # nothing begun
    # a raw detection pending: a second begin of either kind is refused, the first stays right
    sl, eo, ev = new()
    sl2, eo2, ev2 = new()
    assert raw_begin(None, 64, off, raw, chan, sl, eo, ev, N) == 0
    assert raw_begin(None, 64, off, raw, chan, sl2, eo2, ev2, N) == 1
    assert b"not ended" in lib.rawdtw_last_error(ctx)
    assert lib.rawdtw_detect_begin(ctx, None, 64, vp(sig_off), vp(sig), vp(eo2), vp(ev2), N) == 1
    assert lib.rawdtw_detect_end(ctx, None) == 0
    assert np.array_equal(sl, want_len) and np.array_equal(eo, want_off) and not eo2.any() and not sl2.any()
    assert_same_events(ev[:int(eo[-1])], want, "first raw detection")
    # a float detection pending: a raw begin is refused
    feo, fev = np.zeros(65, np.uint64), np.zeros(N, F32)
    assert lib.rawdtw_detect_begin(ctx, None, 64, vp(sig_off), vp(sig), vp(feo), vp(fev), N) == 0
    assert raw_begin(None, 64, off, raw, chan, sl2, eo2, ev2, N) == 1
    assert lib.rawdtw_detect_end(ctx, None) == 0
    assert np.array_equal(feo, fwant_off) and not eo2.any()
    assert_same_events(fev[:int(feo[-1])], fwant, "first float detection")
    # the refusals, each RAWDTW_ERR_INVALID with a worded error and nothing for rawdtw_detect_end to end
    bad = off.copy()
    bad[5] = bad[4] - 1
    huge = off.copy()
    huge[64:] += np.uint64(1 << 32)
    wide = ra.EventOptions(window_length2=70000).c()
    refused = [
        ("null", (None, 64, None, raw, chan, sl2, eo2, ev2, N)), ("null", (None, 64, off, None, chan, sl2, eo2, ev2, N)),
        ("null", (None, 64, off, raw, None, sl2, eo2, ev2, N)), ("null", (None, 64, off, raw, chan, None, eo2, ev2, N)),
        ("null", (None, 64, off, raw, chan, sl2, None, ev2, N)), ("null", (None, 64, off, raw, chan, sl2, eo2, None, N)),
        ("descend", (None, 64, bad, raw, chan, sl2, eo2, ev2, N)), ("2^32", (None, 64, huge, raw, chan, sl2, eo2, ev2, N)),
        ("65535", (C.byref(wide), 64, off, raw, chan, sl2, eo2, ev2, N)),
    ]
    for word, args in refused:
        assert raw_begin(*args) == 1, word
        assert word.encode() in lib.rawdtw_last_error(ctx), (word, lib.rawdtw_last_error(ctx))
        assert lib.rawdtw_detect_end(ctx, None) == 1, word
    assert lib.rawdtw_detect_raw_begin(None, None, 64, vp(off), vp(raw), vp(chan), vp(sl2), vp(eo2), vp(ev2), N) == 1  # no context
    assert not eo2.any() and not sl2.any() and not ev2.any()
    # an empty window is NOT refused here (the float entry refuses it)
    emp = off.copy()
    emp[5] = emp[4]
    assert raw_begin(None, 64, emp, raw, chan, sl2, eo2, ev2, N) == 0
    assert lib.rawdtw_detect_end(ctx, None) == 0
    assert sl2[4] == 0 and sl2[5] > 7000 and eo2[5] == eo2[4]
    # and the context still works
    check_against_host(eng, raws, chan, None, "after the refusals")


@pytest.mark.gpu
def test_raw_detection_between_batch_submit_and_fetch_changes_neither(eng):
    from rawalign_amd import synth

    lib = ra.load_library()
    sref = synth.make_reference([60_000], seed=41)
    eng.upload_reference(sref.forward, sref.reverse)
    offs = {(0, st): eng.reference_offset(0, st) for st in (0, 1)}
    cb, _ = synth.make_candidate_batch(sref, offs, synth.SynthParams(n_reads=256, max_chunks=3), seed=42)
    eng.upload_events(cb.events)
    co = ra.MapOpt().c_struct()
    vp = lambda a: np.ascontiguousarray(a).ctypes.data  # noqa: E731
    arrs = [np.ascontiguousarray(x) for x in (cb.chain_off, cb.anchor_off, cb.anchors, cb.ref_base, cb.read_base)]
    raws, chan = make_dac_reads(512, 4000, seed=43, outlier_rate=0.01)
    raw, off = raw_batch(raws)

    def run(with_detection):
        h = C.c_void_p()
        assert lib.rawdtw_batch_submit(eng._ctx, C.byref(co), cb.n_reads, *[vp(a) for a in arrs], C.byref(h)) == 0
        det = eng.detect_events_raw(raw, off, chan) if with_detection else None
        score, keep = np.zeros(cb.n_chains + 1, F32), np.zeros(cb.n_chains + 1, np.uint8)
        assert lib.rawdtw_batch_fetch_destroy(eng._ctx, h, vp(score), vp(keep)) == 0
        return score[:cb.n_chains].copy(), keep[:cb.n_chains].copy(), det

    s0, k0, _ = run(False)
    s1, k1, (s_len, eoff, ev) = run(True)
    assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)) and np.array_equal(k0, k1)
    want_len, want_off, want = ra.detect_events_raw_host(raw, off, chan, threads=16)
    assert np.array_equal(s_len, want_len) and np.array_equal(eoff, want_off)
    assert_same_events(ev, want, "beside a batch")
    # and the host-side old path agrees with both
    old_len, old_off, old = expect_from_old_path(raws, chan, None)
    assert np.array_equal(s_len, old_len) and np.array_equal(eoff, old_off)
    assert_same_events(ev, old, "old path")
