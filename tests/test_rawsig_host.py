"""Raw signal in, on the host (include/rawdtw.h: rawdtw_signal_to_pa, rawdtw_signal_chunk_table, rawdtw_detect_raw_host): the
library's restatement of ri_read_sig's pA conversion and outlier filter (src/rsig.cpp:216-224) against a numpy restatement of
the same lines, bit for bit on every int16 value; the chunk table against chunks_of on the filtered read (src/rmap.cpp:685-690);
the raw detection against detect_events_host on host-converted chunks.  No device needed."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd.rawsig import CHANNEL_DTYPE, channels, count_kept
from rawalign_amd.synth import make_dac_reads
from tests.test_events_host import assert_same_events

F32 = np.float32
ALL_INT16 = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)

# (digitisation, range, offset)
CHANNELS = [
    (8192.0, 1467.61, 6.0), (8192.0, 1402.882, -9.0), (8192.0, 1499.9, 0.0), (2048.0, 748.5801, -237.0), (8192.0, 1437.976, 13.0),
    (8192.0, 8192.0, 0.0),      # scale 1: 30 and 200 pA fall exactly on raw 30 and 200
    (8192.0, 4096.0, 0.0),      # scale 0.5: on raw 60 and 400
    (8192.0, 8192.0, 0.5),      # the add rounds (raw + 0.5 is exact here; the bounds fall between values)
    (8192.0, -1450.0, -900.0),  # a negative scale
    (0.0, 1450.0, 3.0),         # digitisation 0: the scale is +inf
    (0.0, 0.0, 3.0),            # 0 / 0: NaN
    (8192.0, 1450.0, float("nan")),
    (8192.0, float("inf"), 0.0),
    (1e-30, 1450.0, 0.0),       # the scale overflows to +inf
    (8192.0, 1e-38, 0.0),       # a denormal scale
]
DEGENERATE = CHANNELS[5:]


def np_to_pa(raw, chan):
    """src/rsig.cpp:216-224 in numpy's float32 (IEEE, one rounding an operation).  Returns (kept pA in order, keep mask)."""
    dig, ran, offset = (F32(x) for x in chan)
    with np.errstate(all="ignore"):
        pa = (np.asarray(raw).astype(F32) + offset) * (ran / dig)
        keep = (pa > F32(30)) & (pa < F32(200))
    return pa[keep], keep


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


@pytest.mark.parametrize("chan", CHANNELS, ids=[str(c) for c in CHANNELS])
def test_to_pa_equals_the_restatement_on_every_int16_value(chan):
    want, keep = np_to_pa(ALL_INT16, chan)
    got = ra.to_pa(ALL_INT16, chan)
    assert len(got) == len(want) == int(keep.sum())
    assert np.array_equal(bits(got), bits(want))
    assert count_kept(ALL_INT16, chan) == len(want)  # pa == NULL
    # one value at a time too: nothing depends on the neighbours
    rng = np.random.default_rng(1)
    for r in rng.integers(-32768, 32768, 50):
        one = np.array([r], np.int16)
        assert np.array_equal(bits(ra.to_pa(one, chan)), bits(np_to_pa(one, chan)[0]))


def test_the_bounds_are_exclusive_and_the_degenerate_channels_do_what_ieee_says():
    keep = np_to_pa(ALL_INT16, (8192.0, 8192.0, 0.0))[1]
    assert np.array_equal(ALL_INT16[keep], np.arange(31, 200))  # 30 and 200 are dropped, 31 and 199 kept
    assert np.array_equal(ra.to_pa(ALL_INT16, (8192.0, 8192.0, 0.0)), np.arange(31, 200).astype(F32))
    assert len(ra.to_pa(ALL_INT16, (8192.0, -1450.0, -900.0))) > 500  # a negative scale keeps the values below the offset
    for chan in [(0.0, 1450.0, 3.0), (0.0, 0.0, 3.0), (8192.0, 1450.0, float("nan")), (8192.0, float("inf"), 0.0)]:
        assert len(ra.to_pa(ALL_INT16, chan)) == 0, chan  # infinities and NaN are dropped
    assert len(ra.to_pa(ALL_INT16, CHANNELS[0])) > 900


def test_make_dac_reads_plants_what_it_says():
    for rate in (0.0, 0.001, 0.3):
        raws, chan = make_dac_reads(40, 4000, seed=5, outlier_rate=rate)
        assert chan.dtype == CHANNEL_DTYPE and all(r.dtype == np.int16 for r in raws)
        assert np.all(chan["digitisation"] == 8192) and np.all((chan["range"] >= 1400) & (chan["range"] <= 1500))
        assert np.all(chan["offset"] == np.rint(chan["offset"])) and np.any(chan["offset"] < 0) and np.any(chan["offset"] > 0)
        dropped = sum(int((~np_to_pa(r, c)[1]).sum()) for r, c in zip(raws, chan))
        if rate == 0.0:
            assert dropped == 0
        else:
            assert 0.5 * rate * 160000 < dropped < 1.5 * rate * 160000 + 40
        if rate == 0.3:  # both sides
            pa = (raws[0].astype(F32) + chan[0]["offset"]) * (chan[0]["range"] / chan[0]["digitisation"])
            assert np.any(pa <= 30) and np.any(pa >= 200)


CS, MAXC = 500, 6


def read_with_l_sig(l_sig, rate, seed, tail_outliers=0):
    """a read whose filtered length is exactly l_sig: outliers at `rate` in between, then tail_outliers raw outliers.  Returns
    (raw, channel, the outliers this function added itself)"""
    raws, chan = make_dac_reads(1, max(int(l_sig / (1 - rate) * 1.2) + 64, 64), seed=seed, outlier_rate=rate)
    raw, ch = raws[0], chan[0]
    keep = np_to_pa(raw, ch)[1]
    assert keep.sum() >= l_sig
    cut = 0 if l_sig == 0 else int(np.nonzero(keep)[0][l_sig - 1]) + 1
    raw = raw[:cut]
    own = tail_outliers
    if l_sig == 0 and rate > 0:
        raw, own = np.full(37, -32000, np.int16), own + 37  # nothing but outliers
    if tail_outliers:
        raw = np.concatenate([raw, np.full(tail_outliers, 32000, np.int16)])
    return raw, ch, own


@pytest.mark.parametrize("rate", [0.0, 0.001, 0.3])
def test_chunk_table_windows_hold_exactly_the_chunks_of_the_filtered_read(rate):
    lens = [0, 1, CS - 1, CS, CS + 1, 3 * CS, 2 * CS + 17, MAXC * CS, MAXC * CS + 1, (MAXC + 3) * CS + 250]
    n_dropped = 0
    for k, l_sig in enumerate(lens):
        for tail in (0, CS):  # (CS: the read's last chunk_size raw samples are all outliers)
            raw, ch, own = read_with_l_sig(l_sig, rate, seed=100 + k, tail_outliers=tail)
            want, keep = np_to_pa(raw, ch)
            n_dropped += int((~keep).sum()) - own  # (the generator's)
            assert len(want) == l_sig
            got_l, start = ra.chunk_table(raw, ch, CS, MAXC)
            off = ra.chunks_of(want, CS, MAXC)
            assert got_l == l_sig, (l_sig, tail)
            assert len(start) == len(off), (l_sig, tail, start, off)
            assert len(start) - 1 == min(MAXC, -(-l_sig // CS))
            for c in range(len(start) - 1):
                a, b = int(start[c]), int(start[c + 1])
                assert keep[a], "a window starts on a kept sample"
                assert keep[b - 1] or c + 2 < len(start), "the last one ends behind a kept sample"
                win = np_to_pa(raw[a:b], ch)[0]
                assert np.array_equal(bits(win), bits(want[int(off[c]):int(off[c + 1])])), (l_sig, tail, c)
            if l_sig == 0:
                assert list(start) == [0]
    # a long read at the default cut, across the table pass's own block edges
    raws, chan = make_dac_reads(1, 200_000, seed=7, outlier_rate=rate)
    want, keep = np_to_pa(raws[0], chan[0])
    n_dropped += int((~keep).sum())
    got_l, start = ra.chunk_table(raws[0], chan[0])
    off = ra.chunks_of(want)
    assert got_l == len(want) > 30 * 4000 and len(start) == len(off) == 31
    for c in range(30):
        assert keep[int(start[c])]
        assert np.array_equal(bits(np_to_pa(raws[0][int(start[c]):int(start[c + 1])], chan[0])[0]), bits(want[int(off[c]):int(off[c + 1])]))
    assert (n_dropped == 0) if rate == 0 else (n_dropped > 100)


def test_chunk_table_on_degenerate_channels_and_refusals():
    lib = ra.load_library()
    rng = np.random.default_rng(3)
    raw = rng.integers(-2000, 2000, 5000).astype(np.int16)
    for chan in DEGENERATE:
        want, keep = np_to_pa(raw, chan)
        got_l, start = ra.chunk_table(raw, chan, 100, 7)
        assert got_l == len(want)
        off = ra.chunks_of(want, 100, 7)
        assert len(start) == len(off)
        for c in range(len(start) - 1):
            assert np.array_equal(bits(np_to_pa(raw[int(start[c]):int(start[c + 1])], chan)[0]), bits(want[int(off[c]):int(off[c + 1])]))
    ch = channels((8192.0, 1450.0, 0.0))
    l, n = C.c_uint64(), C.c_uint32()
    start = np.zeros(8, np.uint64)
    assert lib.rawdtw_signal_chunk_table(ch.ctypes.data, len(raw), raw.ctypes.data, 0, 7, C.byref(l), C.byref(n), start.ctypes.data) == 1
    assert lib.rawdtw_signal_chunk_table(None, len(raw), raw.ctypes.data, 100, 7, C.byref(l), C.byref(n), start.ctypes.data) == 1
    assert lib.rawdtw_signal_to_pa(ch.ctypes.data, len(raw), None, None, C.byref(l)) == 1
    assert lib.rawdtw_signal_chunk_table(ch.ctypes.data, len(raw), raw.ctypes.data, 100, 0, C.byref(l), C.byref(n), start.ctypes.data) == 0
    assert n.value == 0 and l.value == len(np_to_pa(raw, (8192.0, 1450.0, 0.0))[0])


def raw_batch(raws):
    off = np.concatenate([[0], np.cumsum([len(r) for r in raws])]).astype(np.uint64)
    return (np.concatenate(raws) if len(raws) else np.zeros(0, np.int16)).astype(np.int16), off


def host_converted(raws, chan):
    """the old path's input: every window converted by to_pa; windows that keep nothing leave the batch"""
    sigs = [ra.to_pa(r, c) for r, c in zip(raws, chan)]
    lens = np.array([len(s) for s in sigs], np.uint32)
    full = [s for s in sigs if len(s)]
    off = np.concatenate([[0], np.cumsum([len(s) for s in full])]).astype(np.uint64)
    return lens, (np.concatenate(full) if full else np.zeros(0, F32)), off


def expect_from_old_path(raws, chan, opt):
    """(s_len, event_off, events) as detect_events_host gives them on the host-converted chunks"""
    lens, sig, off = host_converted(raws, chan)
    eoff_full, ev = ra.detect_events_host(sig, off, opt, threads=8) if len(off) > 1 else (np.zeros(1, np.uint64), np.zeros(0, F32))
    counts = np.zeros(len(raws), np.uint64)
    counts[lens > 0] = np.diff(eoff_full)
    return lens, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), ev


@pytest.mark.parametrize("contracted", [False, True])
@pytest.mark.parametrize("threads", [1, 8])
def test_detect_raw_host_equals_detect_events_host_on_host_converted_chunks(contracted, threads):
    opt = ra.EventOptions(contracted=contracted)
    rng = np.random.default_rng(11)
    for rate in (0.0, 0.001, 0.3):
        lens = [4000] * 12 + [int(x) for x in rng.integers(1, 4000, 12)]
        raws, chan = make_dac_reads(len(lens), lens, seed=int(rate * 1000) + 20, outlier_rate=rate)
        raws[5] = np.zeros(0, np.int16)                # an empty window
        raws[9] = np.full(3000, 30000, np.int16)       # an all-outlier window
        raw, off = raw_batch(raws)
        dropped = sum(int((~np_to_pa(r, c)[1]).sum()) for r, c in zip(raws, chan)) - 3000
        assert (dropped == 0) if rate == 0 else (dropped > 10)
        want_len, want_off, want = expect_from_old_path(raws, chan, opt)
        s_len, eoff, ev = ra.detect_events_raw_host(raw, off, chan, opt, threads=threads)
        assert np.array_equal(s_len, want_len) and np.array_equal(eoff, want_off)
        assert_same_events(ev, want, (rate, threads))
        assert s_len[5] == 0 and s_len[9] == 0 and eoff[6] == eoff[5] and eoff[10] == eoff[9]
        assert eoff[-1] > 1000
        # a first offset that is not 0
        s2, e2, v2 = ra.detect_events_raw_host(np.concatenate([np.zeros(5, np.int16), raw]), off + np.uint64(5), chan, opt, threads=threads)
        assert np.array_equal(s2, want_len) and np.array_equal(e2, want_off)
        assert_same_events(v2, want, "offset")


def test_detect_raw_host_refusals_and_events_cap():
    lib = ra.load_library()
    raws, chan = make_dac_reads(3, 4000, seed=9, outlier_rate=0.001)
    raw, off = raw_batch(raws)
    s_len, want_off, want = ra.detect_events_raw_host(raw, off, chan)
    tot = int(want_off[-1])
    sl, eoff, ev = np.zeros(3, np.uint32), np.zeros(4, np.uint64), np.full(tot, -7.0, F32)
    args = lambda cap: (None, 3, off.ctypes.data, raw.ctypes.data, chan.ctypes.data, sl.ctypes.data, eoff.ctypes.data,  # noqa: E731
                        ev.ctypes.data, cap, 2)
    assert lib.rawdtw_detect_raw_host(*args(tot - 1)) == 4  # RAWDTW_ERR_RANGE, event_off filled, no event written
    assert np.array_equal(eoff, want_off) and np.array_equal(sl, s_len) and np.all(ev == -7.0)
    assert lib.rawdtw_detect_raw_host(*args(tot)) == 0
    assert_same_events(ev, want, "exactly enough")
    with pytest.raises(ra.RawDTWError) as e:
        ra.detect_events_raw_host(raw, off, chan, events_cap=tot - 1)
    assert e.value.status == 4 and np.array_equal(e.value.event_off, want_off)
    bad = off.copy()
    bad[2] = bad[1] - 1
    with pytest.raises(ra.RawDTWError) as e:  # offsets that descend
        ra.detect_events_raw_host(raw, bad, chan)
    assert e.value.status == 1
    with pytest.raises(ra.RawDTWError) as e:
        ra.detect_events_raw_host(raw, off, chan, ra.EventOptions(window_length1=65536))
    assert e.value.status == 1
    assert lib.rawdtw_detect_raw_host(None, 3, off.ctypes.data, raw.ctypes.data, None, sl.ctypes.data, eoff.ctypes.data, ev.ctypes.data, tot, 2) == 1
    # no window at all
    s0, e0, v0 = ra.detect_events_raw_host(np.zeros(0, np.int16), np.zeros(1, np.uint64), np.zeros(0, CHANNEL_DTYPE))
    assert len(s0) == 0 and list(e0) == [0] and len(v0) == 0
