"""Event detection on the host (include/rawdtw.h: rawdtw_detect_events, rawdtw_detect_events_host): the library's restatement of
detect_events (src/revent.c:190-210) against the reference's own answers (tests/golden/detect_events_ref.npz, both builds),
against a plain-Python restatement, across thread counts, and its refusals.  No device needed."""
import math
import os

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd._lib import RawDTWError
from tests.events_cases import DEFAULT, EDGE_LENGTHS, OPTION_SETS, cases, events_sha256, inputs_sha256

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "detect_events_ref.npz"))


@pytest.fixture(scope="module")
def all_cases(fixture):
    cs = cases()
    assert inputs_sha256(cs) == str(fixture["inputs_sha256"]), "tests/events_cases.py no longer generates the fixture's inputs"
    assert [c[0] for c in cs] == list(fixture["names"])
    return cs


def opts(o, contracted):
    return ra.EventOptions(*o, contracted=contracted)


@pytest.mark.parametrize("form", ["plain", "contracted"])
def test_host_restatement_equals_reference(fixture, all_cases, form):
    bad = []
    for k, (name, sig, o) in enumerate(all_cases):
        ev = ra.detect_events(sig, opts(o, form == "contracted"))
        if len(ev) != fixture[f"n_events_{form}"][k] or events_sha256(ev) != bytes(fixture[f"sha256_{form}"][k]):
            bad.append((name, len(ev), int(fixture[f"n_events_{form}"][k])))
    assert not bad, bad[:10]
    # the two forms really are different computations on these inputs
    assert np.any(fixture["sha256_plain"] != fixture["sha256_contracted"])


def py_detect_events(sig, o):
    """revent.c:22-188, plain form, in np.float32 scalars and Python floats (the doubles)."""
    w1, w2, t1, t2, ph = int(o[0]), int(o[1]), F32(o[2]), F32(o[3]), F32(o[4])
    n = len(sig)
    ps, pss = [F32(0)] * (n + 1), [F32(0)] * (n + 1)
    for i in range(n):
        x = F32(sig[i])
        ps[i + 1] = ps[i] + x
        pss[i + 1] = pss[i] + x * x

    def tstat(w):
        t = [F32(0)] * (n + 1)
        if n < 2 * w or w < 2:
            return t
        wf = F32(w)
        for i in range(w, n - w + 1):
            s1, q1 = ps[i], pss[i]
            if i > w:
                s1 = s1 - ps[i - w]
                q1 = q1 - pss[i - w]
            s2, q2 = ps[i + w] - ps[i], pss[i + w] - pss[i]
            m1, m2 = s1 / wf, s2 / wf
            cv = q1 / wf - m1 * m1 + q2 / wf - m2 * m2
            cv = max(cv, F32(np.finfo(F32).tiny))
            t[i] = F32(abs(float(m2 - m1)) / math.sqrt(float(cv / wf)))
        return t

    sig_t = [tstat(w1), tstat(w2)]
    thr, wl = [t1, t2], [w1, w2]
    st = [dict(pv=F32(np.finfo(F32).max), pp=-1, mt=0, valid=False) for _ in range(2)]
    peaks = []
    for i in range(n):
        for k in range(2):
            d = st[k]
            if d["mt"] >= i:
                continue
            v = sig_t[k][i]
            if d["pp"] == -1:
                if v < d["pv"]:
                    d["pv"] = v
                elif v - d["pv"] > ph:
                    d["pv"], d["pp"] = v, i
            else:
                if v > d["pv"]:
                    d["pv"], d["pp"] = v, i
                if k == 0 and d["pv"] > thr[0]:
                    st[1].update(mt=d["pp"] + wl[0], pp=-1, pv=F32(np.finfo(F32).max), valid=False)
                if d["pv"] - v > ph and d["pv"] > thr[k]:
                    d["valid"] = True
                if d["valid"] and (i - d["pp"]) > wl[k] // 2:
                    peaks.append(d["pp"])
                    d["pp"], d["pv"], d["valid"] = -1, v, False
    if not peaks:
        return np.zeros(0, F32)
    n_ev = 1 + sum(1 for p in peaks[1:] if 0 < p < n)
    ev, s, s2 = [], 0.0, 0.0
    l_ps, l_peak = F32(0), F32(0)
    for pi in range(n_ev):
        end = peaks[pi] if pi < n_ev - 1 else n
        e = (ps[end] - l_ps) / (F32(end) - l_peak)
        ev.append(e)
        s += float(e)
        s2 += float(e * e)
        l_ps, l_peak = ps[end], F32(end)
    mean = s / n_ev
    var = s2 / n_ev - mean * mean
    with np.errstate(all="ignore"):  # (a one-event chunk: std 0, NaN)
        sd = np.sqrt(np.float64(var))
        return np.array([np.float64(float(e) - mean) / sd for e in ev], np.float64).astype(F32)


def assert_same_events(got, want, what):
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert len(got) == len(want), (what, len(got), len(want))
    g, w = got.view(np.uint32).copy(), want.view(np.uint32).copy()
    g[np.isnan(got)] = 0x7FC00000
    w[np.isnan(want)] = 0x7FC00000
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def test_python_restatement_equals_host_restatement():
    rng = np.random.default_rng(77)
    sets = [DEFAULT] + list(OPTION_SETS.values())
    lens = list(EDGE_LENGTHS) + [int(x) for x in rng.integers(26, 2000, 30)]
    from rawalign_amd.synth import make_raw_reads

    reads = make_raw_reads(len(lens), lens, seed=78)
    n_events = 0
    for k, sig in enumerate(reads):
        o = sets[k % len(sets)]
        want = py_detect_events(sig, o)
        got = ra.detect_events(sig, opts(o, False))
        assert_same_events(got, want, (k, len(sig), o))
        n_events += len(got)
    assert n_events > 1000


@pytest.mark.parametrize("contracted", [False, True])
def test_batch_equals_per_chunk_calls_on_any_thread_count(contracted):
    from rawalign_amd.synth import make_raw_reads

    rng = np.random.default_rng(5)
    lens = [4000] * 40 + [int(x) for x in rng.integers(1, 4000, 40)] + list(EDGE_LENGTHS) + [65536]
    reads = make_raw_reads(len(lens), lens, seed=6)
    reads[3] = np.full(4000, 90.0, F32)  # no events
    sig = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    o = ra.EventOptions(contracted=contracted)
    per = [ra.detect_events(s, o) for s in reads]
    want_off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.uint64)
    for threads in (1, 4, 16):
        eoff, ev = ra.detect_events_host(sig, off, o, threads=threads)
        assert np.array_equal(eoff, want_off), threads
        assert_same_events(ev, np.concatenate(per), threads)
    assert want_off[4] == want_off[3]
    # a first offset that is not 0: the chunks are where the offsets say
    eoff, ev = ra.detect_events_host(np.concatenate([np.zeros(7, F32), sig]), off + np.uint64(7), o, threads=4)
    assert np.array_equal(eoff, want_off)
    assert_same_events(ev, np.concatenate(per), "offset")


def test_refusals():
    lib = ra.load_library()
    import ctypes as C

    sig = np.ones(100, F32)
    out = np.zeros(100, F32)
    n = C.c_uint32(7)
    assert lib.rawdtw_detect_events(None, 0, sig.ctypes.data, out.ctypes.data, C.byref(n)) == 1  # s_len 0: revent.c:24
    with pytest.raises(RawDTWError) as e:
        ra.detect_events(sig, ra.EventOptions(window_length1=65536))
    assert e.value.status == 1
    with pytest.raises(RawDTWError) as e:
        ra.detect_events(sig, ra.EventOptions(window_length2=1 << 31))
    assert e.value.status == 1
    ra.detect_events(np.ones(10, F32), ra.EventOptions(window_length1=65535, window_length2=65535))  # the bound itself is allowed
    with pytest.raises(RawDTWError) as e:  # offsets that descend
        ra.detect_events_host(sig, np.array([0, 50, 40, 100], np.uint64))
    assert e.value.status == 1
    with pytest.raises(RawDTWError) as e:  # an empty chunk
        ra.detect_events_host(sig, np.array([0, 50, 50, 100], np.uint64))
    assert e.value.status == 1
    # events_cap too small: RAWDTW_ERR_RANGE, event_off still right
    from rawalign_amd.synth import make_raw_reads

    reads = make_raw_reads(3, 4000, seed=9)
    sig = np.concatenate(reads)
    off = np.array([0, 4000, 8000, 12000], np.uint64)
    want_off, want = ra.detect_events_host(sig, off)
    eoff = np.zeros(4, np.uint64)
    ev = np.full(16, -7.0, F32)
    st = lib.rawdtw_detect_events_host(None, 3, off.ctypes.data, sig.ctypes.data, eoff.ctypes.data, ev.ctypes.data, 16, 2)
    assert st == 4 and np.array_equal(eoff, want_off) and np.all(ev == -7.0)
    st = lib.rawdtw_detect_events_host(None, 3, off.ctypes.data, sig.ctypes.data, eoff.ctypes.data, None, int(want_off[-1]), 2)
    assert st == 1  # null events


def test_no_boundary_gives_no_events_and_peaks_stay_below_samples(all_cases):
    assert len(ra.detect_events(np.full(4000, 100.5, F32))) == 0
    assert len(ra.detect_events(np.ones(1, F32))) == 0
    worst = 0.0
    for name, sig, o in all_cases:
        for c in (False, True):
            ev = ra.detect_events(sig, opts(o, c))
            assert len(ev) <= max(len(sig) - 1, 0), name
            worst = max(worst, len(ev) / len(sig))
    assert worst <= 0.5, worst  # (peak_height 0 and thresholds 0 included)
