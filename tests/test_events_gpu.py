"""Event detection on the device (include/rawdtw.h: rawdtw_detect_begin / rawdtw_detect_end, rawdtw_events.hip) against the
reference's own answers (tests/golden/detect_events_ref.npz) and against the host restatement, bit for bit (any NaN equals any
NaN), in the plain and the contracted form; page-locked and pageable results, the refusals, and a detection begun while a DTW
batch is in flight on the same context."""
import ctypes as C
import os

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd._lib import RawDTWError
from rawalign_amd.synth import make_raw_reads
from tests.events_cases import cases, events_sha256, inputs_sha256
from tests.test_events_host import assert_same_events

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FORMS = [False, True]


@pytest.fixture(scope="module")
def eng():
    e = ra.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "detect_events_ref.npz"))


@pytest.fixture(scope="module")
def groups(fixture):
    """the fixture's cases grouped by options: {options: [(index, name, signal)]}"""
    cs = cases()
    assert inputs_sha256(cs) == str(fixture["inputs_sha256"])
    g = {}
    for k, (name, sig, o) in enumerate(cs):
        g.setdefault(tuple(o), []).append((k, name, sig))
    return g


def batch(sigs):
    off = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.uint64)
    return np.concatenate(sigs).astype(F32), off


def check_against_host(eng, sigs, o, what):
    sig, off = batch(sigs)
    want_off, want = ra.detect_events_host(sig, off, o, threads=16)
    got_off, got = eng.detect_events(sig, off, o)
    assert np.array_equal(got_off, want_off), what
    assert_same_events(got, want, what)
    return got_off


@pytest.mark.gpu
@pytest.mark.parametrize("contracted", FORMS)
def test_device_equals_reference_fixture(eng, fixture, groups, contracted):
    form = "contracted" if contracted else "plain"
    bad, worst = [], 0.0
    for o, items in groups.items():
        sig, off = batch([s for _, _, s in items])
        eoff, ev = eng.detect_events(sig, off, ra.EventOptions(*o, contracted=contracted))
        for j, (k, name, s) in enumerate(items):
            e = ev[int(eoff[j]):int(eoff[j + 1])]
            if len(e) != fixture[f"n_events_{form}"][k] or events_sha256(e) != bytes(fixture[f"sha256_{form}"][k]):
                bad.append((name, len(e), int(fixture[f"n_events_{form}"][k])))
            assert len(e) <= len(s) - 1 or len(e) == 0, name  # never more events than peaks, nor peaks than s_len - 1
            worst = max(worst, len(e) / len(s))
    assert not bad, bad[:10]
    assert worst <= 0.5, worst  # (peak_height 0 and thresholds 0 included)


@pytest.mark.gpu
@pytest.mark.parametrize("contracted", FORMS)
def test_device_equals_host_on_realistic_edge_and_mixed_batches(eng, groups, contracted):
    reads = make_raw_reads(4096, 4000, seed=31)
    eoff = check_against_host(eng, reads, ra.EventOptions(contracted=contracted), "4096 chunks")
    assert eoff[-1] > 4096 * 300  # ~440 events a chunk
    for o, items in groups.items():  # the edge lengths and every option set
        check_against_host(eng, [s for _, _, s in items], ra.EventOptions(*o, contracted=contracted), o)
    # a batch mixing everything at the default options: realistic chunks, tails, edge lengths, a 250 000-sample read
    rng = np.random.default_rng(32)
    mixed = [s for items in groups.values() for _, _, s in items] + reads[:500]
    mixed = [mixed[i] for i in rng.permutation(len(mixed))]
    check_against_host(eng, mixed, ra.EventOptions(contracted=contracted), "mixed")
    long = make_raw_reads(1, 250000, seed=33)[0]
    check_against_host(eng, reads[:100] + [long] + reads[100:200], ra.EventOptions(contracted=contracted), "long")


@pytest.mark.gpu
def test_page_locked_and_pageable_results_are_identical(eng):
    reads = make_raw_reads(300, [int(x) for x in np.random.default_rng(4).integers(1, 4000, 300)], seed=34)
    sig, off = batch(reads)
    a_off, a, ms = eng.detect_events(sig, off, pinned=True, kernel_ms=True)
    b_off, b, ms2 = eng.detect_events(sig, off, pinned=False, kernel_ms=True)
    assert np.array_equal(a_off, b_off)
    assert_same_events(a, b, "pinned vs pageable")
    assert ms > 0 and ms2 > 0
    lib = ra.load_library()
    assert lib.rawdtw_host_is_page_locked(C.c_void_p(eng._ev_stage["ev"].ptr)) == 1


@pytest.mark.gpu
def test_second_begin_is_refused_and_first_detection_stays_right(eng):
    lib = ra.load_library()
    reads = make_raw_reads(64, 4000, seed=35)
    sig, off = batch(reads)
    want_off, want = ra.detect_events_host(sig, off, threads=8)
    eoff, ev = np.zeros(len(off), np.uint64), np.zeros(int(off[-1]), F32)
    eoff2, ev2 = np.zeros(len(off), np.uint64), np.zeros(int(off[-1]), F32)
    vp = lambda a: a.ctypes.data  # noqa: E731
    assert lib.rawdtw_detect_end(eng._ctx, None) == 1  # nothing begun
    assert lib.rawdtw_detect_begin(eng._ctx, None, 64, vp(off), vp(sig), vp(eoff), vp(ev), int(off[-1])) == 0
    assert lib.rawdtw_detect_begin(eng._ctx, None, 64, vp(off), vp(sig), vp(eoff2), vp(ev2), int(off[-1])) == 1
    ms = C.c_float()
    assert lib.rawdtw_detect_end(eng._ctx, C.byref(ms)) == 0
    assert np.array_equal(eoff, want_off) and not eoff2.any()
    assert_same_events(ev[:int(eoff[-1])], want, "first detection")
    # refusals of begin, nothing enqueued: an empty chunk, descending offsets, a window above 65 535
    bad = off.copy()
    bad[5] = bad[4]
    assert lib.rawdtw_detect_begin(eng._ctx, None, 64, vp(bad), vp(sig), vp(eoff2), vp(ev2), int(off[-1])) == 1
    bad[5] = bad[4] - 1
    assert lib.rawdtw_detect_begin(eng._ctx, None, 64, vp(bad), vp(sig), vp(eoff2), vp(ev2), int(off[-1])) == 1
    o = ra.EventOptions(window_length2=70000).c()
    assert lib.rawdtw_detect_begin(eng._ctx, C.byref(o), 64, vp(off), vp(sig), vp(eoff2), vp(ev2), int(off[-1])) == 1
    assert lib.rawdtw_detect_end(eng._ctx, None) == 1  # (none of them began anything)
    assert not eoff2.any()


@pytest.mark.gpu
def test_too_small_events_cap_gives_range_with_event_off_filled(eng):
    reads = make_raw_reads(40, 4000, seed=36)
    sig, off = batch(reads)
    want_off, _ = ra.detect_events_host(sig, off)
    with pytest.raises(RawDTWError) as e:
        eng.detect_events(sig, off, pinned=False, events_cap=int(want_off[-1]) - 1)
    assert e.value.status == 4
    assert np.array_equal(e.value.event_off, want_off)
    got_off, got = eng.detect_events(sig, off, pinned=False, events_cap=int(want_off[-1]))  # exactly enough
    assert np.array_equal(got_off, want_off)
    with pytest.raises(RawDTWError) as e:
        eng.detect_events(sig, off, pinned=True, events_cap=100)
    assert e.value.status == 4 and np.array_equal(e.value.event_off, want_off)


@pytest.mark.gpu
def test_detection_between_batch_submit_and_fetch_changes_neither(eng):
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
    reads = make_raw_reads(512, 4000, seed=43)
    sig, off = batch(reads)

    def run(with_detection):
        h = C.c_void_p()
        assert lib.rawdtw_batch_submit(eng._ctx, C.byref(co), cb.n_reads, *[vp(a) for a in arrs], C.byref(h)) == 0
        det = eng.detect_events(sig, off) if with_detection else None
        score, keep = np.zeros(cb.n_chains + 1, F32), np.zeros(cb.n_chains + 1, np.uint8)
        assert lib.rawdtw_batch_fetch_destroy(eng._ctx, h, vp(score), vp(keep)) == 0
        return score[:cb.n_chains].copy(), keep[:cb.n_chains].copy(), det

    s0, k0, _ = run(False)
    s1, k1, (eoff, ev) = run(True)
    assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)) and np.array_equal(k0, k1)
    want_off, want = ra.detect_events_host(sig, off, threads=16)
    assert np.array_equal(eoff, want_off)
    assert_same_events(ev, want, "beside a batch")
