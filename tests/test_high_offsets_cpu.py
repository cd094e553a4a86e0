"""tests/high_offset_cases.py pinned on the CPU, so that a drifting generator cannot hollow out tests/test_high_offsets_gpu.py: the places
straddle what they claim to, the decoys lie where a truncated offset lands and hold other content, every job used answers differently
on that content, and the three direction lists pass 2^32 + 2^28 bytes in one sub-batch by the formulas."""
import numpy as np
import pytest

import rawalign_amd as ra
from tests import banded_tb_cases as bc
from tests import high_offset_cases as hc
from tests import traceback_cases as tc
from tests.util import oracle_costs


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_every_place_straddles_what_it_claims():
    assert hc.REF_FLOATS == (1 << 32) + (1 << 27) and hc.EV_FLOATS == (1 << 31) + (1 << 27) and hc.EV_FLOATS < (1 << 32)
    for places, marks, seg, arena in ((hc.REF_PLACES, hc.REF_MARKS, hc.SEG_REF, hc.REF_FLOATS), (hc.EV_PLACES, hc.EV_MARKS, hc.SEG_EV, hc.EV_FLOATS)):
        assert places[0] == 0 and places[3] + seg == arena and list(places) == sorted(places)
        for p, mark in zip(places, marks):
            if mark is not None:
                assert p < mark < p + seg and p % 4 != 0
                assert min(mark - p, p + seg - mark) >= seg // 4   # a good part of the segment on either side
        for a, b in zip(places, places[1:]):
            assert a + seg <= b
    assert hc.REF_MARKS[1:3] == (1 << 30, 1 << 32) and hc.EV_MARKS[1:3] == (1 << 30, 1 << 31)
    # windows of every list lie on both sides of the mark inside a straddling copy
    for jobs in (hc.score_jobs(), hc.semiglobal_jobs()):
        for key, places, marks in (("ref_off", hc.REF_PLACES, hc.REF_MARKS), ("read_off", hc.EV_PLACES, hc.EV_MARKS)):
            for p, mark in zip(places[1:3], marks[1:3]):
                at = jobs[key].astype(np.int64) + p
                assert (at < mark).any() and (at >= mark).any()


def test_every_decoy_exists_is_disjoint_and_differs():
    assert hc.REF_DECOYS == [(1 << 27) - hc.SEG_REF, (1 << 31) - 60003]
    assert hc.EV_DECOYS == [(1 << 27) - hc.SEG_EV]
    for places, dec, seg, arena in ((hc.REF_PLACES, hc.REF_DECOYS, hc.SEG_REF, hc.REF_FLOATS), (hc.EV_PLACES, hc.EV_DECOYS, hc.SEG_EV, hc.EV_FLOATS)):
        spans = sorted([(p, p + seg) for p in places] + [(d, d + seg) for d in dec])
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= arena
        # wherever a place, taken modulo a power of two below it, is another offset, a decoy or a planted copy at another shift lies there
        for p in places:
            for w in hc.MODULI:
                kind, shift = hc.alias_of(p, w, places, dec, seg)
                assert kind in ("same", "decoy", "planted"), (p, w)
                if kind == "planted":
                    assert shift > 1000, (p, w, shift)
        # the arena's end (past every mark) always meets a decoy
        assert all(hc.alias_of(places[3], w, places, dec, seg)[0] == "decoy" for w in hc.MODULI if places[3] >= w)
    for seg, decoy in ((hc.ref_segment(), hc.ref_decoy()), (hc.ev_segment(), hc.ev_decoy())):
        assert seg.shape == decoy.shape and np.isfinite(seg).all() and np.isfinite(decoy).all()
        assert (bits(seg) != bits(decoy)).mean() > 0.99 and (bits(seg) != bits(hc.FILL)[0]).all()
        for shift in (9998, 39998, 100001):   # a copy read at another offset is other content as well
            if shift < len(seg) // 2:
                assert (bits(seg[shift:shift + 20000]) != bits(seg[:20000])).mean() > 0.99


def test_shifted_goes_there_and_back():
    low, high = hc.spread(hc.semiglobal_jobs(), 16)
    assert len(low) == 16 * len(hc.semiglobal_jobs())
    ri, ei = hc.round_robin(len(low))
    assert {(int(a), int(b)) for a, b in zip(ri[:16], ei[:16])} == {(a, b) for a in range(4) for b in range(4)}
    assert np.array_equal(high["ref_off"] - low["ref_off"], np.array(hc.REF_PLACES, np.uint64)[ri])
    assert np.array_equal(high["read_off"].astype(np.int64) - low["read_off"], np.array(hc.EV_PLACES, np.int64)[ei])
    assert (high["ref_off"] >= (1 << 32)).any() and (high["read_off"] >= (1 << 31)).any()
    assert (high["ref_off"] + high["m"]).max() <= hc.REF_FLOATS and (high["read_off"].astype(np.int64) + high["n"]).max() <= hc.EV_FLOATS
    back = hc.shifted(high, np.array(hc.REF_PLACES, np.int64)[ri], np.array(hc.EV_PLACES, np.int64)[ei], back=True)
    assert back.tobytes() == low.tobytes()
    cb = hc.candidate_batch()
    rp, ep = hc.batch_places()
    hi = hc.shifted(cb, rp, ep)
    assert (hi.ref_base >= (1 << 32)).any() and (hi.read_base >= (1 << 30)).any() and (hi.read_base >= (1 << 31)).any()
    for r in range(cb.n_reads):   # a read's chains share its events
        assert len(set(hi.read_base[int(cb.chain_off[r]):int(cb.chain_off[r + 1])].tolist())) == 1
    lo = hc.shifted(hi, rp, ep, back=True)
    assert np.array_equal(lo.ref_base, cb.ref_base) and np.array_equal(lo.read_base, cb.read_base)


# ---- an aliased read is a certain mismatch: every job answers differently on the decoy content ---------------------------------------------
CONTENTS = ("events", "reference", "both")


def contents(which):
    return (hc.ev_decoy() if which != "reference" else hc.ev_segment(), hc.ref_decoy() if which != "events" else hc.ref_segment())


@pytest.mark.parametrize("which", CONTENTS)
def test_decoy_content_changes_every_scoring_job(oracle, which):
    ev, ref = contents(which)
    for jobs in (hc.score_jobs(), hc.class_jobs(), hc.traceback_jobs(), hc.direction_windows("full")):
        want = oracle_costs(oracle, jobs, hc.ev_segment(), hc.ref_segment())
        other = oracle_costs(oracle, jobs, ev, ref)
        assert (bits(want) != bits(other)).all()


@pytest.mark.parametrize("which", CONTENTS)
def test_decoy_content_changes_every_semiglobal_and_banded_job(which):
    ev, ref = contents(which)
    for jobs in (hc.semiglobal_jobs(), hc.direction_windows("semiglobal")):
        for (a, b, _, ex), (x, y, _, _) in zip(hc.windows(jobs), hc.windows(jobs, ev, ref)):
            if len(a) == 1 and ex:
                continue   # (one row less itself: 0 on any content; its end column still moves)
            assert bits(ra.semiglobal_host(a, b, ex)[0])[0] != bits(ra.semiglobal_host(x, y, ex)[0])[0], (len(a), len(b))
    for jobs in (hc.banded_jobs(), hc.direction_windows("banded")):
        for (a, b, R, ex), (x, y, _, _) in zip(hc.windows(jobs), hc.windows(jobs, ev, ref)):
            assert bits(ra.banded_tb_host(a, b, R, ex).cost)[0] != bits(ra.banded_tb_host(x, y, R, ex).cost)[0], (len(a), len(b), R)


@pytest.mark.parametrize("which", CONTENTS)
def test_decoy_content_changes_every_batch_job(oracle, which):
    ev, ref = contents(which)
    cb = hc.candidate_batch()
    for opt in (ra.MapOpt(), ra.MapOpt(dtw_border_constraint=0, dtw_fill_method=0), ra.MapOpt(dtw_border_constraint=0, dtw_fill_method=1)):
        want, other = hc.batch_expected(oracle, cb, opt), hc.batch_expected(oracle, cb, opt, ev, ref)
        assert (bits(want[2]) != bits(other[2])).all() and len(want[2]) >= cb.n_chains
        assert 0 < want[1].sum() < cb.n_chains   # kept and cut chains both
    opt = ra.MapOpt(dtw_border_constraint=2)
    want, other = hc.local_expected(cb, opt), hc.local_expected(cb, opt, ev, ref)
    assert (bits(want[2]) != bits(other[2])).all() and len(want[2]) == cb.n_chains and 0 < want[1].sum() < cb.n_chains


# ---- the direction lists ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["full", "semiglobal", "banded"])
def test_direction_lists_pass_the_mark_in_one_sub_batch(kind):
    low, high, which = hc.direction_jobs(kind)
    win = hc.direction_windows(kind)
    assert len(win) == hc.N_WINDOWS == len({(int(j["n"]), int(j["m"]), int(j["band_radius"])) for j in win}) and set(which.tolist()) == set(range(7))
    assert low.tobytes() == win[which].tobytes()
    total = hc.direction_total(kind, low)
    assert total > hc.DIR_FLOOR and hc.direction_total(kind, low[:-1]) <= hc.DIR_FLOOR   # the smallest prefix of the cycle that passes
    assert hc.sub_batches(kind, low) == [len(low)] and total + 256 * len(low) < hc.BUDGET
    assert len(hc.sub_batches(kind, low, 1 << 30)) >= 4   # (the cut's restatement does cut)
    # the restated formulas against the helpers the suite already has
    if kind == "full":
        assert tc.split([(int(j["n"]), int(j["m"])) for j in low], tc.DEFAULT_BUDGET) == [(0, len(low))]
        assert tc.split([(int(j["n"]), int(j["m"])) for j in low], 1 << 30) == [(b, c) for b, c in zip(np.cumsum([0] + hc.sub_batches(kind, low, 1 << 30))[:-1], hc.sub_batches(kind, low, 1 << 30))]
    if kind == "banded":
        assert bc.sub_batches(low, tc.DEFAULT_BUDGET >> 20) == [len(low)] and bc.sub_batches(low, 1024) == hc.sub_batches(kind, low, 1 << 30)
        assert all(bc.slanted_radius(int(j["n"]), int(j["m"]), int(j["band_radius"])) + 1 <= bc.MAX_K for j in win)
    if kind == "semiglobal":   # the same shapes cost a full-matrix traceback the same bytes when the events are the shorter side
        assert all(hc.semi_dir_bytes(int(j["n"]), int(j["m"])) == tc.dir_bytes_for(int(j["n"]), int(j["m"])) for j in win)
        assert sorted({hc.semi_class(int(j["n"]), int(j["m"])) for j in win}) == [0, 1, 2, 3, 4]
        assert 3.9e9 < hc.semi_dir_bytes(400, 29903) * 1024 < 1 << 32   # profiles/semiglobal_span_probe.json's 1 024 jobs: 3.9 GB, below the mark
    assert (high["ref_off"] >= (1 << 32)).any() and (high["read_off"] >= (1 << 31)).any()
    assert len(low) < 1500 and int((low["n"].astype(np.int64) + low["m"] - 1).sum()) < 40_000_000   # a few hundred jobs, paths of a few dozen MB


def test_the_seven_windows_host_paths_are_the_oracles(oracle):
    """where the oracle has the function: DTW_global_tb for the full matrix, the banded cost for the banded traceback; the semiglobal
    restatements against each other (the traceback's cost, start and end columns are the span's)"""
    for a, b, R, ex in hc.windows(hc.direction_windows("banded")):
        r = ra.banded_tb_host(a, b, R, ex)
        assert bits(r.cost)[0] == bits(oracle.dtw_banded(a, b, R, ex))[0] and len(r.i) > 0
    for a, b, _, ex in hc.windows(hc.direction_windows("semiglobal")):
        r, ej = ra.semiglobal_host(a, b, ex, traceback=True)
        c, j0, sej = ra.semiglobal_span_host(a, b, ex)
        assert bits(r.cost)[0] == bits(c)[0] and ej == sej and int(r.j[0]) == j0
    for a, b, _, ex in hc.windows(hc.direction_windows("full"))[:3]:
        c, pi, pj, pd = oracle.dtw_global_tb(a, b, ex)
        assert bits(c)[0] == bits(oracle.dtw_global(a, b, ex))[0] and pi[0] == 0 and pj[0] == 0
