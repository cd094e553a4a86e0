"""What tests/shape_lattice_cases.py claims, derived and pinned without a device: the table of which lane body a part meets at
which fraction and up to what length, the identity between classify()'s division-free radius (rawdtw_runs.hip) and
slanted_radius() (dtw.cpp:298-300) over the whole lattice, the library's job lists for the arrangements, the host planner on
the job-list lattice under every knob set, the input conditions of the fold cases by the oracle alone, and the generated
wave-band header against its generator.

Sensitivity, shown here and not on the device (a wrong radius there indexes outside a pass's LDS image): the restated
identity with either `>` read as `>=` fails test_classify_identity (test_classify_identity_is_sharp)."""
import os
import sys

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd._lib import load_library
from rawalign_amd.dtw import plan_dry_run
from tests import shape_lattice_cases as L


def test_table_of_reachable_bodies():
    """per fraction: the tile parts of radius 1, 2, 3 (pairs, longest N) and the side list's pairs over [1, 80]^2; the distinct
    tile records over all fractions"""
    records = set()
    print()
    print("frac   R=1 pairs (N)   R=2 pairs (N)   R=3 pairs (N)   side list")
    for frac in L.FRACS:
        row = L.table_row(frac)
        print(f"{frac:<5}  {row[0][0]:>5} ({row[0][1]:>2})      {row[1][0]:>5} ({row[1][1]:>2})      {row[2][0]:>5} ({row[2][1]:>2})      {row[3]:>5}")
        assert row == L.TABLE[frac], frac
        assert sum(r[0] for r in row[:3]) + row[3] == len(L.STREAM_LATTICE)
        records |= {t for t in (L.tile_record(n, m, frac) for n, m in L.STREAM_LATTICE) if t is not None}
    at_default = {t for t in (L.tile_record(n, m, 0.10) for n, m in L.STREAM_LATTICE) if t is not None}
    print(f"distinct tile records over the fractions: {len(records)} of {73 * 73 * 3 + 73 * 3} the record can hold; pairs at 0.10: {len(at_default)}")
    assert len(records) == L.N_TILE_RECORDS
    assert L.TABLE[0.10][0][1] == 19   # the default fraction runs lane_dp_r1 up to N = 19 only


def _classify(n, m, frac, gt=lambda a, b: a > b, lane_max_n=L.LANE_MAX_N, lane_max_radius=L.LANE_MAX_RADIUS):
    """classify() of rawdtw_runs.hip as it is written: no division"""
    r0 = int(np.float32(n) * np.float32(frac))
    r0 = r0 if r0 > 1 else 1
    N = n if n > m else m
    dr = (N - (m if n > m else n)) * r0
    R = r0 + (1 if gt(dr, 0) else 0) + (1 if gt(dr, N) else 0)
    tile = N <= lane_max_n and r0 <= lane_max_radius and dr <= (lane_max_radius - r0) * N
    return R, tile


def _identity_failures(gt=lambda a, b: a > b):
    bad = []
    for frac in L.FRACS:
        for n, m in L.STREAM_LATTICE:
            R, tile = _classify(n, m, frac, gt)
            want_R = L.radius(n, m, frac)
            want_tile = max(n, m) <= L.LANE_MAX_N and want_R <= L.LANE_MAX_RADIUS
            if tile != want_tile or (want_tile and R != want_R):
                bad.append((frac, n, m, R, want_R, tile, want_tile))
    return bad


def test_classify_identity():
    """tile eligibility everywhere, and the radius wherever the part is a tile's (the only place classify()'s R counts), equal
    slanted_radius(); the lattice holds the boundaries dr == N and dr == 2N, where the identity could break, at every r0 <= 3
    that has them: dr = (N - M) r0 < N r0 with M >= 1, so dr == N needs r0 >= 2 (M = N / 2 at 2, 2N / 3 at 3) and dr == 2N needs
    r0 = 3 (M = N / 3) -- and one short of and one beyond each of them"""
    assert _identity_failures() == []
    seen = set()
    for frac in L.FRACS:
        for n, m in L.STREAM_LATTICE:
            r0, N = L.r0_of(n, frac), max(n, m)
            dr = (N - min(n, m)) * r0
            if r0 <= 3 and N <= L.LANE_MAX_N:
                seen |= {(r0, k, d) for k in (1, 2) for d in (-1, 0, 1) if dr == k * N + d}
    at = {(r0, k) for r0, k, d in seen if d == 0}
    assert at == {(2, 1), (3, 1), (3, 2)}, at
    assert {(r0, k, d) for r0, k in at for d in (-1, 1)} <= seen


def test_classify_identity_is_sharp():
    """with `>` read as `>=` the restated identity breaks (at dr == N: a radius one too large)"""
    bad = _identity_failures(gt=lambda a, b: a >= b)
    assert bad and any((max(n, m) - min(n, m)) * L.r0_of(n, frac) == max(n, m) for frac, n, m, *_ in bad)


@pytest.fixture(scope="module")
def ref():
    return L.reference()


@pytest.mark.parametrize("frac", L.FRACS)
def test_library_job_lists_equal_the_cases(ref, frac):
    """rawdtw_batch_build_jobs at the fraction: every part of the singles and shuffled arrangements with the cases module's n, m,
    band_radius (r0: the slant is the kernels') and exclude_last"""
    lib = load_library()
    for name in ("singles", "shuffled"):
        for chains, per_read in L.arrangement(name, frac):
            case = L.make_case(chains, ref, per_read)
            jobs, job_off = L.build_jobs(lib, case.cb, L.align_opt(frac))
            n, m, r0, ex = L.expected_parts(chains, frac)
            assert len(jobs) == len(n) == sum(len(c) for c in chains)
            for got, want in ((jobs["n"], n), (jobs["m"], m), (jobs["band_radius"], r0), (jobs["exclude_last"], ex)):
                assert np.array_equal(got.astype(np.int64), want), (name, frac)
            assert int(job_off[-1]) == len(jobs)


def test_arrangements_hold_the_lattice_once():
    for frac in L.FRACS:
        for name in ("sorted", "shuffled", "singles"):
            parts = [p for chains, _ in L.arrangement(name, frac) for c in chains for p in c]
            assert sorted(parts) == L.STREAM_LATTICE and all(len(c) <= L.CHAIN_PARTS for chains, _ in L.arrangement(name, frac) for c in chains)
        for c in L.peak_parts(frac):
            assert len({L.tile_record(n, m, frac)[2] for n, m in c}) == 1


def test_dry_run_of_the_job_lattice():
    """the host planner takes the job-list lattice under every knob set, and every class the set routes jobs to has some"""
    jobs, events, rf = L.job_lattice()
    assert len(jobs) == 100 * 100 * 10 * 2 + 81 * 3 * 2
    got = {}
    print()
    for knobs in L.KNOB_SETS:
        if "device_plan" in knobs:   # (the context's choice between its two paths: the planner is the same)
            continue
        info, tiles = plan_dry_run(jobs, len(events), 2 * len(rf), options=knobs)
        got[L.knob_id(knobs)] = info
        print(f"{L.knob_id(knobs):<18} lane {info['n_lane_jobs']:>6}  wave/band {info['n_wave_band_jobs']:>6}  full {info['n_full_jobs']}  tiles {tiles}")
        assert info["n_jobs"] == len(jobs) and info["n_lane_jobs"] + info["n_wave_band_jobs"] == len(jobs) and info["n_full_jobs"] == 0
        assert info["n_lane_jobs"] > 0 and info["n_wave_band_jobs"] > 0 and tiles > 0
    d = got["default"]["n_lane_jobs"]
    assert got["lane_max_radius1"]["n_lane_jobs"] < d and got["lane_max_n20"]["n_lane_jobs"] < d


@pytest.mark.parametrize("frac", L.FOLD_FRACS)
def test_fold_inputs_decide_between_keep_and_cut(oracle, ref, frac):
    """by the oracle alone: at every finite min_score at least a fifth of the chains are kept and at least a fifth cut (-1e10), and
    among the kept chains of at least one read in ten the running best rises more than once"""
    cases = L.fold_cases(frac, L.fold_reference())
    lens = [len(c) for _, chains in cases for c in chains]
    reads = np.concatenate([np.diff(case.cb.chain_off.astype(np.int64)) for case, _ in cases])
    assert min(lens) >= 1 and max(lens) <= 120 and reads.min() >= 3 and reads.max() <= 12 and sum(lens) == len(L.STREAM_LATTICE)
    lib = load_library()
    print()
    for bonus, min_score, fused in L.FOLD_PARAMS:
        opt = ra.MapOpt(dtw_band_radius_frac=frac, dtw_match_bonus=bonus, dtw_min_score=min_score, fused_score=fused)
        keeps, cuts, rises = [], [], 0
        for case, _ in cases:
            cb = case.cb
            jobs, _ = L.build_jobs(lib, cb, opt)
            score, keep, _ = L.oracle_expect(oracle, case, jobs, opt)
            keeps.append(keep.astype(bool))
            cuts.append(score == np.float32(-1e10))
            for r in range(cb.n_reads):
                best, n = np.float32(0.0), 0
                for c in range(int(cb.chain_off[r]), int(cb.chain_off[r + 1])):
                    if keep[c] and score[c] > best:
                        best, n = score[c], n + 1
                rises += n > 1
        keep, cut = np.concatenate(keeps), np.concatenate(cuts)
        print(f"frac {frac} bonus {bonus} min_score {min_score:g} fused {int(fused)}: {len(keep)} chains in {len(reads)} reads, kept {keep.mean():.2f}, "
              f"cut {cut.mean():.2f}, reads whose best rises more than once {rises}")
        if min_score > -1e8:
            assert keep.mean() >= 0.2 and cut.mean() >= 0.2
            assert rises * 10 >= len(reads)
        else:   # nothing falls below the bound: every chain is kept unless the read's running best cut it (rmap.cpp:515: from 0)
            assert np.array_equal(keep, ~cut)


def test_generated_header_is_the_generators():
    """rawalign_amd/csrc/rawdtw_wband_asm.h is what scripts/gen_wband_asm.py writes, byte for byte (the Makefile does not regenerate it)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    try:
        import gen_wband_asm
    finally:
        sys.path.pop(0)
    with open(os.path.join(root, "rawalign_amd", "csrc", "rawdtw_wband_asm.h"), "rb") as f:
        assert f.read() == gen_wband_asm.header_text().encode()
