"""Seeding a minimizer index (w > 0) on the device with the context's "seed_minimizer" option on (rawdtw_seed.hip: k_seed_filter
without the mask test, k_seed_min, k_seed_probe on given hashes) against the reference's recorded answers (tests/golden/seed_ref.npz,
seed_min_ref.npz) and the host path, hit for hit and in order; the resident form, the chaining behind it and the mapper's two seeded
rounds.  Exact equality of integers and float bits everywhere.  Nothing here reads the reference itself."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapper, seeding
from rawalign_amd import mapping as M
from rawalign_amd.dtw import ANCHOR_DTYPE
from rawalign_amd.events import PinnedArray
from rawalign_amd.seeding import HIT_DTYPE, SeedIndex, SeedParams
from tests import map_ref_cases as mc
from tests import seed_cases as sc
from tests import seed_min_cases as smc
from tests.test_device_chain import REC_DTYPE, SEED_DTYPE
from tests.test_resident_round_gpu import _whole_mapper, place_in_arena, same_hits, seeds_of, vp

pytestmark = pytest.mark.gpu
INVALID, RANGE, UNSUPPORTED = 1, 4, 5
OPTION = "seed_minimizer"


@pytest.fixture(scope="module")
def ref():
    return mc.make_reference()


@pytest.fixture(scope="module")
def six5(ref):
    return SeedIndex.from_signals(ref.forward, ref.reverse, SeedParams(w=5), threads=4)


def engine(si, on=True):
    e = ra.Engine(0)
    if on:
        e.set_option(OPTION, 1)
    e.upload_seed_index(si)
    return e


def check_against_host(eng, si, chunks, what, **kw):
    ev, off = sc.flat(chunks)
    want_off, want = seeding.seed_hits_host(si, ev, off, threads=16)
    got_off, got = eng.seed_hits(ev, off, **kw)
    assert np.array_equal(got_off, want_off), what
    same_hits(got, want, what)
    return want_off, want


# ---- 1. device = host = fixture ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w1", "w5", "w10", "w255"])
def test_device_equals_the_recorded_minimizer_cases(name):
    sfx = sc.Fixture()
    fwd, rev, p, chunks = sc.build_case(name)
    assert p.w == int(name[1:]) and sc.case_sha256(fwd, rev, chunks) == sfx.sha(name)
    si = SeedIndex.from_signals(fwd, rev, p, threads=4)
    e = engine(si)
    try:
        ev, off = sc.flat(chunks)
        for pinned in (True, False):
            hoff, hits = e.seed_hits(ev, off, pinned=pinned)
            assert np.array_equal(hoff, sfx.hit_off(name)) and np.array_equal(sc.hit_rows(hits), sfx.hits(name)), (name, pinned)
            assert len(hits) > 0
        check_against_host(e, si, chunks, name)
    finally:
        e.close()


@pytest.mark.parametrize("name", smc.CASES)
def test_device_equals_the_tie_fixture(name):
    fx = smc.Fixture()
    fwd, rev, p, chunks = smc.build_case(name)
    assert sc.case_sha256(fwd, rev, chunks) == fx.sha(name)
    si = SeedIndex.from_signals(fwd, rev, p, threads=4)
    e = engine(si)
    try:
        ev, off = sc.flat(chunks)
        for pinned in (True, False):
            hoff, hits = e.seed_hits(ev, off, pinned=pinned)
            assert np.array_equal(hoff, fx.hit_off(name)) and fx.check_rows(name, sc.hit_rows(hits)), (name, pinned)
            assert len(hits) > 0
        check_against_host(e, si, chunks, name)
    finally:
        e.close()


# ---- 2. a batch of mixed lengths --------------------------------------------------------------------------------------------------------
def mixed_chunks(ref, e=6, w=5):
    rng = np.random.default_rng(6)
    edge = list(range(e - 1, e + w + 1))   # e - 1 .. e + w
    chunks = []
    for k in range(300):
        arr = (ref.forward, ref.reverse)[k % 2][k % 3]
        lo = int(rng.integers(0, len(arr) - 500))
        n = ([0, 1] + edge)[(k // 4) % (2 + len(edge))] if k % 4 == 0 else int(rng.integers(1, 501))
        chunks.append(np.ascontiguousarray(arr[lo:lo + n], np.float32))
    chunks[0], chunks[-1] = chunks[0][:0], chunks[-1][:0]   # (the batch's first and last chunk are empty)
    chunks[150] = np.ascontiguousarray(ref.forward[0][1000:1500], np.float32)
    return chunks


def test_a_batch_of_mixed_lengths_equals_the_host(ref, six5):
    chunks = mixed_chunks(ref)
    lens = {len(c) for c in chunks}
    assert lens >= set([0, 1] + list(range(5, 12))) and max(lens) == 500
    e = engine(six5)
    try:
        want_off, want = check_against_host(e, six5, chunks, "pinned", pinned=True)
        check_against_host(e, six5, chunks, "pageable", pinned=False)
        assert len(want) > 1000
        ev, off = sc.flat(chunks)
        assert e.seed_hits(ev, off, pinned=True, kernel_ms=True)[2] > 0
    finally:
        e.close()


def test_a_cap_one_short_is_range_with_the_offsets_filled_and_no_hit_written(ref, six5):
    lib = ra.load_library()
    chunks = mixed_chunks(ref)[140:160]
    ev, off = sc.flat(chunks)
    n = len(chunks)
    want_off, want = seeding.seed_hits_host(six5, ev, off)
    total = int(want_off[-1])
    assert total > 100
    p = lambda a: a.ctypes.data  # noqa: E731
    e = engine(six5)
    try:
        for pinned in (True, False):
            if pinned:
                keep = [PinnedArray(n + 1, np.uint64), PinnedArray(total, HIT_DTYPE)]
                hoff, hits = keep[0].array, keep[1].array
            else:
                hoff, hits = np.zeros(n + 1, np.uint64), np.zeros(total, HIT_DTYPE)
            hits.view(np.uint8)[:] = 0xAB
            canary = hits.copy()
            assert lib.rawdtw_seed_begin(e._ctx, n, p(off), p(ev), p(hoff), p(hits), total - 1) == 0
            assert lib.rawdtw_seed_end(e._ctx, None) == RANGE
            assert np.array_equal(hoff, want_off) and np.array_equal(hits, canary), pinned
            assert lib.rawdtw_seed_begin(e._ctx, n, p(off), p(ev), p(hoff), p(hits), total) == 0   # exactly enough
            assert lib.rawdtw_seed_end(e._ctx, None) == 0
            same_hits(hits[:total], want, "exact cap")
    finally:
        e.close()


# ---- 3. resident ---------------------------------------------------------------------------------------------------------------------------
def test_resident_minimizer_seeding_and_the_chaining_behind_it(ref, six5):
    """tests/test_resident_round_gpu.py's shape at w = 5: chunks in scattered slots of the event arena, _fetch against the host, and
    rawdtw_chain_round_begin_resident against rawdtw_chain_round fed the host-built seed list, bit for bit."""
    rng = np.random.default_rng(45)
    fx = mc.Fixture(ref=ref)
    chunks = [np.ascontiguousarray(fx.events[int(fx.ev_off[k]):int(fx.ev_off[k + 1])]) for k in range(0, 40)]
    chunks[7] = np.ascontiguousarray(ref.forward[0][30:34])                       # a read with no hits (shorter than e) ...
    chunks[11] = rng.normal(0, 3, 300).astype(np.float32)                         # ... and one from nowhere
    n = len(chunks)
    copt = M.default_chain_opt(mc.E)
    e = engine(six5)
    lib = e.lib
    try:
        start, ln = place_in_arena(e, chunks, rng)
        ev, off = sc.flat(chunks)
        hoff, hits = seeding.seed_hits_host(six5, ev, off, threads=8)
        assert len(hits) > 500
        rs = e.seed_resident(start, ln, kernel_ms=True)
        assert np.array_equal(rs.hit_off, hoff)
        for pinned in (True, False):
            same_hits(rs.fetch(pinned=pinned), hits, ("fetch", pinned))
        hoff = hoff.astype(np.int64)
        sits = np.zeros(n, np.uint8)
        sits[[3, 20, n - 1]] = 1                                                   # reads that sit the round out
        chunk_start = rng.integers(0, 3000, n).astype(np.uint32)                   # non-zero chunk starts ...
        chunk_start[0] = 0
        prev = []                                                                  # ... and previous seeds for two reads in three
        for r in range(n):
            k = 0 if sits[r] or r % 3 == 0 else int(rng.integers(1, 60))
            p = np.zeros(k, SEED_DTYPE)
            p["key"], p["target_position"], p["query_position"] = rng.integers(0, 6, k), rng.integers(0, 6000, k), rng.integers(0, 3000, k)
            if k > 4:   # (a true little chain among them)
                p["key"][:4], p["target_position"][:4], p["query_position"][:4] = 1, 500 + 9 * np.arange(4), 40 + 9 * np.arange(4)
            prev.append(p)
        per_read = [np.zeros(0, SEED_DTYPE) if sits[r] else np.concatenate([prev[r], seeds_of(hits[hoff[r]:hoff[r + 1]], chunk_start[r])]) for r in range(n)]
        assert len(per_read[7]) == len(prev[7])
        seed_off = np.concatenate([[0], np.cumsum([len(s) for s in per_read])]).astype(np.uint64)
        prev_off = np.concatenate([[0], np.cumsum([len(p) for p in prev])]).astype(np.uint64)
        prev_all = np.concatenate(prev + [np.zeros(1, SEED_DTYPE)])
        read_base = (np.arange(n, dtype=np.uint32) * 1000).astype(np.uint32)
        key_base = (np.arange(6, dtype=np.uint64) * 100000 + 7).astype(np.uint64)
        cap = n * 32

        def outs():
            return np.zeros(n + 1, np.uint64), np.zeros(cap + 1, np.uint64), np.zeros(cap, REC_DTYPE), np.zeros(int(seed_off[-1]) + 1, ANCHOR_DTYPE)

        d = [C.c_void_p() for _ in range(3)]
        want = outs()
        allseeds = np.concatenate(per_read + [np.zeros(1, SEED_DTYPE)])
        assert lib.rawdtw_chain_round(e._ctx, C.byref(copt), n, vp(seed_off), vp(allseeds), vp(read_base), 6, vp(key_base), vp(want[0]), vp(want[1]),
                                      vp(want[2]), cap, vp(want[3]), *[C.byref(x) for x in d]) == 0
        nc = int(want[0][-1])
        na = int(want[1][nc])
        assert nc >= 10 and na > 2 * nc   # (chains, and anchors in them: not a comparison of nothing)
        got = outs()
        assert lib.rawdtw_chain_round_begin_resident(e._ctx, C.byref(copt), n, vp(seed_off), vp(prev_off), vp(prev_all), vp(chunk_start), vp(sits),
                                                     vp(read_base), 6, vp(key_base), vp(got[0]), vp(got[1]), vp(got[2]), cap, vp(got[3])) == 0, lib.rawdtw_last_error(e._ctx)
        assert lib.rawdtw_chain_round_end(e._ctx, *[C.byref(x) for x in d]) == 0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1][:nc + 1], want[1][:nc + 1])
        assert got[2][:nc].tobytes() == want[2][:nc].tobytes() and got[3][:na].tobytes() == want[3][:na].tobytes()
    finally:
        e.close()


# ---- 4. the mapper --------------------------------------------------------------------------------------------------------------------------
MAPPER_W, MAPPER_HOST_MAPPED = 5, 8   # the choice below and the host's count


def test_the_mapper_seeds_a_minimizer_round_on_its_context(ref):
    """Whole raw reads at the largest w of {5, 3, 2} for which the HOST-seeded mapper maps at least half of the nine: the lines of
    rawdtw_mapper_round_seeded with the option on, and of rawdtw_mapper_round_seeded_resident, are the host-seeded mapper's, whole."""
    wr = mc.WholeReads(0, ref=ref)
    assert wr.n_reads == 9
    opt, copt = mc.whole_project_opts("default", 0)
    reads = list(range(wr.n_reads))

    def lines(si, on, resident=False):
        e = ra.Engine(0)
        try:
            if on:
                e.set_option(OPTION, 1)
            e.upload_reference(ref.forward, ref.reverse)
            cm = _whole_mapper(e, wr, opt, copt, groups=1, device_chain=True)
            got, rounds = mapper.map_reads_c(wr, reads, cm, seed_index=si, resident=resident)
            st = cm.resident_stats()
            cm.close()
            return got, rounds, st
        finally:
            e.close()

    chosen = None
    for w in (5, 3, 2):
        si = SeedIndex.from_signals(ref.forward, ref.reverse, SeedParams(w=w), threads=4)
        host, rounds, st = lines(si, False)
        mapped = sum("\t*\t" not in ln for ln in host)
        print("w = %d: the host-seeded mapper maps %d of %d reads in %d rounds" % (w, mapped, wr.n_reads, rounds))
        if 2 * mapped >= wr.n_reads:
            chosen = w
            break
    assert chosen is not None
    assert (chosen, mapped) == (MAPPER_W, MAPPER_HOST_MAPPED)
    assert st == dict(resident_rounds=0, fallback_rounds=0, hit_bytes_to_host=0, seed_bytes_to_device=0)
    got, rounds_d, _ = lines(si, True)
    assert got == host and rounds_d == rounds
    got, rounds_r, st = lines(si, True, resident=True)
    print("resident:", rounds_r, st)
    assert got == host and rounds_r == rounds
    assert st["resident_rounds"] > 0 and st["fallback_rounds"] == 0 and st["hit_bytes_to_host"] == 0


# ---- 5. the option off ----------------------------------------------------------------------------------------------------------------------
def test_with_the_option_off_a_minimizer_table_is_refused_as_before(ref, six5):
    lib = ra.load_library()
    chunks = mixed_chunks(ref)[140:160]
    ev, off = sc.flat(chunks)
    n = len(chunks)
    want_off, want = seeding.seed_hits_host(six5, ev, off)
    total = int(want_off[-1])
    p = lambda a: a.ctypes.data  # noqa: E731
    hoff, hits = np.zeros(n + 1, np.uint64), np.zeros(total, HIT_DTYPE)
    e = engine(six5, on=False)
    try:
        v = C.c_int64(-1)
        assert lib.rawdtw_get_option(e._ctx, OPTION.encode(), C.byref(v)) == 0 and v.value == 0
        assert lib.rawdtw_seed_begin(e._ctx, n, p(off), p(ev), p(hoff), p(hits), total) == UNSUPPORTED
        assert b"rawdtw_seed_hits_host" in lib.rawdtw_last_error(e._ctx)
        assert lib.rawdtw_seed_end(e._ctx, None) == INVALID and not hoff.any() and not hits.view(np.uint8).any()   # (nothing begun)
        start, ln = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        assert lib.rawdtw_seed_resident_begin(e._ctx, n, p(start), p(ln), p(hoff)) == UNSUPPORTED
        assert lib.rawdtw_seed_resident_end(e._ctx, None) == INVALID and not hoff.any()
        e.set_option(OPTION, 1)
        assert lib.rawdtw_get_option(e._ctx, OPTION.encode(), C.byref(v)) == 0 and v.value == 1
        assert lib.rawdtw_seed_begin(e._ctx, n, p(off), p(ev), p(hoff), p(hits), total) == 0
        assert lib.rawdtw_seed_end(e._ctx, None) == 0
        assert np.array_equal(hoff, want_off)
        same_hits(hits, want, "after set_option")
    finally:
        e.close()
    # a w == 0 table: the same hits with the option 0 and 1
    six0 = SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)
    want_off, want = seeding.seed_hits_host(six0, ev, off)
    e = engine(six0, on=False)
    try:
        for value in (0, 1):
            e.set_option(OPTION, value)
            got_off, got = e.seed_hits(ev, off)
            assert np.array_equal(got_off, want_off), value
            same_hits(got, want, ("w == 0", value))
    finally:
        e.close()
