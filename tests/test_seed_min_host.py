"""The minimizer sketch (w > 0) on the host against the reference's recorded answers on inputs with ties
(tests/golden/seed_min_ref.npz, tests/seed_min_cases.py), the checks that those inputs discriminate, and the "seed_minimizer"
option on the ABI.  No device."""
import ctypes as C
import os

import numpy as np
import pytest

from rawalign_amd import mapper, seeding
from rawalign_amd._lib import load_library
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex, SeedParams
from tests import map_ref_cases as mc
from tests import seed_cases as sc
from tests import seed_min_cases as smc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def fx():
    return smc.Fixture()


@pytest.mark.parametrize("name", smc.CASES)
def test_host_sketch_and_hits_equal_the_fixture(fx, name):
    fwd, rev, p, chunks = smc.build_case(name)
    assert sc.case_sha256(fwd, rev, chunks) == fx.sha(name)
    for c, ev in enumerate(chunks):
        h, pos = seeding.sketch(ev, p)
        wh, wp = fx.sketch(name, c)
        assert np.array_equal(h, wh) and np.array_equal(pos, wp), (name, c)
    ev, off = sc.flat(chunks)
    for threads in (1, 3):
        si = SeedIndex.from_signals(fwd, rev, p, threads=threads)
        hoff, hits = seeding.seed_hits_host(si, ev, off, threads=threads)
        assert np.array_equal(hoff, fx.hit_off(name)) and fx.check_rows(name, sc.hit_rows(hits)), (name, threads)


# ---- the inputs discriminate ------------------------------------------------------------------------------------------------------------
def emers(ev, p):
    """(hash, position of the first event) of every e-mer of a chunk under ri_sketch_min's filter: numpy and Python integers only"""
    ev = np.asarray(ev, np.float32)
    kept, last = [], 0
    for i in range(len(ev)):
        if i > 0 and abs(np.float32(ev[i] - ev[last])) < sc.DIFF:
            continue
        kept.append(i)
        last = i
    bits = ev.view(np.uint32)
    code = [(int(bits[i]) >> 30 << p.lq) | ((int(bits[i]) >> (32 - p.q)) & ((1 << p.lq) - 1)) for i in kept]
    qb, out, M = p.lq + 2, [], 0xFFFFFFFF
    for m in range(len(kept) - p.e + 1):
        k = 0
        for j in range(p.e):
            k = k << qb | code[m + j]
        k &= (1 << (qb * p.e)) - 1
        k &= M   # hash64 with the 32-bit mask (rsketch.c:6-15)
        k = (~k + (k << 21)) & M
        k ^= k >> 24
        k = (k + (k << 3) + (k << 8)) & M
        k ^= k >> 14
        k = (k + (k << 2) + (k << 4)) & M
        k ^= k >> 28
        k = (k + (k << 31)) & M
        out.append((k, kept[m]))
    return out


def window_minimum_model(ev, p):
    """OUR OWN formulation, not the reference's state machine: every e-mer that is a minimum of some full window of w e-mers, ties
    included, once, in order; with fewer than w e-mers the latest minimum."""
    em = emers(ev, p)
    if not em:
        return []
    h = np.array([x[0] for x in em], np.uint64)
    if len(h) < p.w:
        return [em[len(h) - 1 - int(np.argmin(h[::-1]))]]
    chosen = np.zeros(len(h), bool)
    for s in range(len(h) - p.w + 1):
        win = h[s:s + p.w]
        chosen[s:s + p.w] |= win == win.min()
    return [em[i] for i in np.nonzero(chosen)[0]]


def test_a_plain_window_minimum_is_not_the_references_sketch(fx):
    """The state machine of rsketch.c:193-219 is not "every minimum of a full window": the recorded sketches say so on the small
    alphabets.  (Were the two the same there, the fixture would not tell a kernel that implements the model from one that
    implements the reference.)"""
    differ = 0
    for name in smc.ALPHA_CASES:
        fwd, rev, p, chunks = smc.build_case(name)
        n = 0
        for c, ev in enumerate(chunks):
            wh, wp = fx.sketch(name, c)
            model = window_minimum_model(ev, p)
            n += [x[0] for x in model] != wh.tolist() or [x[1] for x in model] != wp.tolist()
        print(name, "chunks where the model differs:", n, "of", len(chunks))
        differ += n
    assert differ >= 10, differ


def test_a_recorded_sketch_holds_equal_hashes_inside_one_window(fx):
    found = 0
    for name in smc.ALPHA_CASES + smc.MOTIF_CASES:
        fwd, rev, p, chunks = smc.build_case(name)
        for c, ev in enumerate(chunks):
            wh, wp = fx.sketch(name, c)
            index_of = {pos: m for m, (_, pos) in enumerate(emers(ev, p))}
            m = [index_of[int(x)] for x in wp]
            for a in range(len(wh)):
                for b in range(a + 1, len(wh)):
                    if wh[a] == wh[b] and m[a] != m[b] and abs(m[a] - m[b]) < p.w:
                        found += 1
    print("pairs of equal hashes less than w e-mers apart:", found)
    assert found >= 1


def test_the_masked_event_mid_chunk_is_kept_and_coded(fx):
    """ri_sketch_min has no RI_MASK_SIGNAL test: the hits of the mask-mid-chunk case are not those of the same chunk under the w = 0
    rule's kept set (the masked value dropped, the positions behind it moved back by one)."""
    fwd, rev, p, chunks = smc.build_case("values")
    ev, at = smc.mask_mid_chunk(fwd)
    assert np.array_equal(ev.view(np.uint32), chunks[1].view(np.uint32)) and ev[at] == smc.MASK_SIGNAL
    si = SeedIndex.from_signals(fwd, rev, p, threads=2)
    _, with_mask = seeding.seed_hits_host(si, ev, np.array([0, len(ev)], np.uint64))
    dropped = np.delete(ev, at)
    _, without = seeding.seed_hits_host(si, dropped, np.array([0, len(dropped)], np.uint64))
    moved = sc.hit_rows(without)
    moved[:, 3] += (moved[:, 3] >= at).astype(np.uint32)
    rows = sc.hit_rows(with_mask)
    hoff = fx.hit_off("values")
    assert np.array_equal(rows, fx.z["values/hits"].astype(np.uint32)[int(hoff[1]):int(hoff[2])])
    assert len(rows) > 0 and not np.array_equal(rows, moved)


# ---- the option on the ABI ---------------------------------------------------------------------------------------------------------------
def test_the_option_is_documented_and_a_null_context_is_refused():
    lib = load_library()
    text = open(os.path.join(ROOT, "include", "rawdtw.h")).read()
    assert '"seed_minimizer"' in text
    assert '"seed_minimizer"' in open(os.path.join(ROOT, "README.md")).read()
    x = C.c_int64(7)
    assert lib.rawdtw_get_option(None, b"seed_minimizer", C.byref(x)) == INVALID and x.value == 7
    assert lib.rawdtw_set_option(None, b"seed_minimizer", 1) == INVALID


def test_a_mapper_without_a_context_still_refuses_a_resident_round():
    ref = mc.make_reference()
    six = SeedIndex.from_signals(ref.forward, ref.reverse, SeedParams(w=5), threads=3)
    fx = mc.Fixture(ref=ref)
    opt, copt = mc.project_opts("default", 0)
    cm = mapper.CMapper(None, opt, StopOpt(), ["seq%d" % s for s in range(len(fx.lens))], [int(x) for x in fx.lens], slot_events=2048,
                        max_reads=4, chain_opt=copt, output_chains=True, threads=2)
    try:
        ids = [cm.add_read("read_%d" % r, fx.n_chunks(r) * 4000, fx.n_chunks(r)) for r in range(2)]
        chunks = [np.ascontiguousarray(fx.chunk(r, 0)[0], np.float32) for r in range(2)]
        ev, eoff = sc.flat(chunks)
        rid = np.array(ids, np.uint32)
        vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        assert cm.lib.rawdtw_mapper_round_seeded_resident(cm._h, six._h, len(rid), vp(rid), vp(eoff), vp(ev)) == UNSUPPORTED
        assert b"seed_minimizer" in cm.lib.rawdtw_mapper_last_error(cm._h)
        assert all(cm.state(i) == (False, 0) for i in ids)
        assert cm.resident_stats() == dict(resident_rounds=0, fallback_rounds=0, hit_bytes_to_host=0, seed_bytes_to_device=0)
    finally:
        cm.close()
