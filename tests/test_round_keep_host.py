"""What a round keeps as the next round's previous seeds, on the host (rawdtw_round_keep_host) -- against a plain-Python restatement on
constructed rounds (tests/round_keep_cases.py), integers and bytes; against the reference's recorded primary chains of
tests/golden/map_ref_rounds.npz in the order the mapper's write_seeds lays them down; the store's layout
(rawalign_amd/csrc/rawdtw_keep_layout.h) by a stand-alone C++ program; and the symbols and refusals that need no device.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd.dtw import NOT_KEPT, SEED_DTYPE
from tests import map_ref_cases as K
from tests import round_end_cases as R
from tests import round_keep_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")


def check_against_restatement(rd, cap, kept, soff, seeds):
    w_kept, w_lists = KC.restate(rd, cap)
    assert np.array_equal(kept, w_kept), np.nonzero(kept != w_kept)[0][:10]
    assert int(soff[0]) == 0 and len(soff) == rd.n_reads + 1
    for r, w in enumerate(w_lists):
        got = seeds[int(soff[r]):int(soff[r + 1])]
        assert len(got) == (0 if w is None else len(w)), r
        assert w is None or got.tobytes() == w.tobytes(), r
    return w_kept


@pytest.mark.parametrize("name", ["edges", "one-read", "seventy"])
def test_constructed_rounds_against_plain_python(name):
    rd = KC.rounds()[name]
    kept, soff, seeds = ra.round_keep_host(*rd.arrays(), KC.CAP)
    w = check_against_restatement(rd, KC.CAP, kept, soff, seeds)
    if name == "edges":   # the cases are what they say
        by = {e[0]: int(w[i]) for i, e in enumerate(KC.edge_reads())}
        assert by["no-chain-at-all"] == 0 and by["chains-but-no-primary"] == 0 and by["one-primary-of-one-anchor"] == 1
        assert by["two-primaries-not-in-chain-order-63-64"] == 127 and by["one-chain-of-65"] == 65 and by["one-chain-of-200"] == 200
        assert by["exactly-the-cap"] == KC.CAP and by["one-above-the-cap"] == NOT_KEPT and by["one-chain-above-the-cap"] == NOT_KEPT
        assert by["declined"] == NOT_KEPT and by["declined-with-primaries-listed"] == NOT_KEPT and by["sixty-four-primaries-of-four"] == 256
        assert by["thirty-two-primaries-shuffled"] == sum(1 + (k * 5) % 9 for k in range(32)) <= KC.CAP
    if name == "seventy":
        assert (w == NOT_KEPT).sum() >= 5 and (w == 0).sum() >= 5 and ((w > 64) & (w != NOT_KEPT)).sum() >= 5
    # counts and offsets alone (seeds_out NULL) are the same
    lib = ra.load_library()
    k2, s2 = np.zeros(rd.n_reads, np.uint32), np.zeros(rd.n_reads + 1, np.uint64)
    a = [x.ctypes.data_as(C.c_void_p) for x in rd.arrays()]
    assert lib.rawdtw_round_keep_host(rd.n_reads, *a, KC.CAP, k2.ctypes.data_as(C.c_void_p), s2.ctypes.data_as(C.c_void_p), None) == 0
    assert np.array_equal(k2, kept) and np.array_equal(s2, soff)


@pytest.mark.parametrize("cap", [1, 64, 127, 2 ** 20])
def test_the_cap_decides_alone(cap):
    rd = KC.rounds()["seventy"]
    check_against_restatement(rd, cap, *ra.round_keep_host(*rd.arrays(), cap))


@pytest.mark.parametrize("name,form", [("default", 0), ("global_full", 1), ("minanch3", 0)])
def test_the_references_primary_chains_in_write_seeds_order(name, form):
    """the fixture's rounds: the candidates' anchors laid out as a device-chained round leaves them, the round end's out / primary from
    the host restatement (which tests/test_round_end_host.py ties to the reference); what is kept must be, chain by chain, the reference's
    recorded primary chains -- sequence, strand, anchor count and the digest of the anchors -- best first, anchors in the order they lie"""
    rd, want = R.fixture_round(name, form)
    out, primary = rd.host()
    sizes = [c.n_anchors for (_, _, cands, _, _) in want for c in cands]
    anchor_off = np.zeros(len(sizes) + 1, np.uint64)
    anchor_off[1:] = np.cumsum(sizes)
    anchors = np.concatenate([np.ascontiguousarray(c.anchors, ra.ANCHOR_DTYPE) for (_, _, cands, _, _) in want for c in cands] + [np.zeros(0, ra.ANCHOR_DTYPE)])
    kept, soff, seeds = ra.round_keep_host(rd.chain_off, rd.recs, anchor_off, anchors, out, primary, 2 ** 20)
    assert not (kept == NOT_KEPT).any() and int(kept.max()) > 20
    n_chains = 0
    for i, (r, rnd, cands, chains, _) in enumerate(want):
        mine = seeds[int(soff[i]):int(soff[i + 1])]
        assert len(mine) == sum(int(ch["n_anchors"]) for ch in chains) == int(kept[i]), (r, rnd)
        at = 0
        for ch in chains:   # write_seeds: for every chain of rd.chains, for every anchor: {ref * 2 + strand, target, query}
            part = mine[at:at + int(ch["n_anchors"])]
            at += len(part)
            assert (part["key"] == int(ch["seq"]) * 2 + int(ch["strand"])).all(), (r, rnd)
            a = np.zeros(len(part), ra.ANCHOR_DTYPE)
            a["target_position"], a["query_position"] = part["target_position"], part["query_position"]
            assert bytes(K.anchors_digest(a)) == bytes(ch["digest"]), (r, rnd)
            n_chains += 1
    assert n_chains > 50   # (the fixture has a few dozen reads of several rounds: not an empty comparison)


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_keep_layout(tmp_path, flags):
    """tests/abi/keep_layout.cpp: n_slots 1 and 3 x N 1, 64 and 65 -- no two halves overlap, counts and seeds aligned, the total size"""
    exe = os.path.join(str(tmp_path), "keep_layout")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "abi", "keep_layout.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok 6", run.stdout + run.stderr


def test_symbols_and_refusals_that_need_no_device():
    lib = ra.load_library()
    for sym in ("rawdtw_chain_keep_reserve", "rawdtw_round_keep_host", "rawdtw_round_keep", "rawdtw_batch_round_end_keep", "rawdtw_batch_round_keep_fetch",
                "rawdtw_chain_kept_fetch", "rawdtw_chain_round_begin_resident_kept", "rawdtw_mapper_kept_stats"):
        assert hasattr(lib, sym), sym
    rd = KC.rounds()["one-read"]
    a = [x.ctypes.data_as(C.c_void_p) for x in rd.arrays()]
    kept, soff, seeds = np.zeros(1, np.uint32), np.zeros(2, np.uint64), np.zeros(200, SEED_DTYPE)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.rawdtw_round_keep_host(1, *a, KC.CAP, vp(kept), vp(soff), vp(seeds)) == 0
    for missing in (0, 1, 2, 4, 5):   # chain_off, recs, anchor_off, out, primary
        b = list(a)
        b[missing] = None
        assert lib.rawdtw_round_keep_host(1, *b, KC.CAP, vp(kept), vp(soff), vp(seeds)) != 0, missing
    assert lib.rawdtw_round_keep_host(1, *a, KC.CAP, None, vp(soff), vp(seeds)) != 0
    assert lib.rawdtw_round_keep_host(1, *a, KC.CAP, vp(kept), None, vp(seeds)) != 0
    b = list(a)
    b[3] = None   # kept seeds asked for, no anchors to take them from
    assert lib.rawdtw_round_keep_host(1, *b, KC.CAP, vp(kept), vp(soff), vp(seeds)) != 0
    # no read: nothing to do
    assert lib.rawdtw_round_keep_host(0, vp(np.zeros(1, np.uint64)), None, None, None, vp(rd.out), None, KC.CAP, vp(kept), vp(soff), None) == 0
    assert int(soff[0]) == 0
    # a primary index outside its read
    bad = rd.primary.copy()
    bad[0] = 3
    assert lib.rawdtw_round_keep_host(1, a[0], a[1], a[2], a[3], a[4], vp(bad), KC.CAP, vp(kept), vp(soff), vp(seeds)) != 0
    # a null context / mapper
    assert lib.rawdtw_chain_keep_reserve(None, 1, 1) != 0 and lib.rawdtw_round_keep(None, 0, *a, None, None) != 0
    assert lib.rawdtw_batch_round_end_keep(None, None, None) != 0 and lib.rawdtw_batch_round_keep_fetch(None, None, None) != 0
    assert lib.rawdtw_chain_kept_fetch(None, 0, None, 0, None) != 0 and lib.rawdtw_mapper_kept_stats(None, None, None, None, None, None) != 0
