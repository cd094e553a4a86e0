"""The long path of the device chaining (rawdtw_set_option "chain_long_seeds"; k_chain_sort_long and k_chain_long in
rawalign_amd/csrc/rawdtw_chain.hip): reads above k_chain's cap of 2 048 seeds, chained with their state in device memory, against the host
restatement (rawdtw_chain_anchors + rawdtw_sort_by_chaining_score) exactly as tests/test_device_chain.py compares the short path -- scores
bit for bit, positions, every anchor -- and the counters of rawdtw_chain_round_stats."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapping as M
from rawalign_amd.dtw import ANCHOR_DTYPE
from tests.test_device_chain import REC_DTYPE, SEED_DTYPE, compare, device_round, host_chains, lists_of_one_little_chain, random_read, vp, y_shaped_round

pytestmark = pytest.mark.gpu
UNSUPPORTED = 5
RING = 1024   # k_chain_long's LDS ring (kRing)
# the option sets of test_chains_of_random_reads_equal_the_host_restatement: default, narrow band, few skips, score filtering off, one chain a list
OPTION_SETS = (None, M.ChainOpt(2000, 5000, 20, 25, 2, 3, 10.0, 6, 0), M.ChainOpt(2000, 5000, 5000, 3, 2, 3, 10.0, 6, 0),
               M.ChainOpt(500, 300, 5000, 25, 2, 5, 10.0, 6, 1), M.ChainOpt(2000, 5000, 5000, 25, 4, 1, 30.0, 8, 0))


def sizes_round():
    """short and long reads interleaved: a long read first, last, and next to another one; key counts 1, 2, 5 and dup 0.05, 0.15 among both"""
    rng = np.random.default_rng(71)
    plan = [(2049, 1, 0.05), (0, 1, 0.05), (1, 2, 0.05), (2050, 2, 0.15), (4095, 5, 0.05), (63, 2, 0.15), (4096, 1, 0.15), (300, 5, 0.05),
            (4097, 2, 0.05), (5000, 5, 0.15), (2048, 2, 0.05), (8192, 1, 0.05), (300, 1, 0.15), (8193, 5, 0.15)]
    reads = [random_read(rng, n, nk, 20 * n + 200, dup=dup) if n else np.zeros(0, SEED_DTYPE) for n, nk, dup in plan]
    # the running maximum crosses the lists (rmap.cpp:431): list 0 holds a diagonal of 2 100 anchors, list 1 one of twelve, whose end scores
    # 39 -- above min_chaining_score, far below half of list 0's 6 303 -- and is a chain only to a DP that starts list 1's maximum at 0
    s = np.zeros(2112, SEED_DTYPE)
    s["target_position"][:2100], s["query_position"][:2100] = 500 + 3 * np.arange(2100), 3 * np.arange(2100)
    s["key"][2100:], s["target_position"][2100:], s["query_position"][2100:] = 1, 500 + 3 * np.arange(12), 3 * np.arange(12)
    reads.insert(5, s[rng.permutation(len(s))])
    return reads


def long_counts(per_read, cap):
    lens = [len(s) for s in per_read if len(s) > cap]
    return len(lens), sum(lens)


def test_long_and_short_reads_of_one_round_equal_the_host():
    per_read = sizes_round()
    eng = ra.Engine(0)
    try:
        eng.set_option("chain_long_seeds", 65536)
        want_reads, want_seeds = long_counts(per_read, 2048)
        assert want_reads == 9
        one_list = host_chains(eng.lib, M.default_chain_opt(6), per_read[5])
        assert len(one_list) == 1 and one_list[0][1] == 0   # (the second list's diagonal is filtered by the first list's maximum)
        for k, copt in enumerate(OPTION_SETS):
            copt = copt or M.default_chain_opt(6)
            before = eng.chain_round_stats()
            compare(eng.lib, copt, per_read, device_round(eng, copt, per_read))
            st = eng.chain_round_stats()
            assert (st["rounds"] - before["rounds"], st["long_reads"] - before["long_reads"], st["long_seeds"] - before["long_seeds"]) == (1, want_reads, want_seeds), k
    finally:
        eng.close()


def test_a_lowered_cap_routes_reads_of_61_seeds_to_the_long_path(monkeypatch):
    monkeypatch.setenv("RAWDTW_CHAIN_MAX_SEEDS", "60")
    rng = np.random.default_rng(72)
    per_read = [random_read(rng, n, 1 + k % 3, 40 * n, dup=0.1) for k, n in enumerate((60, 61, 64, 65, 127, 128, 129, 700))]
    eng = ra.Engine(0)
    try:
        eng.set_option("chain_long_seeds", 4096)
        copt = M.default_chain_opt(6)
        compare(eng.lib, copt, per_read, device_round(eng, copt, per_read))
        st = eng.chain_round_stats()
        assert (st["long_reads"], st["long_seeds"]) == (7, 61 + 64 + 65 + 127 + 128 + 129 + 700)   # (60 is k_chain's)
        # ... and every size from 1 up, each as the long path's only read (a cap of 1)
        monkeypatch.setenv("RAWDTW_CHAIN_MAX_SEEDS", "1")
        e1 = ra.Engine(0)
        try:
            e1.set_option("chain_long_seeds", 4096)
            small = [random_read(rng, n, 2, 300) for n in (1, 2, 3, 5, 17, 63)]
            compare(e1.lib, copt, small, device_round(e1, copt, small))
            assert e1.chain_round_stats()["long_reads"] == 5
        finally:
            e1.close()
    finally:
        eng.close()


def test_a_chain_that_runs_into_a_used_anchor_in_the_long_path(monkeypatch):
    monkeypatch.setenv("RAWDTW_CHAIN_MAX_SEEDS", "1")
    eng = ra.Engine(0)
    try:
        eng.set_option("chain_long_seeds", 4096)
        copt = M.default_chain_opt(6)
        per_read = y_shaped_round(eng.lib, copt)
        compare(eng.lib, copt, per_read, device_round(eng, copt, per_read))
        assert eng.chain_round_stats()["long_reads"] == 2   # (the empty read is k_chain's)
    finally:
        eng.close()


def test_the_tie_rule_in_the_long_path(monkeypatch):
    """more than 16 chains with two equal scores among them decline the round (std::sort's order is its own there), 16 are ordered as the host
    orders them, and the context goes on after the declined round"""
    monkeypatch.setenv("RAWDTW_CHAIN_MAX_SEEDS", "1")
    rng = np.random.default_rng(75)
    eng = ra.Engine(0)
    try:
        eng.set_option("chain_long_seeds", 4096)
        copt = M.default_chain_opt(6)
        assert device_round(eng, copt, [lists_of_one_little_chain(20)], n_keys=32)[0] == UNSUPPORTED
        ok16 = [lists_of_one_little_chain(16)]
        compare(eng.lib, copt, ok16, device_round(eng, copt, ok16, n_keys=32))
        plain = [random_read(rng, 100, 2, 5000)]
        compare(eng.lib, copt, plain, device_round(eng, copt, plain))
        assert eng.chain_round_stats()["long_reads"] == 3
    finally:
        eng.close()


def run_then_diagonal(rng, prefix, run=2 * RING + 128 + 324, n_prefix=300, dist=4000):
    """one list: a run of `run` (2 500) equal targets with ascending queries (every one passes over the others: rmap.cpp:458-459), then 500
    anchors on a diagonal; `prefix`: `n_prefix` anchors on a diagonal `dist` targets in front of the run, which the run's later anchors reach
    only across all the run's anchors before them -- with 2 500, far behind the ring -- and which decides their scores and, through the one
    the diagonal links to, the best chain's"""
    T = 10000
    s = np.zeros(run + 500 + (n_prefix if prefix else 0), SEED_DTYPE)
    s["target_position"][:run], s["query_position"][:run] = T, 2 * np.arange(run)
    s["target_position"][run:run + 500], s["query_position"][run:run + 500] = T + 10 + 3 * np.arange(500), 2 * run + 3 * np.arange(500)
    if prefix:
        s["target_position"][run + 500:], s["query_position"][run + 500:] = T - dist + 3 * np.arange(n_prefix), 3 * np.arange(n_prefix)
    return s[rng.permutation(len(s))]


def through_prefix_run_and_diagonal(lib, copt, read):
    t = host_chains(lib, copt, read)[0][4]["target_position"]
    return (t < 10000).sum() > 100 and (t == 10000).sum() == 1 and (t > 10000).sum() > 100


def test_candidates_beyond_the_ring_are_read_from_scratch():
    rng = np.random.default_rng(73)
    eng = ra.Engine(0)
    try:
        eng.set_option("chain_long_seeds", 65536)
        for prefix in (False, True):
            read = [run_then_diagonal(rng, prefix)]
            for band in (5000, 20, 20000):
                copt = M.ChainOpt(2000, 5000, band, 25, 2, 3, 10.0, 6, 0)
                before = eng.chain_round_stats()["far_steps"]
                compare(eng.lib, copt, read, device_round(eng, copt, read))
                far = eng.chain_round_stats()["far_steps"] - before
                print("prefix", prefix, "band", band, "far_steps", far)
                assert (far > 0) if band > RING else (far == 0), (prefix, band, far)
        # with the prefix the far candidates decide the result: the best chain runs prefix -> one anchor of the run -> diagonal
        assert through_prefix_run_and_diagonal(eng.lib, M.default_chain_opt(6), run_then_diagonal(np.random.default_rng(73), True))
        # the ring's wrap: the diagonal's first anchor links to the run's fourth from the end (the last whose query is far enough back for the
        # slope test, rmap.cpp:474).  A prefix of 321 and a run of 963 put that anchor at index 1 280, the first of a block, and the prefix's last
        # at 320: exactly the ring's reach (960) behind it, in the slot that the block's last anchor (1 343) would take in a ring one entry
        # short.  That anchor's score and predecessor come from that slot, and the best chain runs through it.
        wrap = [run_then_diagonal(rng, True, run=963, n_prefix=321, dist=1918)]
        copt = M.default_chain_opt(6)
        assert through_prefix_run_and_diagonal(eng.lib, copt, wrap[0])
        best = host_chains(eng.lib, copt, wrap[0])[0][4]
        assert int(best["query_position"][best["target_position"] == 10000][0]) == 2 * 959
        compare(eng.lib, copt, wrap, device_round(eng, copt, wrap))
        # a plain random long read never looks behind the ring
        copt = M.default_chain_opt(6)
        before = eng.chain_round_stats()["far_steps"]
        plain = [random_read(rng, 3000, 2, 60000)]
        compare(eng.lib, copt, plain, device_round(eng, copt, plain))
        assert eng.chain_round_stats()["far_steps"] == before
        # dense ties: unit steps on one diagonal (tests/test_device_chain.py's case, at 3 000 seeds)
        s = np.zeros(3000, SEED_DTYPE)
        s["target_position"] = 50 + np.arange(3000) // 2
        s["query_position"] = np.arange(3000) // 3
        ties = [s[rng.permutation(3000)]]
        compare(eng.lib, copt, ties, device_round(eng, copt, ties))
    finally:
        eng.close()


def test_what_the_device_still_declines_with_the_option_on():
    rng = np.random.default_rng(74)
    eng = ra.Engine(0)
    try:
        copt = M.default_chain_opt(6)
        eng.set_option("chain_long_seeds", 65536)
        # a long read with more than 32 chains: 40 lists with the same little chain each, and seeds without a partner to make it long
        one = np.zeros(4, SEED_DTYPE)
        one["target_position"], one["query_position"] = [100, 110, 120, 130], [5, 15, 25, 35]
        many = []
        for k in range(40):
            x = one.copy()
            x["key"] = k
            many.append(x)
        pad = np.zeros(2100, SEED_DTYPE)
        pad["key"], pad["target_position"], pad["query_position"] = 40, 10000 * np.arange(2100), 7
        big = np.concatenate(many + [pad])
        assert device_round(eng, copt, [big[rng.permutation(len(big))]], n_keys=64)[0] != 0
        # a read above the option's value declines at begin; the context goes on
        eng.set_option("chain_long_seeds", 3000)
        ok = [random_read(rng, 3000, 2, 50000), random_read(rng, 100, 2, 5000)]
        assert device_round(eng, copt, [random_read(rng, 3001, 2, 50000)] + ok)[0] == UNSUPPORTED
        compare(eng.lib, copt, ok, device_round(eng, copt, ok))
        # the option back at 0: the short cap declines as before
        eng.set_option("chain_long_seeds", 0)
        assert device_round(eng, copt, [random_read(rng, 2049, 2, 50000)] + ok[1:])[0] == UNSUPPORTED
        compare(eng.lib, copt, ok[1:], device_round(eng, copt, ok[1:]))
    finally:
        eng.close()


def test_device_arrays_of_a_round_with_long_reads_feed_the_dtw(monkeypatch):
    """6 reads, two of them above a cap lowered to just below their seed counts: d_anchors / d_ref_base / d_read_base brought home equal the host
    arrays, and rawdtw_batch_submit_device from them gives the costs of rawdtw_batch_submit from the host arrays."""
    from rawalign_amd import mapper, synth

    ref = synth.make_reference([150_000], seed=31)
    n = 6
    src = mapper.SyntheticSeeds(ref, n, seed=9, max_chunks=2)
    evs, per_read, read_base, at = [], [], np.zeros(n, np.uint32), 0
    for r in range(n):
        ev, hits = src.chunk(r, 0)
        read_base[r] = at
        at += len(ev)
        evs.append(np.asarray(ev, np.float32))
        s = np.zeros(len(hits), SEED_DTYPE)
        for k, (sq, st, t, q) in enumerate(hits):
            s[k] = (sq * 2 + (1 if st else 0), t, q)
        per_read.append(s)
    lens = sorted(len(s) for s in per_read)
    cap = lens[-3]
    assert cap >= 1 and lens[-2] > cap, lens
    monkeypatch.setenv("RAWDTW_CHAIN_MAX_SEEDS", str(cap))
    eng = ra.Engine(0)
    lib = eng.lib
    try:
        eng.set_option("chain_long_seeds", 65536)
        eng.upload_reference(ref.forward, ref.reverse)
        eng.upload_events(np.concatenate(evs))
        copt = M.default_chain_opt(6)
        key_base = np.array([eng.reference_offset(0, 0), eng.reference_offset(0, 1)], np.uint64)
        seed_off = np.zeros(n + 1, np.uint64)
        seed_off[1:] = np.cumsum([len(s) for s in per_read])
        allseeds = np.concatenate(per_read + [np.zeros(1, SEED_DTYPE)])
        cap_c = n * 32
        chain_off, anchor_off, recs = np.zeros(n + 1, np.uint64), np.zeros(cap_c + 1, np.uint64), np.zeros(cap_c, REC_DTYPE)
        anchors = np.zeros(int(seed_off[-1]) + 1, ANCHOR_DTYPE)
        d_a, d_rb, d_qb = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert lib.rawdtw_chain_round(eng._ctx, C.byref(copt), n, vp(seed_off), vp(allseeds), vp(read_base), 2, vp(key_base), vp(chain_off), vp(anchor_off), vp(recs),
                                      cap_c, vp(anchors), C.byref(d_a), C.byref(d_rb), C.byref(d_qb)) == 0
        assert eng.chain_round_stats()["long_reads"] == 2
        compare(lib, copt, per_read, (0, chain_off, anchor_off, recs, anchors, None, None, None))
        nc, na = int(chain_off[-1]), int(anchor_off[int(chain_off[-1])])
        assert nc >= n // 2
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

        def dev_array(ptr, dtype, count):
            out = np.zeros(count, dtype)
            assert hip.hipMemcpy(vp(out), ptr, out.nbytes, 2) == 0
            return out
        h_ref_base = key_base[recs["key"][:nc]].astype(np.uint64)
        h_read_base = np.repeat(read_base, np.diff(chain_off).astype(np.int64)).astype(np.uint32)
        d_anch = dev_array(d_a, ANCHOR_DTYPE, na)
        assert (d_anch["target_position"] == anchors[:na]["target_position"]).all() and (d_anch["query_position"] == anchors[:na]["query_position"]).all()
        assert (dev_array(d_rb, np.uint64, nc) == h_ref_base).all() and (dev_array(d_qb, np.uint32, nc) == h_read_base).all()
        co = ra.MapOpt().c_struct()
        out = {}
        for dev in (1, 0):
            h = C.c_void_p()
            if dev:
                st = lib.rawdtw_batch_submit_device(eng._ctx, C.byref(co), n, vp(chain_off), vp(anchor_off), d_a, d_rb, d_qb, C.byref(h))
            else:
                st = lib.rawdtw_batch_submit(eng._ctx, C.byref(co), n, vp(chain_off), vp(anchor_off), vp(anchors), vp(h_ref_base), vp(h_read_base), C.byref(h))
            assert st == 0, lib.rawdtw_last_error(eng._ctx)
            score, keep = np.zeros(nc + 1, np.float32), np.zeros(nc + 1, np.uint8)
            assert lib.rawdtw_batch_fetch_destroy(eng._ctx, h, vp(score), vp(keep)) == 0
            out[dev] = (score[:nc].copy(), keep[:nc].copy())
        assert (out[0][0].view(np.uint32) == out[1][0].view(np.uint32)).all() and (out[0][1] == out[1][1]).all()
    finally:
        eng.close()
