"""Device chaining with "chain_max_chains" on (rawalign_amd/csrc/rawdtw_chain.hip: k_chain<true> / k_chain_long<true>, chain_order_many with
the restated std::sort of rawdtw_sort_order.h): reads with more than 32 chains, and with more than 16 of which many have equal scores, no
longer send the round back to the host -- chains, order, records and anchors equal the host's (rawdtw_chain_anchors +
rawdtw_sort_by_chaining_score, which calls std::sort itself), bit for bit, through both kernels, into the DTW batch and through the mapper.
Inputs: tests/chain_many_cases.py (checked on the host by tests/test_chain_many_cases_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from rawalign_amd import mapper
from rawalign_amd import mapping as M
from rawalign_amd.dtw import ANCHOR_DTYPE
from rawalign_amd.mapping import StopOpt
from tests import chain_many_cases as cm
from tests import map_ref_cases as mc
from tests import optins_cases as oc
from tests.test_device_chain import REC_DTYPE, SEED_DTYPE, compare, lists_of_one_little_chain, vp
from tests.test_round_keep_gpu import whole_mapper

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 5
OPTION = "chain_max_chains"


def device_round(eng, copt, per_read, n_keys, read_base=None, key_base=None):
    """tests/test_device_chain.py's device_round with out arrays for what the option allows: a chain has at least min_num_anchors anchors, so
    the round has no more than seeds / min_num_anchors (32 a read with the option off)"""
    lib, n = eng.lib, len(per_read)
    seed_off = np.zeros(n + 1, np.uint64)
    seed_off[1:] = np.cumsum([len(s) for s in per_read])
    seeds = np.concatenate(list(per_read) + [np.zeros(1, SEED_DTYPE)])
    read_base = (np.arange(n, dtype=np.uint32) * 1000).astype(np.uint32) if read_base is None else read_base
    key_base = (np.arange(n_keys, dtype=np.uint64) * 100000 + 7).astype(np.uint64) if key_base is None else key_base
    cap = max(n * 32, int(seed_off[-1]) // max(1, copt.min_num_anchors) + 1)
    chain_off, anchor_off, recs = np.zeros(n + 1, np.uint64), np.zeros(cap + 1, np.uint64), np.zeros(cap, REC_DTYPE)
    anchors = np.zeros(int(seed_off[-1]) + 1, ANCHOR_DTYPE)
    d_a, d_rb, d_qb = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st = lib.rawdtw_chain_round(eng._ctx, C.byref(copt), n, vp(seed_off), vp(seeds), vp(read_base), n_keys, vp(key_base), vp(chain_off), vp(anchor_off), vp(recs),
                                cap, vp(anchors), C.byref(d_a), C.byref(d_rb), C.byref(d_qb))
    return st, chain_off, anchor_off, recs, anchors, (d_a, d_rb, d_qb), read_base, key_base


def delta(after, before):
    return {k: after[k] - before[k] for k in after}


@pytest.fixture(scope="module")
def eng():
    e = ra.Engine(0)
    e.set_option(OPTION, 512)
    yield e
    e.close()


# ---- 1. tied lists ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [17, 20, 32, 33, 40, 64, 65, 100, 300])
def test_lists_of_equal_chains_are_ordered_as_the_host_orders_them(eng, k):
    """k chains of one score: above 16 the order is std::sort's own (not the identity), above 32 the records leave the kernels' old arrays.
    Without the option every one of these declines the round."""
    copt = M.default_chain_opt(6)
    per_read = [lists_of_one_little_chain(k)]
    before = eng.chain_order_stats()
    out = device_round(eng, copt, per_read, n_keys=k)
    assert out[0] == 0, eng.lib.rawdtw_last_error(eng._ctx)
    assert int(out[1][1]) == k and len(set(out[3]["key"][:k].tolist())) == k
    assert out[3]["key"][:k].tolist() != list(range(k))   # (the order of equal elements is not the order they came in)
    compare(eng.lib, copt, per_read, out)
    d = delta(eng.chain_order_stats(), before)
    assert (d["reads_above_32"], d["reads_ordered_restated"]) == (int(k > 32), 1) and eng.chain_order_stats()["max_chains_a_read"] >= k


# ---- 2. mixed ties ------------------------------------------------------------------------------------------------------------------------
def test_a_round_of_reads_with_many_tied_chains_among_plain_reads_equals_the_host(eng):
    copt = M.default_chain_opt(6)
    per_read = cm.mixed_round()
    cnt, _ = cm.counts(eng.lib, copt, per_read)
    assert cm.tied_above(cnt, 16) >= 30 and len(per_read) == 100
    before = eng.chain_order_stats()
    compare(eng.lib, copt, per_read, device_round(eng, copt, per_read, n_keys=cm.MIXED_KEYS))
    d = delta(eng.chain_order_stats(), before)
    assert (d["reads_above_32"], d["reads_ordered_restated"]) == (cm.above(cnt, 32), cm.above(cnt, 16))
    assert eng.chain_order_stats()["max_chains_a_read"] >= max(n for n, _ in cnt)
    # other options: one chain a list, a longer minimum (records start at seed_off / 4), score filtering off
    for copt2 in (M.ChainOpt(2000, 5000, 5000, 25, 4, 1, 10.0, 6, 0), M.ChainOpt(2000, 5000, 5000, 25, 1, 3, 5.0, 6, 1)):
        compare(eng.lib, copt2, per_read[:40], device_round(eng, copt2, per_read[:40], n_keys=cm.MIXED_KEYS))


# ---- 3. real seeding, 4. the long path -------------------------------------------------------------------------------------------------------
def test_a_round_seeded_on_48_sequences_equals_the_host(eng):
    copt = M.default_chain_opt(6)
    _, per_read = cm.seeded_round()
    cnt, _ = cm.counts(eng.lib, copt, per_read)
    assert cm.tied_above(cnt, 16) >= 20 and cm.above(cnt, 32) >= 3
    before = eng.chain_order_stats()
    compare(eng.lib, copt, per_read, device_round(eng, copt, per_read, n_keys=2 * cm.N_SEQ))
    assert delta(eng.chain_order_stats(), before)["reads_above_32"] == cm.above(cnt, 32)


def test_the_same_round_through_the_long_path(monkeypatch):
    monkeypatch.setenv("RAWDTW_CHAIN_MAX_SEEDS", "60")
    copt = M.default_chain_opt(6)
    _, per_read = cm.seeded_round()
    e = ra.Engine(0)
    try:
        e.set_option("chain_long_seeds", 4096)
        e.set_option(OPTION, 512)
        cnt, _ = cm.counts(e.lib, copt, per_read)
        compare(e.lib, copt, per_read, device_round(e, copt, per_read, n_keys=2 * cm.N_SEQ))
        st, od = e.chain_round_stats(), e.chain_order_stats()
        long_reads = [len(s) for s in per_read if len(s) > 60]
        assert (st["long_reads"], st["long_seeds"]) == (len(long_reads), sum(long_reads)) and len(long_reads) >= 50
        assert od["reads_above_32"] == cm.above(cnt, 32) >= 3 and od["reads_ordered_restated"] == cm.above(cnt, 16)
        assert od["max_chains_a_read"] == max(n for n, _ in cnt)
        # the constructed round too: its reads of many little lists are long under this cap, its plain reads on either side of it
        mixed = cm.mixed_round()[:40]
        compare(e.lib, copt, mixed, device_round(e, copt, mixed, n_keys=cm.MIXED_KEYS))
    finally:
        e.close()


# ---- 5. what still declines ------------------------------------------------------------------------------------------------------------------
def test_what_still_declines_and_the_options_range():
    copt = M.default_chain_opt(6)
    e = ra.Engine(0)
    try:
        lib = e.lib
        for bad in (-1, 4097):
            assert lib.rawdtw_set_option(e._ctx, OPTION.encode(), bad) == INVALID
            assert e.get_option(OPTION) == 0
        for good in (1, 4096, 0):
            e.set_option(OPTION, good)
            assert e.get_option(OPTION) == good
        # the option off: 20 tied lists decline, as they always have
        assert device_round(e, copt, [lists_of_one_little_chain(20)], n_keys=64)[0] == UNSUPPORTED
        assert e.chain_order_stats() == dict(reads_above_32=0, reads_ordered_restated=0, max_chains_a_read=0)
        # 40: a read of 40 tied chains is chained, one of 41 declines the round; the context goes on
        e.set_option(OPTION, 40)
        plain = lists_of_one_little_chain(3)
        ok = [plain, lists_of_one_little_chain(40)]
        compare(lib, copt, ok, device_round(e, copt, ok, n_keys=64))
        assert device_round(e, copt, [plain, lists_of_one_little_chain(41)], n_keys=64)[0] == UNSUPPORTED
        assert OPTION in lib.rawdtw_last_error(e._ctx).decode()
        compare(lib, copt, ok, device_round(e, copt, ok, n_keys=64))
        assert e.chain_order_stats() == dict(reads_above_32=2, reads_ordered_restated=2, max_chains_a_read=40)   # (the declined round is not counted)
        # 1: one chain a read
        e.set_option(OPTION, 1)
        one = [lists_of_one_little_chain(1), np.zeros(0, SEED_DTYPE)]
        compare(lib, copt, one, device_round(e, copt, one, n_keys=64))
        assert device_round(e, copt, [lists_of_one_little_chain(2)], n_keys=64)[0] == UNSUPPORTED
        # 4 096, the largest: 500 lists of one chain (2 000 seeds, k_chain's largest read but 48)
        e.set_option(OPTION, 4096)
        big = [lists_of_one_little_chain(500), plain]
        compare(lib, copt, big, device_round(e, copt, big, n_keys=512))
    finally:
        e.close()


# ---- 6. into the DTW -------------------------------------------------------------------------------------------------------------------------
def test_the_dtw_batch_from_the_devices_many_chains_equals_the_batch_from_host_arrays(eng):
    """tests/test_device_chain.py::test_the_dtw_batch_straight_from_the_devices_chains_equals_the_batch_from_host_arrays on the seeded round:
    rawdtw_batch_submit_device on the arrays the compaction left against rawdtw_batch_submit of the host copies, sparse + banded"""
    lib, copt, ref = eng.lib, M.default_chain_opt(6), cm.reference()
    reads, per_read = cm.seeded_round()
    n = len(reads)
    eng.upload_reference(ref.forward, ref.reverse)
    eng.upload_events(np.concatenate(reads))
    read_base = (np.arange(n, dtype=np.uint32) * 400).astype(np.uint32)
    key_base = np.array([eng.reference_offset(k >> 1, k & 1) for k in range(2 * cm.N_SEQ)], np.uint64)
    st, chain_off, anchor_off, recs, anchors, (d_a, d_rb, d_qb), _, _ = device_round(eng, copt, per_read, 2 * cm.N_SEQ, read_base, key_base)
    assert st == 0, lib.rawdtw_last_error(eng._ctx)
    nc = int(chain_off[-1])
    assert int(np.diff(chain_off).max()) > 32
    h_ref_base = key_base[recs["key"][:nc]].astype(np.uint64)
    h_read_base = np.repeat(read_base, np.diff(chain_off).astype(np.int64)).astype(np.uint32)
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
    assert out[1][1].sum() > 0


# ---- 7. the mapper ---------------------------------------------------------------------------------------------------------------------------
def mapper_run(options, device_chain, resident, stop):
    """map_reads_c over chain_many_cases.mapper_reads on an engine of its own: (lines, log, rounds, the counters)"""
    ref, si, src = cm.reference(), cm.seed_index(), cm.mapper_reads()
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        for k, v in options.items():
            e.set_option(k, v)
        opt, copt = mc.whole_project_opts("default", 0)
        c = whole_mapper(e, src, opt, copt, stop) if device_chain else mapper.CMapper(
            e, opt, stop, ["seq%d" % s for s in range(cm.N_SEQ)], [cm.SEQ_LEN] * cm.N_SEQ, slot_events=4096, max_reads=src.n_reads, chain_opt=copt,
            output_chains=True, threads=3, carry=False, groups=1, device_chain=False)
        lines, rounds = mapper.map_reads_c(src, list(range(src.n_reads)), c, seed_index=si, resident=resident)
        out = dict(lines=lines, log=c.log(), rounds=rounds, anchor_bytes=c.timing()["anchor_bytes"], resident=c.resident_stats(), round_end=c.round_end_stats(),
                   kept=c.kept_stats(), chain=e.chain_round_stats(), order=e.chain_order_stats())
        c.close()
        return out
    finally:
        e.close()


@pytest.mark.parametrize("stop", ["never", "default"])
def test_the_mapper_keeps_its_rounds_on_the_device(stop):
    """24 reads of three chunks on 48 sequences.  A mapper that chains on the device with the option on gives the lines and the log of one that
    chains on the host, and sends no anchor list up (rawdtw_mapper_timing's slot 5: what a round chained on the host hands to the device); with the
    option off the same reads do fall back.  Resident rounds with every other opt-in on: no fall-back round, every read ended and kept on the
    device (the fixture's reads have at most 64 chains: tests/test_chain_many_cases_cpu.py)."""
    mk = oc.never if stop == "never" else StopOpt
    host = mapper_run({}, False, False, mk())
    assert sum("\tnc:i:0" not in ln for ln in host["lines"]) >= 12 and host["anchor_bytes"] > 0
    on = mapper_run({OPTION: 512}, True, False, mk())
    assert on["lines"] == host["lines"] and on["log"] == host["log"] and on["rounds"] == host["rounds"]
    assert on["anchor_bytes"] == 0 and on["chain"]["rounds"] == on["rounds"]
    assert on["order"]["reads_above_32"] >= 1 and 32 < on["order"]["max_chains_a_read"] <= 64
    off = mapper_run({}, True, False, mk())
    assert off["lines"] == host["lines"] and off["anchor_bytes"] > 0   # (the fixture does decline without the option)
    res = mapper_run(dict(oc.ALL_ON, **{OPTION: 512}), True, True, mk())
    print(stop, res["resident"], res["round_end"], res["kept"], res["order"])
    assert res["lines"] == host["lines"] and res["rounds"] == host["rounds"]
    assert res["resident"]["fallback_rounds"] == 0 and res["resident"]["resident_rounds"] == res["rounds"] and res["resident"]["hit_bytes_to_host"] == 0
    assert res["round_end"]["rounds"] == res["rounds"] and res["round_end"]["reads_declined"] == 0 and res["round_end"]["reads_device"] > 0
    assert res["kept"]["reads_not_kept"] == 0 and res["kept"]["reads_from_host"] == 0
    assert res["order"] == on["order"]
    res_off = mapper_run(oc.ALL_ON, True, True, mk())
    assert res_off["lines"] == host["lines"] and res_off["resident"]["fallback_rounds"] >= 1
