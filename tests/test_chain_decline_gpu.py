"""Device chaining with "chain_decline_reads" on (rawalign_amd/csrc/rawdtw_chain.hip: k_chain_scan<true>, k_chain_compact<true>,
k_declined_seeds; rawdtw_chain_round_declined / _declined_seeds / _append): a read the device cannot chain is declined alone, the rest of its
round is chained on the device as before, and the host's chains of the declined reads join the round's batch in device memory.  The prediction
is rawdtw_chain_decline_host; the chains are compared with the host restatement (rawdtw_chain_anchors + rawdtw_sort_by_chaining_score) bit for
bit.  Inputs: tests/chain_decline_cases.py (checked on the host by tests/test_chain_decline_cases_cpu.py).  Every test here sets the option,
which the library before it refuses."""
import ctypes as C

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from oracle.loader import Oracle, OrcOpt
from rawalign_amd import mapping as M
from rawalign_amd import seeding
from rawalign_amd.dtw import ANCHOR_DTYPE
from tests import chain_decline_cases as dc
from tests import chain_many_cases as cm
from tests import map_ref_cases as mc
from tests import seed_cases as sc
from tests.test_device_chain import REC_DTYPE, SEED_DTYPE, host_chains, vp
from tests.test_resident_round_gpu import place_in_arena, seeds_of

pytestmark = pytest.mark.gpu
INVALID, RANGE, UNSUPPORTED = 1, 4, 5
OPTION = "chain_decline_reads"


@pytest.fixture(scope="module")
def eng():
    """an engine under the lowered cap on seeds a read (read at rawdtw_create), with the option on"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RAWDTW_CHAIN_MAX_SEEDS", str(dc.SEED_CAP))
        e = ra.Engine(0)
    e.set_option(OPTION, 1)
    yield e
    e.close()


def dev_array(ptr, dtype, count):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(max(count, 1), dtype)
    if count:
        assert hip.hipMemcpy(vp(out), ptr, count * out.itemsize, 2) == 0
    return out[:count]


class Round:
    """rawdtw_chain_round_begin + _end over per_read, with out arrays that hold what the round can have: seeds / min_num_anchors chains"""

    def __init__(self, eng, copt, per_read, n_keys=dc.N_KEYS, read_base=None, key_base=None):
        self.eng, self.copt, self.per_read, n = eng, copt, per_read, len(per_read)
        self.n = n
        self.seed_off = np.zeros(n + 1, np.uint64)
        self.seed_off[1:] = np.cumsum([len(s) for s in per_read])
        self.seeds = np.concatenate(list(per_read) + [np.zeros(1, SEED_DTYPE)])
        self.read_base = (np.arange(n, dtype=np.uint32) * 1000 + 3).astype(np.uint32) if read_base is None else read_base
        self.key_base = (np.arange(n_keys, dtype=np.uint64) * 100000 + 7).astype(np.uint64) if key_base is None else key_base
        self.cap = max(n * 32, int(self.seed_off[-1]) // max(1, copt.min_num_anchors) + 1)
        self.chain_off, self.anchor_off = np.zeros(n + 1, np.uint64), np.zeros(self.cap + 1, np.uint64)
        self.recs, self.anchors = np.zeros(self.cap, REC_DTYPE), np.zeros(int(self.seed_off[-1]) + 1, ANCHOR_DTYPE)
        self.dev = [C.c_void_p() for _ in range(3)]
        lib = eng.lib
        self.st = lib.rawdtw_chain_round_begin(eng._ctx, C.byref(copt), n, vp(self.seed_off), vp(self.seeds), vp(self.read_base), len(self.key_base),
                                               vp(self.key_base), vp(self.chain_off), vp(self.anchor_off), vp(self.recs), self.cap, vp(self.anchors))
        if self.st == 0:
            self.st = lib.rawdtw_chain_round_end(eng._ctx, *[C.byref(x) for x in self.dev])
        self.error = lib.rawdtw_last_error(eng._ctx).decode()

    def chains_of(self, r, ext=None):
        """read r's chains as comparable tuples, from the host arrays and the three device arrays; ext: after an append, (chain_off_ext,
        anchor_off_ext, recs, anchors) with the appended chains behind the round's"""
        co, ao, recs, anchors = (self.chain_off, self.anchor_off, self.recs, self.anchors) if ext is None else ext
        nc = int(co[-1])
        na = int(ao[nc])
        d_anch, d_refb, d_rbc = dev_array(self.dev[0], ANCHOR_DTYPE, na), dev_array(self.dev[1], np.uint64, nc), dev_array(self.dev[2], np.uint32, nc)
        out = []
        for c in range(int(co[r]), int(co[r + 1])):
            a0, a1 = int(ao[c]), int(ao[c + 1])
            assert anchors[a0:a1].tobytes() == d_anch[a0:a1].tobytes(), (r, c)
            out.append((recs[c].tobytes(), anchors[a0:a1].tobytes(), int(d_refb[c]), int(d_rbc[c])))
        return out

    def append(self, app):
        """rawdtw_chain_round_append of host_append_arrays' chains: chains_of's `ext`, and the device pointers"""
        nc0 = int(self.chain_off[-1])
        na0 = int(self.anchor_off[nc0])
        ext, aext, dev = self.eng.chain_round_append(self.n, nc0, *app)
        nca = int(app[0][-1])
        assert aext[:nc0 + 1].tobytes() == self.anchor_off[:nc0 + 1].tobytes() and int(aext[-1]) == na0 + int(app[2][-1])
        return (ext, aext, np.concatenate([self.recs[:nc0], app[1][:nca]]), np.concatenate([self.anchors[:na0], app[3]])), dev


def want_chains(lib, copt, seeds, read_base, key_base):
    """the host restatement of a read's chains, in Round.chains_of's form"""
    out = []
    for score, key, start, end, an in host_chains(lib, copt, seeds):
        rec = np.zeros(1, REC_DTYPE)
        rec[0] = (score, key, start, end, len(an))
        a = np.zeros(len(an), ANCHOR_DTYPE)
        a["target_position"], a["query_position"] = an["target_position"], an["query_position"]
        out.append((rec.tobytes(), a.tobytes(), int(key_base[key]), int(read_base)))
    return out


def host_append_arrays(lib, copt, per_read, reads):
    """the declined reads' chains as rawdtw_chain_round_append takes them: chain_off and anchor_off from 0, records, anchors end-first"""
    chain_off, anchor_off, recs, anchors = [0], [0], [], []
    for r in reads:
        for score, key, start, end, an in host_chains(lib, copt, per_read[r]):
            recs.append((score, key, start, end, len(an)))
            a = np.zeros(len(an), ANCHOR_DTYPE)
            a["target_position"], a["query_position"] = an["target_position"], an["query_position"]
            anchors.append(a)
            anchor_off.append(anchor_off[-1] + len(an))
        chain_off.append(len(recs))
    return (np.array(chain_off, np.uint64), np.array(recs, REC_DTYPE) if recs else np.zeros(1, REC_DTYPE), np.array(anchor_off, np.uint64),
            np.concatenate(anchors + [np.zeros(1, ANCHOR_DTYPE)]))


# ---- 1. the round-level case ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("many", [0, dc.MANY])
@pytest.mark.parametrize("order", ["given", "rotated", "reversed"])
def test_a_read_is_declined_alone_and_the_rest_is_chained_on_the_device(eng, order, many):
    copt, lib = M.default_chain_opt(6), eng.lib
    reads = dc.round_reads()
    idx = dc.orders()[order]
    per_read = [reads[i] for i in idx]
    eng.set_option("chain_max_chains", many)
    try:
        why, _ = ra.chain_decline_host(copt, per_read, dc.SEED_CAP, 0, many)
        assert {idx[r]: int(w) for r, w in enumerate(why) if w} == dc.DECLINED[many]
        rd = Round(eng, copt, per_read)
        assert rd.st == 0, rd.error
        got_reads, got_why = eng.chain_round_declined()
        want_reads = np.flatnonzero(why)
        print(order, many, got_reads.tolist(), got_why.tolist())
        assert got_reads.tolist() == want_reads.tolist() and got_why.tolist() == why[want_reads].tolist()
        assert (why[0] != 0) == (order == "rotated") and (why[-1] != 0) == (order == "reversed")
        kept = [r for r in range(len(per_read)) if not why[r]]
        mine = [rd.chains_of(r) for r in kept]   # (before the next round takes the workspace)
        alone = Round(eng, copt, [per_read[r] for r in kept], read_base=rd.read_base[kept].copy())
        assert alone.st == 0 and len(eng.chain_round_declined()[0]) == 0
        n_chains = 0
        for k, r in enumerate(kept):
            got = mine[k]
            assert got == want_chains(lib, copt, per_read[r], rd.read_base[r], rd.key_base), (order, many, r)
            assert got == alone.chains_of(k), (order, many, r)
            n_chains += len(got)
        for r in want_reads:
            assert rd.chain_off[r] == rd.chain_off[r + 1], r
        assert n_chains == int(rd.chain_off[-1]) > 0
    finally:
        eng.set_option("chain_max_chains", 0)


# ---- 2. everybody declines, 3. nobody does -----------------------------------------------------------------------------------------------------
def test_a_round_of_reads_above_the_cap_is_appended_whole(eng):
    copt, lib = M.default_chain_opt(6), eng.lib
    per_read = dc.all_above()
    n = len(per_read)
    rd = Round(eng, copt, per_read)
    assert rd.st == 0, rd.error
    got_reads, got_why = eng.chain_round_declined()
    assert got_reads.tolist() == list(range(n)) and got_why.tolist() == [1] * n
    assert not rd.chain_off.any() and rd.anchor_off[0] == 0
    ext, dev = rd.append(host_append_arrays(lib, copt, per_read, range(n)))
    assert [x.value for x in dev] == [x.value for x in rd.dev]
    assert not ext[0][:n + 1].any() and int(ext[0][-1]) > 0
    for j in range(n):
        assert rd.chains_of(n + j, ext) == want_chains(lib, copt, per_read[j], rd.read_base[j], rd.key_base), j


def test_a_round_nobody_declines_is_the_round_with_the_option_off(eng):
    copt = M.default_chain_opt(6)
    per_read = dc.none_above()
    on = Round(eng, copt, per_read)
    assert on.st == 0 and len(eng.chain_round_declined()[0]) == 0
    on_dev = [on.chains_of(r) for r in range(on.n)]
    ext, _ = on.append((np.zeros(1, np.uint64), np.zeros(1, REC_DTYPE), np.zeros(1, np.uint64), np.zeros(1, ANCHOR_DTYPE)))
    assert ext[0].tobytes() == on.chain_off.tobytes()   # (nothing to append: the batch's read list is the round's)
    eng.set_option(OPTION, 0)
    try:
        off = Round(eng, copt, per_read)
        assert off.st == 0 and len(eng.chain_round_declined()[0]) == 0
        for name in ("chain_off", "anchor_off", "recs", "anchors"):
            assert getattr(on, name).tobytes() == getattr(off, name).tobytes(), name
        assert on_dev == [off.chains_of(r) for r in range(off.n)] and int(on.chain_off[-1]) > 16
    finally:
        eng.set_option(OPTION, 1)


# ---- 4. the declined reads' seeds, from a resident round ---------------------------------------------------------------------------------------
def test_the_declined_reads_seeds_of_a_resident_round_come_home():
    """rawdtw_chain_round_begin_resident lays the seed list down on the device (previous anchors from the host, hits from the resident seeding);
    k_declined_seeds brings home the stretches of the reads above a cap of 150 seeds: as multisets, what the host computes for them"""
    rng = np.random.default_rng(45)
    ref = mc.make_reference()
    six = seeding.SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)
    fx = mc.Fixture(ref=ref)
    chunks = [np.ascontiguousarray(fx.events[int(fx.ev_off[k]):int(fx.ev_off[k + 1])]) for k in range(0, 40)]
    n, cap_seeds = len(chunks), 150
    copt = M.default_chain_opt(mc.E)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RAWDTW_CHAIN_MAX_SEEDS", str(cap_seeds))
        e = ra.Engine(0)
    lib = e.lib
    try:
        e.set_option(OPTION, 1)
        e.upload_seed_index(six)
        start, ln = place_in_arena(e, chunks, rng)
        ev, off = sc.flat(chunks)
        hoff, hits = seeding.seed_hits_host(six, ev, off, threads=8)
        hoff = hoff.astype(np.int64)
        sits = np.zeros(n, np.uint8)
        sits[[3, n - 1]] = 1
        chunk_start = rng.integers(0, 3000, n).astype(np.uint32)
        prev = []
        for r in range(n):
            k = 0 if sits[r] or r % 3 == 0 else int(rng.integers(1, 60))
            p = np.zeros(k, SEED_DTYPE)
            p["key"], p["target_position"], p["query_position"] = rng.integers(0, 6, k), rng.integers(0, 6000, k), rng.integers(0, 3000, k)
            prev.append(p)
        per_read = [np.zeros(0, SEED_DTYPE) if sits[r] else np.concatenate([prev[r], seeds_of(hits[hoff[r]:hoff[r + 1]], chunk_start[r])]) for r in range(n)]
        why, _ = ra.chain_decline_host(copt, per_read, cap_seeds, 0, 0)
        want_reads = np.flatnonzero(why)
        assert 2 <= len(want_reads) < n // 2 and set(why[want_reads].tolist()) == {1}, why.tolist()
        seed_off = np.concatenate([[0], np.cumsum([len(s) for s in per_read])]).astype(np.uint64)
        prev_off = np.concatenate([[0], np.cumsum([len(p) for p in prev])]).astype(np.uint64)
        prev_all = np.concatenate(prev + [np.zeros(1, SEED_DTYPE)])
        read_base = (np.arange(n, dtype=np.uint32) * 1000).astype(np.uint32)
        key_base = (np.arange(6, dtype=np.uint64) * 100000 + 7).astype(np.uint64)
        cap = max(n * 32, int(seed_off[-1]) // 2 + 1)
        got = np.zeros(n + 1, np.uint64), np.zeros(cap + 1, np.uint64), np.zeros(cap, REC_DTYPE), np.zeros(int(seed_off[-1]) + 1, ANCHOR_DTYPE)
        d = [C.c_void_p() for _ in range(3)]
        rs = e.seed_resident(start, ln)
        assert np.array_equal(rs.hit_off.astype(np.int64), hoff)
        st = lib.rawdtw_chain_round_begin_resident(e._ctx, C.byref(copt), n, vp(seed_off), vp(prev_off), vp(prev_all), vp(chunk_start), vp(sits),
                                                   vp(read_base), 6, vp(key_base), vp(got[0]), vp(got[1]), vp(got[2]), cap, vp(got[3]))
        assert st == 0, lib.rawdtw_last_error(e._ctx)
        assert lib.rawdtw_chain_round_end(e._ctx, *[C.byref(x) for x in d]) == 0, lib.rawdtw_last_error(e._ctx)
        got_reads, got_why = e.chain_round_declined()
        assert got_reads.tolist() == want_reads.tolist() and got_why.tolist() == [1] * len(want_reads)
        soff, seeds = e.chain_round_declined_seeds()
        assert soff.tolist() == np.concatenate([[0], np.cumsum([len(per_read[r]) for r in want_reads])]).tolist()
        for j, r in enumerate(want_reads):
            mine = seeds[int(soff[j]):int(soff[j + 1])]
            assert np.array_equal(np.sort(mine, order=SEED_DTYPE.names), np.sort(per_read[r], order=SEED_DTYPE.names)), r
        # an array that is too small: RAWDTW_ERR_RANGE, the offsets filled
        small_off, small = np.zeros(len(want_reads) + 1, np.uint64), np.zeros(int(soff[-1]), SEED_DTYPE)
        assert lib.rawdtw_chain_round_declined_seeds(e._ctx, vp(small_off), vp(small), int(soff[-1]) - 1) == RANGE
        assert small_off.tolist() == soff.tolist() and not small["target_position"].any()
        # the reads the device chained equal the round fed the host-built list
        for r in range(n):
            if not why[r]:
                want = host_chains(lib, copt, per_read[r])
                assert int(got[0][r + 1] - got[0][r]) == len(want), r
    finally:
        e.close()


# ---- 5. append, then the DTW -------------------------------------------------------------------------------------------------------------------
SEEDED_CAP = 850   # of the seeded round's 60 reads (476 .. 973 seeds) eight are above it; others decline for 33 .. 36 chains and for ties above 16


@pytest.fixture
def eng850():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RAWDTW_CHAIN_MAX_SEEDS", str(SEEDED_CAP))
        e = ra.Engine(0)
    e.set_option(OPTION, 1)
    yield e
    e.close()


def test_the_batch_over_the_appended_round_equals_the_oracles_loop(eng850):
    """the seeded round of tests/chain_many_cases.py under the default caps on chains and 850 seeds a read: the device's chains and the host's
    chains of the declined reads as ONE batch (rawdtw_batch_submit_device over the extended read list), every chain's score and keep against
    the oracle's sequential align_chain loop (rmap.cpp:248-293, 515-524)"""
    eng = eng850
    lib, copt, ref = eng.lib, M.default_chain_opt(6), cm.reference()
    reads, per_read = cm.seeded_round()
    n = len(reads)
    why, _ = ra.chain_decline_host(copt, per_read, SEEDED_CAP, 0, 0)
    n_chains = np.array([len(host_chains(lib, copt, s)) for s in per_read])
    declined = np.flatnonzero(why)
    print("declined", len(declined), "of", n, "reasons", sorted(set(why[declined].tolist())))
    assert {1, 4, 6} <= set(why.tolist()) and sum(1 for r in range(n) if not why[r] and n_chains[r]) >= 20
    eng.upload_reference(ref.forward, ref.reverse)
    events = np.concatenate(reads)
    eng.upload_events(events)
    read_base = (np.arange(n, dtype=np.uint32) * 400).astype(np.uint32)
    key_base = np.array([eng.reference_offset(k >> 1, k & 1) for k in range(2 * cm.N_SEQ)], np.uint64)
    rd = Round(eng, copt, per_read, 2 * cm.N_SEQ, read_base, key_base)
    assert rd.st == 0, rd.error
    assert eng.chain_round_declined()[0].tolist() == declined.tolist()
    app = host_append_arrays(lib, copt, per_read, declined)
    spare = np.zeros(2 * n + 2, np.uint64), np.zeros(int(n_chains.sum()) + 2, np.uint64)
    assert lib.rawdtw_chain_round_append(eng._ctx, len(declined) + 1, vp(app[0]), vp(app[1]), vp(app[2]), vp(app[3]), vp(spare[0]), vp(spare[1]),
                                         *[C.byref(x) for x in rd.dev]) == INVALID   # (another number of reads than the round declined)
    (ext, aext, recs, anchors), dev = rd.append(app)
    assert lib.rawdtw_chain_round_append(eng._ctx, len(declined), vp(app[0]), vp(app[1]), vp(app[2]), vp(app[3]), vp(spare[0]), vp(spare[1]),
                                         *[C.byref(x) for x in rd.dev]) == INVALID   # (once a round)
    nr, nc = n + len(declined), int(ext[-1])
    assert nc == int(n_chains.sum()) and int(rd.chain_off[-1]) < nc
    opt = ra.MapOpt()
    co, h = opt.c_struct(), C.c_void_p()
    assert lib.rawdtw_batch_submit_device(eng._ctx, C.byref(co), nr, vp(ext), vp(aext), *dev, C.byref(h)) == 0, lib.rawdtw_last_error(eng._ctx)
    score, keep = np.zeros(nc + 1, np.float32), np.zeros(nc + 1, np.uint8)
    assert lib.rawdtw_batch_fetch_destroy(eng._ctx, h, vp(score), vp(keep)) == 0
    orc = Oracle()
    oopt = OrcOpt(1, 1, opt.dtw_band_radius_frac, opt.dtw_match_bonus, opt.dtw_min_score, 1)
    arena = {int(key_base[k]): (ref.forward if k & 1 else ref.reverse)[k >> 1] for k in range(2 * cm.N_SEQ)}   # (strand 1 selects forward_signals, rmap.cpp:183-188)
    owner = list(range(n)) + declined.tolist()
    kept = 0
    for p in range(nr):
        assert (int(ext[p + 1]) > int(ext[p])) == (n_chains[owner[p]] > 0 and (p >= n) == bool(why[owner[p]])), p
        best = np.float32(0.0)
        for c in range(int(ext[p]), int(ext[p + 1])):
            a = anchors[int(aext[c]):int(aext[c + 1])]
            want = orc.align_chain(a, arena[int(key_base[recs[c]["key"]])], events[int(read_base[owner[p]]):], oopt, float(best))
            assert score[c].view(np.uint32) == np.float32(want).view(np.uint32), (p, c, score[c], want)
            k = want >= np.float32(opt.dtw_min_score)
            assert bool(keep[c]) == bool(k)
            kept += bool(k)
            if k and want > best:
                best = want
    assert kept > 0
    # a new round takes the workspace: the ended round can no longer be appended to
    again = Round(eng, copt, per_read, 2 * cm.N_SEQ, read_base, key_base)
    assert again.st == 0
    rb = lib.rawdtw_chain_round_begin(eng._ctx, C.byref(copt), n, vp(again.seed_off), vp(again.seeds), vp(read_base), len(key_base), vp(key_base),
                                      vp(again.chain_off), vp(again.anchor_off), vp(again.recs), again.cap, vp(again.anchors))
    assert rb == 0
    assert lib.rawdtw_chain_round_append(eng._ctx, len(declined), vp(app[0]), vp(app[1]), vp(app[2]), vp(app[3]), vp(spare[0]), vp(spare[1]),
                                         *[C.byref(x) for x in again.dev]) == INVALID
    assert lib.rawdtw_chain_round_end(eng._ctx, *[C.byref(x) for x in again.dev]) == 0


# ---- 10. the option, and the option off ----------------------------------------------------------------------------------------------------------
def test_the_options_values_and_the_refusals_with_it_off(eng):
    copt, lib = M.default_chain_opt(6), eng.lib
    for bad in (-1, 2, 7):
        assert lib.rawdtw_set_option(eng._ctx, OPTION.encode(), bad) == INVALID and eng.get_option(OPTION) == 1
    eng.set_option(OPTION, 0)
    try:
        assert eng.get_option(OPTION) == 0
        for many, per_read, words in ((0, dc.all_above(), "more seeds than the device chains (2048)"),
                                      (0, [dc.thirty_three_chains()], "more than 16 chains, two of them with equal scores"),
                                      (dc.MANY, [dc.thirty_three_chains()], "more chains than \"chain_max_chains\" allows")):
            eng.set_option("chain_max_chains", many)
            rd = Round(eng, copt, per_read)
            assert rd.st == UNSUPPORTED and words in rd.error and "chain this round on the host" in rd.error, rd.error
            assert len(eng.chain_round_declined()[0]) == 0
            assert lib.rawdtw_chain_round_declined_seeds(eng._ctx, vp(np.zeros(4, np.uint64)), None, 0) == INVALID
    finally:
        eng.set_option("chain_max_chains", 0)
        eng.set_option(OPTION, 1)


# ---- 6 .. 9. the mapper --------------------------------------------------------------------------------------------------------------------
from rawalign_amd import mapper  # noqa: E402
from rawalign_amd.mapping import StopOpt  # noqa: E402
from rawalign_amd.seeding import SeedIndex  # noqa: E402
from tests import optins_cases as oc  # noqa: E402
from tests.test_optins_together_gpu import NO_KEPT, _Watched, _Windows, delta  # noqa: E402
from tests.test_rawsig_host import raw_batch  # noqa: E402
from tests.test_round_keep_gpu import drive, whole_mapper  # noqa: E402
from tests.test_signal_round_gpu import FLOW_CHUNKS, FLOW_READS, flow  # noqa: E402,F401  (flow: the fixture itself)

CAP = "RAWDTW_CHAIN_MAX_SEEDS"
DECLINE_ON = dict(device_round_end=1, resident_chains=4096, **{OPTION: 1})   # ("chain_long_seeds" stays off: with it on no read of these cases is above a cap)


@pytest.fixture(scope="module")
def ref():
    return mc.make_reference()


@pytest.fixture(scope="module")
def six(ref):
    return SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)


@pytest.fixture(scope="module")
def raw_reads():
    raws = mc.make_raw_reads()
    assert mc.raw_sha256(raws) == np.load(mc.READS)["raw_sha256"].tobytes(), "synth.make_genome_raw_reads or tests/map_ref_cases.py drifted"
    return raws


def driven(ref_, si, wr, reads, options, stop, signal=False, cap=None):
    """tests/test_round_keep_gpu.py's drive (every round resident) on an engine of its own, created under the cap: lines, per round the resident
    and the kept stats' increase, and the totals with rawdtw_mapper_decline_stats"""
    with pytest.MonkeyPatch.context() as mp:
        if cap is not None:
            mp.setenv(CAP, str(cap))
        e = ra.Engine(0)
    try:
        e.upload_reference(ref_.forward, ref_.reverse)
        for k, v in options.items():
            e.set_option(k, v)
        opt, copt = mc.whole_project_opts("default", 0)
        cm = _Watched(whole_mapper(e, wr, opt, copt, stop), signal)
        lines, kept, _ = drive(cm, reads, si, lambda k: True)
        out = dict(lines=lines, rounds=list(zip(cm.res, [d for _, d in kept])), resident=cm.resident_stats(), kept=cm.kept_stats(), decline=cm.decline_stats(),
                   round_end=cm.round_end_stats())
        cm.close()
        return out
    finally:
        e.close()


def check_resident_declines(on, case):
    """what the host says a run must have counted (tests/chain_decline_cases.py, pinned by tests/test_chain_decline_cases_cpu.py)"""
    dcl = case["declined"]
    assert on["resident"]["fallback_rounds"] == 0 and on["resident"]["hit_bytes_to_host"] == 0 and on["resident"]["resident_rounds"] == len(dcl)
    assert all(d["fallback_rounds"] == 0 and d["resident_rounds"] == 1 for d, _ in on["rounds"])
    assert on["decline"] == dict(rounds_with_declines=sum(1 for d in dcl if d), reads_declined_seeds=case["by_seeds"], reads_declined_chains=case["by_chains"],
                                 reads_chained_device=case["chained_device"], seed_bytes_to_host=12 * case["declined_seeds"])
    assert on["round_end"]["reads_device"] + on["round_end"]["reads_declined"] == case["pairs"] and on["round_end"]["reads_declined"] == 0
    for k, (_, kd) in enumerate(on["rounds"]):
        assert kd == dict(reads_from_device=case["from_device"][k][0], seeds_from_device=case["from_device"][k][1], reads_from_host=case["from_host"][k][0],
                          seeds_from_host=case["from_host"][k][1], reads_not_kept=len(dcl[k])), (k, kd)
    assert on["resident"]["seed_bytes_to_device"] == 12 * sum(s for _, s in case["from_host"])


@pytest.mark.parametrize("case", ["whole_fb", "whole_default"])
def test_whole_reads_from_signal_decline_a_read_and_stay_resident(ref, six, raw_reads, case):
    """Rounds from signal with the round end, the store and the option on.  whole_fb: the stop rule that never fires under C_FB -- round 3 has one
    read above the cap, which tests/test_optins_together_gpu.py has as a fall-back round with the option off; the lines are those of the run
    with nothing on.  whole_default: the default stop rule under WHOLE_CAP -- five (read, round) pairs decline, one read twice in a row; the
    lines are the reference's recorded ones.  No round falls back, no hit comes home, only the declined reads' seeds do; a declined read is
    not kept and is seeded from the host in the round after, every other read from its half."""
    wr = mc.WholeReads(0, ref=ref)
    reads = _Windows(wr, raw_reads)
    c = dc.MAPPER_CASES[case]
    stop = oc.never() if case == "whole_fb" else StopOpt()
    want = driven(ref, six, wr, reads, {}, stop, True)["lines"] if case == "whole_fb" else [wr.expected_line("default", r) for r in range(wr.n_reads)]
    on = driven(ref, six, wr, reads, DECLINE_ON, stop, True, c["cap"])
    print(case, on["rounds"], on["resident"], on["kept"], on["decline"], on["round_end"])
    assert on["lines"] == want and (case == "whole_fb" or sum("\t*\t" not in ln for ln in want) >= 3)
    check_resident_declines(on, c)


def test_a_read_with_34_chains_is_declined_alone():
    """tests/optins_cases.py's decline_case: the round with the 34-chain read is not chained on the host -- the other three reads are counted as
    chained on the device, the read's 725 seeds come home, and the lines are those of the option-off mapper on an engine of its own"""
    dref, chunks = oc.decline_case()
    si = SeedIndex.from_signals(dref.forward, dref.reverse, threads=4)
    src = oc.EventReads(si, chunks, [len(x) for x in dref.forward])
    off = driven(dref, si, src, src, {}, oc.never())
    assert [d["fallback_rounds"] for d, _ in off["rounds"]] == [int(k == oc.DECLINED_ROUND) for k in range(4)]
    assert off["decline"] == dict(rounds_with_declines=0, reads_declined_seeds=0, reads_declined_chains=0, reads_chained_device=0, seed_bytes_to_host=0)
    on = driven(dref, si, src, src, DECLINE_ON, oc.never())
    print(on["rounds"], on["resident"], on["kept"], on["decline"], on["round_end"])
    assert on["lines"] == off["lines"] and sum("\tnc:i:0" not in ln for ln in on["lines"]) >= 3
    check_resident_declines(on, dc.MAPPER_CASES["decline_case"])


def plain_run(wr, e, stop, groups, device_chain):
    opt, copt = mc.whole_project_opts("default", 0)
    cm = mapper.CMapper(e, opt, stop, ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096, max_reads=wr.n_reads,
                        chain_opt=copt, output_chains=True, threads=3, carry=False, groups=groups, device_chain=device_chain)
    lines, rounds = mapper.map_reads_c(wr, list(range(wr.n_reads)), cm)
    out = dict(lines=lines, log=cm.log(), rounds=rounds, decline=cm.decline_stats(), round_end=cm.round_end_stats(), anchor_bytes=cm.timing()["anchor_bytes"])
    cm.close()
    return out


@pytest.mark.parametrize("round_end", [0, 1])
def test_two_read_groups_each_decline_their_own_reads(ref, round_end):
    """A plain device-chained mapper (hits from the host, no resident round) with two read groups under WHOLE_CAP: in round 1 the first group
    declines read 0, the second reads 1 and 7 (a read's group is its slot's parity).  Lines and log are the host-chained mapper's, no round is
    chained on the host, and with "device_round_end" on every (read, round) is ended once."""
    wr = mc.WholeReads(0, ref=ref)
    c = dc.MAPPER_CASES["whole_default"]
    assert {r % 2 for r in c["declined"][0]} == {0, 1}
    want = [wr.expected_line("default", r) for r in range(wr.n_reads)]
    e0 = ra.Engine(0)
    try:
        e0.upload_reference(ref.forward, ref.reverse)
        host = plain_run(wr, e0, StopOpt(), 2, False)
    finally:
        e0.close()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv(CAP, str(c["cap"]))
        e = ra.Engine(0)
        try:
            e.upload_reference(ref.forward, ref.reverse)
            e.set_option(OPTION, 1)
            e.set_option("device_round_end", round_end)
            on = plain_run(wr, e, StopOpt(), 2, True)   # (the second group's context is created here, under the cap)
        finally:
            e.close()
    print(round_end, on["decline"], on["round_end"])
    assert on["lines"] == host["lines"] == want and on["log"] == host["log"] and on["rounds"] == host["rounds"]
    assert on["anchor_bytes"] == 0 and host["anchor_bytes"] > 0   # (no round's anchor lists went up from the host: none was chained there)
    # (a read group that declines none of its reads in a round would not have fallen back either: its reads are not counted)
    others = sum(sum(1 for r in row if r % 2 == g and r not in d) for row, d in zip(c["chained"], c["declined"]) for g in (0, 1) if any(r % 2 == g for r in d))
    assert on["decline"] == dict(rounds_with_declines=sum(1 for d in c["declined"] if d), reads_declined_seeds=c["by_seeds"], reads_declined_chains=0,
                                 reads_chained_device=others, seed_bytes_to_host=0) and 0 < others < c["chained_device"]
    if round_end:
        assert on["round_end"]["reads_device"] + on["round_end"]["reads_declined"] == c["pairs"] and on["round_end"]["rounds"] == on["rounds"]
    else:
        assert on["round_end"]["rounds"] == 0


def test_the_int16_flow_above_a_cap_without_the_long_path(flow):  # noqa: F811
    """tests/test_optins_together_gpu.py's flow under L_MIX_FLOW with "chain_long_seeds" off: 21 of its 43 (read, round) pairs are above the cap,
    so that every round falls back without the option.  With it no round does, the lines are the option-off mapper's, and the reads declined
    for their seeds are the host's above() figure."""
    sref, si, chan, window, _ = flow
    n = FLOW_READS
    names, lens = ["synth_0"], [len(sref.forward[0])]
    ea = ra.Engine(0)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv(CAP, str(oc.L_MIX_FLOW))
        eb = ra.Engine(0)
    try:
        for e in (ea, eb):
            e.upload_reference(sref.forward, sref.reverse)
        for k, v in DECLINE_ON.items():
            eb.set_option(k, v)
        ca, cb = (mapper.CMapper(e, ra.MapOpt(), StopOpt(), names, lens, slot_events=4096, max_reads=n, threads=3, carry=False, groups=1, device_chain=True)
                  for e in (ea, eb))
        ids = [ca.add_read("read_%d" % r, 4000 * FLOW_CHUNKS, FLOW_CHUNKS) for r in range(n)]
        assert ids == [cb.add_read("read_%d" % r, 4000 * FLOW_CHUNKS, FLOW_CHUNKS) for r in range(n)]
        for c in range(FLOW_CHUNKS):
            sa, sb = [ca.state(i) for i in ids], [cb.state(i) for i in ids]
            assert sa == sb, c
            act = [r for r in range(n) if not sa[r][0]]
            if not act:
                break
            wins = [window(r, c) for r in act]
            raw, off = raw_batch(wins)
            _, eoff, ev = ea.detect_events_raw(raw, off, chan)
            ca.round([ids[r] for r in act], [(ev[int(eoff[k]):int(eoff[k + 1])], []) for k in range(len(act))], seed_index=si, resident=True)
            cb.round_signal([ids[r] for r in act], wins, si, channels=chan)
        assert ca.finish() == 0 and cb.finish() == 0
        la, lb = [ca.paf(i) for i in ids], [cb.paf(i) for i in ids]
        res, dcs, re_ = cb.resident_stats(), cb.decline_stats(), cb.round_end_stats()
        print(res, dcs, re_, cb.kept_stats())
        ca.close()
        cb.close()
    finally:
        ea.close()
        eb.close()
    assert la == lb and sum("\t*\t" not in ln for ln in la) >= FLOW_READS // 2
    assert res["fallback_rounds"] == 0 and res["resident_rounds"] == FLOW_CHUNKS and res["hit_bytes_to_host"] == 0
    want = dc.MAPPER_CASES["flow"]
    assert dcs["reads_declined_seeds"] == oc.FLOW["above"][0] == want["by_seeds"]   # (the host's above() figure)
    assert dcs["reads_declined_chains"] == 0 and dcs["rounds_with_declines"] == want["rounds_with_declines"] and dcs["reads_chained_device"] == want["chained_device"]
    assert dcs["seed_bytes_to_host"] > 12 * oc.L_MIX_FLOW * want["by_seeds"] and oc.FLOW["pairs"] == re_["reads_device"] + re_["reads_declined"]


def test_the_mapper_with_the_option_off_falls_back_as_it_did(ref, six):
    """the same engine options but "chain_decline_reads": round 3 of whole_fb is a fall-back round, its hits come home, and nothing is counted
    as declined alone"""
    wr = mc.WholeReads(0, ref=ref)
    c = dc.MAPPER_CASES["whole_fb"]
    off = driven(ref, six, wr, wr, dict(device_round_end=1, resident_chains=4096), oc.never(), False, c["cap"])
    assert [d["fallback_rounds"] for d, _ in off["rounds"]] == [int(bool(d)) for d in c["declined"]] and off["resident"]["hit_bytes_to_host"] > 0
    assert off["decline"] == dict(rounds_with_declines=0, reads_declined_seeds=0, reads_declined_chains=0, reads_chained_device=0, seed_bytes_to_host=0)
