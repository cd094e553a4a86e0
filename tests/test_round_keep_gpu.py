"""The kept chains on the device (rawalign_amd/csrc/rawdtw_keep.hip: the store, k_keep_primary, rawdtw_round_keep, rawdtw_batch_round_end_keep /
_keep_fetch, rawdtw_chain_kept_fetch; rawdtw_chain_round_begin_resident_kept and k_seed_write_chain in rawdtw_chain.hip / rawdtw_seed.hip;
"resident_chains" in rawdtw_mapper.cpp) against the host restatement rawdtw_round_keep_host -- which tests/test_round_keep_host.py ties to
plain Python and to the reference's recorded chains -- byte for byte, against rawdtw_chain_round fed host-built seed lists, and, for the
mapper, against the reference's lines and the lines of the option-off run."""
import ctypes as C

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from rawalign_amd import mapper, seeding, synth
from rawalign_amd import mapping as M
from rawalign_amd.dtw import ANCHOR_DTYPE, CHAIN_REC_DTYPE, NO_KEEP, NOT_KEPT, PREV_HOST, SEED_DTYPE
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex
from tests import map_ref_cases as mc
from tests import round_end_cases as R
from tests import round_keep_cases as KC
from tests import seed_cases as sc

pytestmark = pytest.mark.gpu
INVALID, RANGE = 1, 4
NEVER = dict(min_bestmap_ratio=1e9, min_meanmap_ratio=1e9, min_chain_anchor=10 ** 6)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- 1. rawdtw_round_keep on constructed rounds -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "one-read", "seventy"])
def test_round_keep_equals_the_host_restatement(name):
    """Every slot's half 0 is filled first by a keep of CAP seeds a read; then the round is kept there (one read in seven nowhere).  Counts
    equal the host's; a kept half holds the host's list byte for byte and, behind it, what was there before; a half whose read was
    not kept (declined, above the cap, no destination) holds all of what was there before; half 1 of every slot was never written."""
    rd = KC.rounds()[name]
    n, cap = rd.n_reads, KC.CAP
    e = ra.Engine(0)
    try:
        with pytest.raises(ra.RawDTWError):   # no store yet
            e.round_keep(*rd.arrays(), np.zeros(n, np.uint32))
        e.chain_keep_reserve(n, cap)
        fill = KC.KeepRound([([cap], [0], False)] * n, 99)
        dst0 = (np.arange(n, dtype=np.uint32) * 2).astype(np.uint32)
        assert (e.round_keep(*fill.arrays(), dst0) == cap).all()
        _, f_off, f_seeds = ra.round_keep_host(*fill.arrays(), cap)
        dst = dst0.copy()
        dst[3::7] = NO_KEEP
        got = e.round_keep(*rd.arrays(), dst)
        w_kept, soff, seeds = ra.round_keep_host(*rd.arrays(), cap)
        want = np.where(dst == NO_KEEP, NOT_KEPT, w_kept).astype(np.uint32)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        assert (want == NOT_KEPT).any() or n == 1
        for r in range(n):
            before = f_seeds[int(f_off[r]):int(f_off[r + 1])]
            cnt, half = e.chain_kept_fetch(r * 2, cap)
            assert e.chain_kept_fetch(r * 2 + 1, 0)[0] == NOT_KEPT, r
            if dst[r] == NO_KEEP:   # not a destination of the second keep: as the first left it
                assert cnt == cap and half.tobytes() == before.tobytes(), r
                continue
            assert cnt == int(want[r]), r
            k = 0 if cnt == NOT_KEPT else cnt
            assert half[:k].tobytes() == seeds[int(soff[r]):int(soff[r + 1])].tobytes(), r
            assert half[k:].tobytes() == before[k:].tobytes(), r
        # refusals, each before anything is enqueued: an address outside the store, the same address twice, more seeds than a half holds
        bad = dst.copy()
        bad[0] = 2 * n
        with pytest.raises(ra.RawDTWError):
            e.round_keep(*rd.arrays(), bad)
        if n > 1:
            bad = dst0.copy()
            bad[1] = bad[0]
            with pytest.raises(ra.RawDTWError):
                e.round_keep(*rd.arrays(), bad)
        with pytest.raises(ra.RawDTWError):
            e.chain_kept_fetch(2 * n, 1)
        with pytest.raises(ra.RawDTWError):
            e.chain_kept_fetch(0, cap + 1)
        assert e.chain_kept_fetch(0, 0)[0] == int(want[0])   # (none of them changed a half)
        assert e.get_option("round_keep_kernel_us") >= 0
    finally:
        e.close()


# ---- 2. the batch form, and seeding from the store ----------------------------------------------------------------------------------------
def seeds_of(hits, chunk_start):
    s = np.zeros(len(hits), SEED_DTYPE)
    s["key"] = hits["ref_seq"] * 2 + (hits["strand"] != 0)
    s["target_position"], s["query_position"] = hits["target_position"], hits["query_position"] + np.uint32(chunk_start)
    return s


class ChainedRound:
    """rawdtw_chain_round on per-read seed lists, its arrays on the host and the device pointers rawdtw_batch_submit_device takes"""

    def __init__(self, e, copt, per_read, read_base, key_base):
        n = len(per_read)
        self.n, self.e = n, e
        self.seed_off = np.zeros(n + 1, np.uint64)
        self.seed_off[1:] = np.cumsum([len(s) for s in per_read])
        allseeds = np.concatenate(list(per_read) + [np.zeros(1, SEED_DTYPE)])
        self.cap = n * 32
        self.chain_off, self.anchor_off = np.zeros(n + 1, np.uint64), np.zeros(self.cap + 1, np.uint64)
        self.recs, self.anchors = np.zeros(self.cap, CHAIN_REC_DTYPE), np.zeros(int(self.seed_off[-1]) + 1, ANCHOR_DTYPE)
        self.d = [C.c_void_p() for _ in range(3)]
        st = e.lib.rawdtw_chain_round(e._ctx, C.byref(copt), n, vp(self.seed_off), vp(allseeds), vp(read_base), len(key_base), vp(key_base), vp(self.chain_off),
                                      vp(self.anchor_off), vp(self.recs), self.cap, vp(self.anchors), *[C.byref(x) for x in self.d])
        assert st == 0, e.lib.rawdtw_last_error(e._ctx)
        self.nc = int(self.chain_off[-1])
        self.na = int(self.anchor_off[self.nc])

    def same(self, other):
        return (np.array_equal(self.chain_off, other[0]) and np.array_equal(self.anchor_off[:self.nc + 1], other[1][:self.nc + 1]) and
                self.recs[:self.nc].tobytes() == other[2][:self.nc].tobytes() and self.anchors[:self.na].tobytes() == other[3][:self.na].tobytes())

    def end_and_keep(self, so, dst, fetch_first=True):
        """submit_device -> round_end_begin -> round_end_keep -> the fetches: (score, keep, out, primary, kept_count, planned on the device)"""
        e, lib, n, nc = self.e, self.e.lib, self.n, self.nc
        co, h = ra.MapOpt(dtw_min_score=5.0).c_struct(), C.c_void_p()
        assert lib.rawdtw_batch_submit_device(e._ctx, C.byref(co), n, vp(self.chain_off), vp(self.anchor_off), *self.d, C.byref(h)) == 0, lib.rawdtw_last_error(e._ctx)
        assert lib.rawdtw_batch_round_end_keep(e._ctx, h, vp(dst)) == INVALID   # no round end begun
        assert lib.rawdtw_batch_round_end_begin(e._ctx, h, C.byref(so), C.c_void_p(e.chain_round_recs()), 1) == 0, lib.rawdtw_last_error(e._ctx)
        for bad in self.bad_dsts(dst):
            assert lib.rawdtw_batch_round_end_keep(e._ctx, h, vp(bad)) == INVALID
        assert lib.rawdtw_batch_round_end_keep(e._ctx, h, vp(dst)) == 0, lib.rawdtw_last_error(e._ctx)
        assert lib.rawdtw_batch_round_end_keep(e._ctx, h, vp(dst)) == INVALID   # one keep at a time
        score, keep = np.zeros(nc + 1, np.float32), np.zeros(nc + 1, np.uint8)
        out, prim, kept = np.zeros(n, ra.ROUND_OUT_DTYPE), np.zeros(nc + 1, np.uint32), np.zeros(n, np.uint32)
        if fetch_first:
            assert lib.rawdtw_batch_fetch(e._ctx, h, vp(score), vp(keep), None) == 0
        assert lib.rawdtw_batch_round_keep_fetch(e._ctx, h, vp(kept)) == INVALID   # the round end is fetched first
        assert lib.rawdtw_batch_round_end_fetch(e._ctx, h, vp(out), vp(prim)) == 0, lib.rawdtw_last_error(e._ctx)
        assert lib.rawdtw_batch_round_keep_fetch(e._ctx, h, vp(kept)) == 0, lib.rawdtw_last_error(e._ctx)
        assert lib.rawdtw_batch_round_keep_fetch(e._ctx, h, vp(kept)) == INVALID
        if not fetch_first:
            assert lib.rawdtw_batch_fetch(e._ctx, h, vp(score), vp(keep), None) == 0
        w, cnt = (C.c_uint64 * 21)(), C.c_uint32()
        assert lib.rawdtw_batch_chunk_profile(e._ctx, h, 0, w, 21, C.byref(cnt)) == 0
        assert lib.rawdtw_batch_destroy(h) == 0
        return score[:nc], keep[:nc], out, prim[:nc], kept, cnt.value != 0

    def bad_dsts(self, dst):
        a, b = dst.copy(), dst.copy()
        a[0] = 2 * self.n          # outside the store
        b[1] = b[0]                # the same address twice
        return a, b

    def check_kept(self, out, prim, kept, dst, cap):
        """counts and halves against rawdtw_round_keep_host on the fetched arrays; -> (the host's counts, offsets, seeds)"""
        w_kept, soff, seeds = ra.round_keep_host(self.chain_off, self.recs[:self.nc], self.anchor_off[:self.nc + 1], self.anchors[:self.na], out, prim, cap)
        want = np.where(dst == NO_KEEP, NOT_KEPT, w_kept).astype(np.uint32)
        assert np.array_equal(kept, want), np.nonzero(kept != want)[0][:10]
        for r in range(self.n):
            if dst[r] == NO_KEEP:
                continue
            cnt, half = self.e.chain_kept_fetch(int(dst[r]), 0 if want[r] == NOT_KEPT else int(want[r]))
            assert cnt == int(want[r]) and half.tobytes() == (b"" if cnt == NOT_KEPT else seeds[int(soff[r]):int(soff[r + 1])].tobytes()), r
        return want, soff, seeds


def test_the_batch_form_and_a_second_round_seeded_from_the_store():
    """rawdtw_chain_round -> rawdtw_batch_submit_device -> rawdtw_batch_round_end_begin -> rawdtw_batch_round_end_keep -> the fetches on 300 reads:
    counts and halves equal rawdtw_round_keep_host on the fetched arrays.  Then a second chunk is seeded in the arena (seed_resident) and chained by
    rawdtw_chain_round_begin_resident_kept with two reads in three taking their previous seeds from the store, the others from the host: chains,
    records and anchors byte-equal to rawdtw_chain_round fed the host-built lists.  Every refusal of the begin, then the round still runs."""
    rng = np.random.default_rng(5)
    ref = synth.make_reference([150_000], seed=31)
    n, cap = 300, 4096
    six = SeedIndex.from_signals(ref.forward, ref.reverse, threads=8)
    syn = mapper.SyntheticSeeds(ref, n, seed=9, max_chunks=2)
    e = ra.Engine(0)
    lib = e.lib
    try:
        e.upload_reference(ref.forward, ref.reverse)
        e.upload_seed_index(six)
        copt = M.default_chain_opt(6)
        evs, per_read, read_base, at = [], [], np.zeros(n, np.uint32), 0
        for r in range(n):
            ev, hits = syn.chunk(r, 0)
            read_base[r] = at
            at += len(ev)
            evs.append(np.asarray(ev, np.float32))
            s = np.zeros(len(hits), SEED_DTYPE)
            for k, (sq, st, t, q) in enumerate(hits):
                s[k] = (sq * 2 + (1 if st else 0), t, q)
            per_read.append(s)
        e.upload_events(np.concatenate(evs))
        key_base = np.array([e.reference_offset(0, 0), e.reference_offset(0, 1)], np.uint64)
        one = ChainedRound(e, copt, per_read, read_base, key_base)
        assert one.nc > n // 2
        dst = (np.arange(n, dtype=np.uint32) * 2 + (np.arange(n, dtype=np.uint32) & 1)).astype(np.uint32)
        dst[9::10] = NO_KEEP
        so = R.select_opt(1)
        h = C.c_void_p()
        co = ra.MapOpt().c_struct()   # no store on the context yet: refused
        assert lib.rawdtw_batch_submit_device(e._ctx, C.byref(co), n, vp(one.chain_off), vp(one.anchor_off), *one.d, C.byref(h)) == 0
        assert lib.rawdtw_batch_round_end_begin(e._ctx, h, C.byref(so), C.c_void_p(e.chain_round_recs()), 1) == 0
        assert lib.rawdtw_batch_round_end_keep(e._ctx, h, vp(dst)) == INVALID
        assert lib.rawdtw_batch_destroy(h) == 0
        e.chain_keep_reserve(n, cap)
        score, keep, out, prim, kept, on_device = one.end_and_keep(so, dst)
        assert on_device and (out["n_primary"] >= 1).sum() > n // 2
        want, soff, kseeds = one.check_kept(out, prim, kept, dst, cap)
        assert ((want != NOT_KEPT) & (want > 0)).sum() > n // 2 and e.get_option("round_keep_kernel_us") >= 0

        # ---- the second round ----
        chunks = [np.ascontiguousarray(syn.chunk(r, 1 if syn.read_job(r).n_chunks_available > 1 else 0)[0], np.float32) for r in range(n)]
        from tests.test_resident_round_gpu import place_in_arena

        start, ln = place_in_arena(e, chunks, rng)
        ev, off = sc.flat(chunks)
        hoff, hits = seeding.seed_hits_host(six, ev, off, threads=8)
        hoff = hoff.astype(np.int64)
        sits = np.zeros(n, np.uint8)
        sits[[4, 50, n - 1]] = 1
        chunk_start = np.array([len(evs[r]) for r in range(n)], np.uint32)
        src = np.full(n, PREV_HOST, np.uint32)
        prev_host, prev_all_reads = [], []
        for r in range(n):
            from_store = r % 3 != 0 and not sits[r] and dst[r] != NO_KEEP and want[r] != NOT_KEPT
            if from_store:
                src[r] = dst[r]
                prev_host.append(np.zeros(0, SEED_DTYPE))
                prev_all_reads.append(kseeds[int(soff[r]):int(soff[r + 1])])
                continue
            k = 0 if sits[r] or r % 6 == 0 else int(rng.integers(1, 40))
            p = np.zeros(k, SEED_DTYPE)
            p["key"], p["target_position"], p["query_position"] = rng.integers(0, 2, k), rng.integers(0, 140000, k), rng.integers(0, 500, k)
            prev_host.append(p)
            prev_all_reads.append(p)
        assert (src != PREV_HOST).sum() > n // 2 and sum(len(prev_all_reads[r]) for r in range(n) if src[r] != PREV_HOST) > n
        lists = [np.zeros(0, SEED_DTYPE) if sits[r] else np.concatenate([prev_all_reads[r], seeds_of(hits[hoff[r]:hoff[r + 1]], chunk_start[r])]) for r in range(n)]
        assert max(len(s) for s in lists) <= 2048
        rs = e.seed_resident(start, ln)
        assert np.array_equal(rs.hit_off.astype(np.int64), hoff)
        seed_off = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.uint64)
        prev_off = np.concatenate([[0], np.cumsum([len(p) for p in prev_host])]).astype(np.uint64)
        prev_all = np.concatenate(prev_host + [np.zeros(1, SEED_DTYPE)])
        cap2 = n * 32

        def kept_round(seed_off_=seed_off, src_=src, sits_=sits, prev_off_=prev_off):
            got = (np.zeros(n + 1, np.uint64), np.zeros(cap2 + 1, np.uint64), np.zeros(cap2, CHAIN_REC_DTYPE), np.zeros(int(seed_off[-1]) + 1, ANCHOR_DTYPE))
            d = [C.c_void_p() for _ in range(3)]
            st = lib.rawdtw_chain_round_begin_resident_kept(e._ctx, C.byref(copt), n, vp(seed_off_), vp(prev_off_), vp(prev_all), vp(src_), vp(chunk_start), vp(sits_),
                                                            vp(read_base), 2, vp(key_base), vp(got[0]), vp(got[1]), vp(got[2]), cap2, vp(got[3]))
            if st == 0:
                st = lib.rawdtw_chain_round_end(e._ctx, *[C.byref(x) for x in d])
            return st, got

        st, got = kept_round()
        assert st == 0, lib.rawdtw_last_error(e._ctx)
        two = ChainedRound(e, copt, lists, read_base, key_base)   # (the seeding's hits stay: a chaining round does not touch them)
        assert two.nc > n // 2 and two.same(got)
        # the refusals, each before anything is enqueued
        r_store = int(np.nonzero(src != PREV_HOST)[0][0])
        bad = src.copy()
        bad[r_store] = 2 * n                                    # an address outside the store
        assert kept_round(src_=bad)[0] == INVALID
        bad = src.copy()
        bad[r_store] = dst[r_store] ^ 1                          # a half that was never written
        assert kept_round(src_=bad)[0] == INVALID
        r_void = int(np.nonzero((dst != NO_KEEP) & (want == NOT_KEPT))[0][0]) if ((dst != NO_KEEP) & (want == NOT_KEPT)).any() else None
        if r_void is not None:                                   # a half whose count is RAWDTW_NOT_KEPT
            bad = src.copy()
            bad[r_void] = dst[r_void]
            assert kept_round(src_=bad)[0] == INVALID
        bad = src.copy()
        bad[4] = dst[4]                                          # a read that sits out and has a source
        assert kept_round(src_=bad)[0] == INVALID
        bad = seed_off.copy()
        bad[r_store + 1:] += 1                                   # a wrong stretch
        assert kept_round(seed_off_=bad)[0] == INVALID
        bad = prev_off.copy()
        bad[r_store + 1:] += 1                                   # a read seeded from the store with previous seeds from the host too
        assert kept_round(prev_off_=bad)[0] == INVALID
        assert lib.rawdtw_chain_round_begin_resident_kept(e._ctx, C.byref(copt), n, vp(seed_off), vp(prev_off), vp(prev_all), None, vp(chunk_start), vp(sits),
                                                          vp(read_base), 2, vp(key_base), vp(got[0]), vp(got[1]), vp(got[2]), cap2, vp(got[3])) == INVALID
        d = [C.c_void_p() for _ in range(3)]
        assert lib.rawdtw_chain_round_end(e._ctx, *[C.byref(x) for x in d]) == INVALID   # (none of them began a round)
        rs = e.seed_resident(start, ln)
        st, again = kept_round()
        assert st == 0 and two.same(again)
    finally:
        e.close()


def test_a_declined_batchs_kept_halves_are_the_redone_round_ends():
    """A device-chained batch that runs out of pass slots (tests/test_stream_path.py's chains as the chaining's seeds) is scored again through the
    job list when it is fetched; its round end runs again on those scores and the keep launch behind it: counts and halves equal
    rawdtw_round_keep_host on what the fetches returned -- whether the batch or the round end is fetched first."""
    from tests.test_stream_path import _chains, _medium

    rng = np.random.default_rng(77)
    ref = [rng.normal(size=60000).astype(np.float32), rng.normal(size=60000).astype(np.float32)]
    n, cap = 300, 4096
    e = ra.Engine(0)
    try:
        e.set_option("tile_lds_floats", 2048)
        e.set_option("pass_pool", 1)
        e.upload_reference([ref[0]], [ref[1]])
        events, chain_off, anchor_off, anchors, slot, read_base_c = _chains(rng, n, 60000, _medium, (1, 30))
        per_read, read_base = [], np.zeros(n, np.uint32)
        for r in range(n):
            c0, c1 = int(chain_off[r]), int(chain_off[r + 1])
            read_base[r] = read_base_c[c0]
            rows = [np.zeros(0, SEED_DTYPE)]
            for c in range(c0, c1):
                a = anchors[int(anchor_off[c]):int(anchor_off[c + 1])]
                s = np.zeros(len(a), SEED_DTYPE)
                s["key"], s["target_position"], s["query_position"] = int(slot[c]), a["target_position"], a["query_position"]
                rows.append(s)
            per_read.append(np.concatenate(rows))
        e.upload_events(events)
        key_base = np.array([e.reference_offset(0, 0), e.reference_offset(0, 1)], np.uint64)
        copt = M.default_chain_opt(6)
        e.chain_keep_reserve(n, cap)
        so = R.select_opt(0)
        halves = []
        for i, fetch_first in enumerate((True, False)):
            rnd = ChainedRound(e, copt, per_read, read_base, key_base)
            assert rnd.nc > n // 2
            dst = (np.arange(n, dtype=np.uint32) * 2 + i).astype(np.uint32)
            score, keep, out, prim, kept, on_device = rnd.end_and_keep(so, dst, fetch_first)
            assert not on_device   # declined: more passes than slots
            want = ra.round_end_host(so, rnd.chain_off, rnd.recs[:rnd.nc], score, keep)
            rd = R.Round([], 0)
            rd.chain_off, rd.recs, rd.score, rd.keep = rnd.chain_off, rnd.recs[:rnd.nc], score, keep
            R.assert_equal_except_declined(rd, (out, prim), want, fetch_first)
            w, _, _ = rnd.check_kept(out, prim, kept, dst, cap)
            assert ((w != NOT_KEPT) & (w > 0)).sum() > n // 2
            halves.append(w)
        assert np.array_equal(halves[0], halves[1])
    finally:
        e.close()


# ---- 3. the mapper ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref():
    return mc.make_reference()


@pytest.fixture(scope="module")
def six(ref):
    return SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)


def whole_mapper(e, wr, opt, copt, stop=None, slot_events=4096):
    return mapper.CMapper(e, opt, stop or StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=slot_events,
                          max_reads=wr.n_reads, chain_opt=copt, output_chains=True, threads=3, carry=False, groups=1, device_chain=True)


def whole_run(ref, six, wr, name, form, resident_chains, stop=None):
    """map_reads_c(..., resident=True), one group, "device_round_end" on: (lines, rounds, resident / round-end / kept stats)"""
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        e.set_option("device_round_end", 1)
        e.set_option("resident_chains", resident_chains)
        assert e.get_option("resident_chains") == resident_chains
        opt, copt = mc.whole_project_opts(name, form)
        cm = whole_mapper(e, wr, opt, copt, stop)
        got, rounds = mapper.map_reads_c(wr, list(range(wr.n_reads)), cm, seed_index=six, resident=True)
        out = (got, rounds, cm.resident_stats(), cm.round_end_stats(), cm.kept_stats())
        cm.close()
        return out
    finally:
        e.close()


DTW_SETS = [k for k, f in mc.WHOLE_SETS.items() if f["flag"] & (mc.EVAL | mc.CIGAR)]
# decided on the CPU (round_keep_cases.whole_reads_host_run: ties on all seven keys, more than 64 chains taking part, NaN, a quotient that is
# not finite -- over every (read, round) of the host-path run): no read of any of these sets, in either build, is declined
STRICT_SETS = ("default", "cigar", "global_full", "frac025")


@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("name", list(mc.WHOLE_SETS))
def test_whole_reads_give_the_references_lines_with_the_chains_kept(six, ref, name, form):
    """"resident_chains" = 4096 (a read never has more than 376 seeds here: tests/test_resident_round_gpu.py): every line is the reference's,
    no round falls back, and previous seeds come from the device.  The sets that carry the strict assert -- no previous seed from the host at
    all -- are default, cigar, global_full and frac025, both builds: the host-path run of each (no device) shows that the round end declines
    none of their reads.  noeval runs no DTW, so its rounds do not end on the device and the store is not used: its counters stay 0."""
    wr = mc.WholeReads(form, ref=ref)
    want = [wr.expected_line(name, r) for r in range(wr.n_reads)]
    declined_host, _ = KC.whole_reads_host_run(name, form)
    got, rounds, res, re_, kp = whole_run(ref, six, wr, name, form, 4096)
    print(name, form, rounds, res, re_, kp)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, form, r)
    assert res["fallback_rounds"] == 0 and res["resident_rounds"] == rounds
    if name not in DTW_SETS:
        assert kp == dict(reads_from_device=0, reads_from_host=0, seeds_from_device=0, seeds_from_host=0, reads_not_kept=0) and re_["rounds"] == 0
        return
    assert kp["seeds_from_device"] > 0 and kp["reads_from_device"] > 0
    assert kp["reads_from_host"] <= re_["reads_declined"]
    assert (name in STRICT_SETS) == (declined_host == 0)
    if name in STRICT_SETS:
        assert re_["reads_declined"] == 0 and kp["seeds_from_host"] == 0 and kp["reads_from_host"] == 0 and kp["reads_not_kept"] == 0
        assert res["seed_bytes_to_device"] == 0   # (12 bytes a seed actually sent up)


def test_mixed_sources_at_the_median_cap(six, ref):
    """"resident_chains" at the median of the reads' per-round primary-anchor totals (from the host-path run of the same reads, all chunks):
    reads above it are not kept and seeded from the host, the others from the device; the lines are those of the option-off run"""
    wr = mc.WholeReads(0, ref=ref)
    stop = StopOpt(**NEVER)
    e0 = whole_run(ref, six, wr, "default", 0, 0, stop)
    assert e0[4] == dict(reads_from_device=0, reads_from_host=0, seeds_from_device=0, seeds_from_host=0, reads_not_kept=0)
    totals = all_chunk_totals(wr)
    cap = int(np.median([t for t in totals if t > 0]))
    on = whole_run(ref, six, wr, "default", 0, cap, stop)
    print(cap, sorted(totals), on[2], on[4])
    assert on[0] == e0[0] and on[1] == e0[1] and on[3] == e0[3]
    assert on[2]["resident_rounds"] == e0[2]["resident_rounds"] and on[2]["fallback_rounds"] == 0
    kp = on[4]
    assert kp["reads_from_device"] > 0 and kp["reads_from_host"] > 0 and kp["reads_not_kept"] > 0
    assert on[2]["seed_bytes_to_device"] == 12 * kp["seeds_from_host"] < e0[2]["seed_bytes_to_device"]
    assert 12 * (kp["seeds_from_host"] + kp["seeds_from_device"]) == e0[2]["seed_bytes_to_device"]


def all_chunk_totals(wr):
    """every (read, round)'s total of primary-chain anchors when no read stops early: the Python mirror with the oracle's scorer (no device)"""
    from oracle.loader import Oracle
    from tests.util import OracleScorer

    opt, copt = mc.whole_project_opts("default", 0)
    totals = []
    mapper.map_reads(wr, list(range(wr.n_reads)), OracleScorer(Oracle(), wr.ref), opt, StopOpt(**NEVER), chain_opt=copt, output_chains=True,
                     on_round=lambda rnd, chains: totals.extend(sum(c.n_anchors for c in ch) for ch in chains.values()))
    return totals


def drive(cm, wr, six, schedule, skip=()):
    """rounds by hand: schedule(round) -> resident?; -> per round the kept stats' increase"""
    ids = [cm.add_read(wr.read_job(r).name, wr.read_job(r).qlen, wr.read_job(r).n_chunks_available) for r in range(wr.n_reads)]
    done, deltas, rnd = {i: 0 for i in ids}, [], 0
    while True:
        act = [(i, r) for r, i in enumerate(ids) if r not in skip and not cm.state(i)[0] and done[i] < wr.n_chunks(r)]
        if not act:
            break
        before = cm.kept_stats()
        resident = schedule(rnd)
        cm.round([i for i, _ in act], [wr.chunk(r, done[i]) for i, r in act], seed_index=six, resident=resident)
        after = cm.kept_stats()
        deltas.append((resident, {k: after[k] - before[k] for k in after}))
        for i, _ in act:
            done[i] += 1
        rnd += 1
    assert cm.finish() == 0
    return [cm.paf(i) for i in ids], deltas, ids


def manual_run(ref, six, wr, resident_chains, schedule, stop, fn=drive, **kw):
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        e.set_option("device_round_end", 1)
        e.set_option("resident_chains", resident_chains)
        opt, copt = mc.whole_project_opts("default", 0)
        cm = whole_mapper(e, wr, opt, copt, stop, **kw)
        out = fn(cm, wr, six, schedule)
        cm.close()
        return out
    finally:
        e.close()


class SplitSecondChunk:
    """a WholeReads whose reads' second chunks come in two pieces: the first 40 events (below min_events = 50: the read sits that round out,
    rmap.cpp:569-572), then the rest"""

    def __init__(self, wr):
        self.wr, self.n_reads, self.lens = wr, wr.n_reads, wr.lens

    def split(self, r):   # (a second chunk too short to leave 50 events behind the cut stays whole: it sits out as it is)
        return self.wr.n_chunks(r) >= 2 and len(self.wr.chunk(r, 1)[0]) >= 40 + 50

    def n_chunks(self, r):
        return self.wr.n_chunks(r) + (1 if self.split(r) else 0)

    def chunk(self, r, c):
        if c == 0 or not self.split(r):
            return self.wr.chunk(r, c)
        if c > 2:
            return self.wr.chunk(r, c - 1)
        ev = self.wr.chunk(r, 1)[0]
        return (ev[:40], []) if c == 1 else (ev[40:], [])

    def read_job(self, r):
        j = self.wr.read_job(r)
        return mapper.ReadJob(j.name, qlen=j.qlen, n_chunks_available=self.n_chunks(r))


def test_a_read_that_sits_a_round_out_is_seeded_from_the_half_kept_two_rounds_earlier(six, ref):
    """Every read's second chunk is fed in two pieces, 40 events and the rest: in the second round every read sits out (its chains stay, nothing is
    kept or taken), and in the third the reads that left chains in the first are seeded from the halves that round kept -- as many reads, with
    as many seeds, as the second round of the same reads fed whole.  The lines are the option-off run's."""
    wr = mc.WholeReads(0, ref=ref)
    sp = SplitSecondChunk(wr)
    assert sum(sp.split(r) for r in range(wr.n_reads)) >= 5
    assert all(len(sp.chunk(r, 1)[0]) < 50 for r in range(wr.n_reads) if sp.n_chunks(r) >= 2)   # every read sits its second round out
    stop = StopOpt(**NEVER)
    off = manual_run(ref, six, sp, 0, lambda k: True, stop)
    on = manual_run(ref, six, sp, 4096, lambda k: True, stop)
    whole = manual_run(ref, six, wr, 4096, lambda k: True, stop)
    print(on[1], whole[1])
    assert on[0] == off[0]
    d, w = on[1], whole[1]
    assert not any(d[0][1].values()) and not any(d[1][1].values())   # no previous seed; every read sits out
    assert d[2][1]["reads_from_device"] == w[1][1]["reads_from_device"] > 0 and d[2][1]["seeds_from_device"] == w[1][1]["seeds_from_device"] > 0
    assert d[2][1]["reads_from_host"] == 0 and d[2][1]["reads_not_kept"] == 0


def test_rounds_through_the_other_entries_invalidate_the_kept_chains(six, ref):
    """resident rounds and rawdtw_mapper_round_seeded rounds in turns: the lines are the option-off run's, and in a resident round directly after a
    non-resident one no read takes its seeds from the device (they all come from the host); after a resident one they do"""
    wr = mc.WholeReads(0, ref=ref)
    stop = StopOpt(**NEVER)
    pattern = lambda k: k % 3 != 2   # noqa: E731  (resident, resident, seeded, resident, ...)
    off = manual_run(ref, six, wr, 0, pattern, stop)
    on = manual_run(ref, six, wr, 4096, pattern, stop)
    assert on[0] == off[0]
    d = on[1]
    print(d)
    assert len(d) >= 4
    saw_device = saw_host = False
    for k, (resident, delta) in enumerate(d):
        if not resident:
            assert not any(delta.values()), k                     # (the store is not used at all)
        elif k > 0 and not d[k - 1][0]:
            assert delta["reads_from_device"] == 0 and delta["reads_from_host"] > 0, k
            saw_host = True
        elif k > 0:
            assert delta["reads_from_host"] == 0 and delta["reads_from_device"] > 0, k
            saw_device = True
    assert saw_device and saw_host


def test_a_failed_round_changes_nothing(six, ref):
    """Slots of 1 200 events: after two rounds that kept chains, the third chunk of some reads no longer fits their slot and the whole round is
    refused (RAWDTW_ERR_RANGE); the round is then run with the reads that fit.  The lines are those of a run that never tried, and of the
    option-off run; the round after the failure takes its seeds from the device as in the run that never tried."""
    wr = mc.WholeReads(0, ref=ref)
    SLOT = 1200
    sizes = [[len(wr.chunk(r, c)[0]) for c in range(wr.n_chunks(r))] for r in range(wr.n_reads)]
    assert all(sum(s[:2]) <= SLOT for s in sizes)
    outgrow = {r for r, s in enumerate(sizes) if len(s) >= 3 and sum(s[:3]) > SLOT}
    fit = {r for r, s in enumerate(sizes) if len(s) >= 3 and sum(s[:3]) <= SLOT}
    assert outgrow and fit
    stop = StopOpt(**NEVER)

    def driver(disturb):
        def run(cm, w, s, schedule):
            ids = [cm.add_read(w.read_job(r).name, w.read_job(r).qlen, w.read_job(r).n_chunks_available) for r in range(w.n_reads)]
            failed, after_failure = 0, None
            for rnd in range(3):
                act = [(i, r) for r, i in enumerate(ids) if rnd < w.n_chunks(r) and not (rnd == 2 and r in outgrow)]
                if rnd == 2 and disturb:
                    everyone = [(i, r) for r, i in enumerate(ids) if rnd < w.n_chunks(r)]
                    before = (cm.kept_stats(), cm.resident_stats(), cm.stats())
                    with pytest.raises(RuntimeError, match="status %d: a read outgrew its slot" % RANGE):
                        cm.round([i for i, _ in everyone], [w.chunk(r, rnd) for _, r in everyone], seed_index=s, resident=True)
                    assert (cm.kept_stats(), cm.resident_stats(), cm.stats()) == before
                    failed += 1
                before = cm.kept_stats()
                cm.round([i for i, _ in act], [w.chunk(r, rnd) for _, r in act], seed_index=s, resident=True)
                if rnd == 2:
                    after_failure = {k: v - before[k] for k, v in cm.kept_stats().items()}
            assert cm.finish() == 0
            return [cm.paf(i) for i in ids], failed, after_failure, cm.kept_stats()
        return run

    off = manual_run(ref, six, wr, 0, None, stop, fn=driver(False), slot_events=SLOT)
    calm = manual_run(ref, six, wr, 4096, None, stop, fn=driver(False), slot_events=SLOT)
    hit = manual_run(ref, six, wr, 4096, None, stop, fn=driver(True), slot_events=SLOT)
    print(calm[2], calm[3])
    assert hit[1] == 1 and hit[0] == calm[0] == off[0]
    assert hit[2] == calm[2] and hit[3] == calm[3] and hit[2]["reads_from_device"] > 0 and hit[2]["reads_from_host"] == 0
