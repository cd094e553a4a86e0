"""k_fold_select (rawdtw_runs.hip: a read a lane, one wave for the reads' first chains and one for the rest) against the
oracle's sequential loop (rmap.cpp:515-524 calling align_chain with the running best), chain by chain and bit for bit:
every chain length around the rounds of sixteen parts at every 16-byte alignment of the chain's first cost, the workgroup's
edges, reads with no chain, with more chains than the lane's LDS cache holds and with hundreds, the ends of the cost array,
a long second chain, and a carried chunk round.

The inputs: a read's events are a stretch of the reference plus noise whose amplitude changes every few events over more than two
decades, so a chain on that diagonal ("good") has part costs of very different magnitudes and a small sum -- it passes the
gate (rmap.cpp:265-268) and is accepted -- while a chain anywhere else ("bad") is cut early.  Every batch is checked on
the CPU to hold a chain whose score changes when its parts are summed in reversed order."""
import ctypes as C

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch

    torch.cuda.is_available()
except Exception:  # pragma: no cover
    torch = None

import rawalign_amd as ra
from rawalign_amd.align import CandidateBatch
from tests.golden_util import bits

pytestmark = pytest.mark.gpu

REF_LEN = 60000
BONUS, MIN_SCORE = 0.4, 0.5
FOLD_CACHE = 8  # rawdtw_runs.hip, kFoldCache: chains behind a read's first whose score and gate stay in LDS
PARTS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49)
CARRY_DTYPE = np.dtype([("prev_src", "<u8"), ("parts", "<u4"), ("flags", "<u4"), ("start_t", "<u4"), ("start_q", "<u4")])  # rawdtw_carry_t


class _Builder:
    """Reads as lists of chains.  A chain is (parts, good) or (steps, good): `parts` steps of 1..6 events are drawn, `good`
    puts it on the read's diagonal.  All good chains of a read start at query 0, so chains with a common run of steps nest."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.ref = np.random.default_rng(4242).normal(size=REF_LEN).astype(np.float32)
        self.events, self.chain_off, self.anchor_off, self.anchors, self.read_base = [], [0], [0], [], []
        self.ev_at = 0

    @property
    def n_anchors(self):
        return self.anchor_off[-1]

    def read(self, chains):
        rng = self.rng
        steps = [np.asarray(c[0] if not np.isscalar(c[0]) else rng.integers(1, 7, size=int(c[0])), np.int64) for c in chains]
        read_len = max([int(s.sum()) + 6 for s in steps], default=0) + 1
        diag = int(rng.integers(0, REF_LEN - 2 * read_len - 8))
        # noise whose amplitude changes every five events over more than two decades, scaled so that no stretch from the read's start
        # costs more than 0.36 an event on its diagonal: a good chain (they start at query 0) stays attainable under the bonus of 0.4,
        # and its cost is large enough beside its score for the sum's last bits to show there
        noise = np.repeat(10.0 ** rng.uniform(-2.5, 0.0, size=read_len // 5 + 1), 5)[:read_len] * rng.normal(size=read_len)
        noise *= 0.36 / np.max(np.cumsum(np.abs(noise)) / np.arange(1, read_len + 1))
        self.events.append((self.ref[diag:diag + read_len] + noise).astype(np.float32))
        for s, (_, good) in zip(steps, chains):
            q = np.concatenate([[0 if good else int(rng.integers(0, 5))], np.cumsum(s)]).astype(np.int64)
            q[1:] += q[0]
            other = diag + read_len + int(rng.integers(0, read_len)) if diag < REF_LEN // 2 else int(rng.integers(0, diag - read_len))
            t = q + (diag if good else other - int(q[0]))
            assert t.min() >= 0 and t.max() < REF_LEN and q.max() < read_len
            a = np.zeros(len(q), ra.ANCHOR_DTYPE)
            a["query_position"], a["target_position"] = q[::-1], t[::-1]  # end-first (rmap.cpp:193-196)
            self.anchors.append(a)
            self.anchor_off.append(self.anchor_off[-1] + len(a))
            self.read_base.append(self.ev_at)
        self.chain_off.append(len(self.anchor_off) - 1)
        self.ev_at += read_len

    def filler_to(self, n_parts, residue):
        """how many anchors (1..4: 0..3 extra) a filler chain in front needs so that a chain of n_parts parts behind it has its
        first cost -- anchor index a1 - 2 -- at `residue` modulo four (the cost array is 256-byte aligned: rawdtw_stream_layout.h)"""
        return 1 + (residue - (self.n_anchors + 1 + n_parts + 1 - 2)) % 4

    def batch(self, eng):
        nc = len(self.anchor_off) - 1
        events = np.concatenate(self.events) if self.events else np.zeros(0, np.float32)
        return CandidateBatch(events, np.array(self.chain_off, np.uint64), np.array(self.anchor_off, np.uint64), np.concatenate(self.anchors),
                              np.full(nc, eng.reference_offset(0, 1), np.uint64), np.array(self.read_base, np.uint32))


def _random_reads(b, n):
    for _ in range(n):
        k = int(b.rng.choice([0, 1, 1, 2, 3, 4]))
        good = int(b.rng.integers(0, max(k, 1)))
        b.read([(int(b.rng.integers(0, 41)), c == good) for c in range(k)])


def _lengths(b):
    """every part count at every alignment, as a read's first chain (the filler is the read in front) and as its second"""
    for second in (False, True):
        for parts in PARTS:
            for residue in range(4):
                filler = (b.filler_to(parts, residue) - 1, False)
                if second:
                    b.read([filler, (parts, True)])
                else:
                    b.read([filler])
                    b.read([(parts, True)])
                assert (b.n_anchors - 2) % 4 == residue


def _counts(b):
    """reads with 0, 1, 2 chains, with one chain more than the first and the lane's cache take, two more, and 300; a long second chain.
    The reads of many chains: good chains at the cache's last place, at the first place behind it and at every twelfth from 20 on,
    each one part longer than the good one before it, steps of 30 events -- attainable (rmap.cpp:246: the span) stays ahead of the
    best score so far (rmap.cpp:306: anchors count twice) for 30 parts, so every one of them is accepted; bad and single-anchor
    chains between them."""
    b.read([])
    b.read([(33, True)])
    b.read([(20, True), (3, False)])
    goods = [0, FOLD_CACHE, FOLD_CACHE + 1] + list(range(20, 290, 12))
    for n in (FOLD_CACHE + 2, FOLD_CACHE + 3, 300):
        b.read([(np.full(1 + goods.index(c), 30), True) if c in goods else (int(b.rng.integers(0, 4)), False) for c in range(n)])
    b.read([])
    b.read([(np.array([2]), True), (400, True), (2, False)])
    b.read([(1, True), (5, False)])


def _edges(b, m):
    """the first chain starts at anchor 0 and is long enough for whole rounds; the last chain ends the list, n_anchors % 4 == m"""
    b.read([(32 + m, True)])
    _random_reads(b, 5)
    b.read([(b.filler_to(33, (m - 2) % 4) - 1, False), (33, True)])
    assert b.n_anchors % 4 == m


CASES = {"lengths": (11, _lengths), "counts": (12, _counts), "edges1": (113, lambda b: _edges(b, 1)), "edges2": (114, lambda b: _edges(b, 2)),
         "edges3": (115, lambda b: _edges(b, 3))}
CASES["reads1"] = (201, lambda b: b.read([(17, True), (33, True), (49, True), (4, False)]))
CASES.update({"reads%d" % n: (100 + n, lambda b, n=n: _random_reads(b, n)) for n in (63, 64, 65, 129)})


@pytest.fixture(scope="module")
def eng():
    e = ra.Engine(0)
    ref = np.random.default_rng(4242).normal(size=REF_LEN).astype(np.float32)
    e.upload_reference([ref], [ref[::-1].copy()])
    yield e
    e.close()


_built = {}


def _case(name, eng):
    if name not in _built:
        b = _Builder(CASES[name][0])
        CASES[name][1](b)
        _built[name] = (b.batch(eng), b.ref)
    return _built[name]


def _check(oracle, cb, ref, score, keep, jc, fused):
    """the oracle's loop; returns (chains cut, chains accepted as the new best, [index in its read of every accepted chain])"""
    from oracle.loader import OrcOpt

    oopt = OrcOpt(1, 1, 0.10, BONUS, MIN_SCORE, fused)
    n_cut, accepted = 0, []
    for r in range(cb.n_reads):
        best = np.float32(0.0)
        c0 = int(cb.chain_off[r])
        for c in range(c0, int(cb.chain_off[r + 1])):
            a = cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])]
            want = oracle.align_chain(a, ref, cb.events[int(cb.read_base[c]):], oopt, float(best))
            assert bits(score[c]) == bits(want), (r, c - c0, len(a) - 1, score[c], want)
            k = want >= np.float32(MIN_SCORE)
            assert bool(keep[c]) == bool(k), (r, c - c0)
            n_cut += want == np.float32(-1e10)
            if k and want > best:
                best = want
                accepted.append(c - c0)
    # the condition on the inputs: some chain's score depends on the order its parts are summed in
    n_parts = np.diff(cb.anchor_off.astype(np.int64)) - 1
    first = np.concatenate([[0], np.cumsum(np.maximum(n_parts, 0))])
    assert first[-1] == len(jc)
    differs = 0
    for c in np.flatnonzero((n_parts >= 3) & (score != np.float32(-1e10))):  # (chains that were not cut: their sums reach the output)
        x = jc[first[c]:first[c + 1]]
        fwd, rev = np.float32(0.0), np.float32(0.0)
        for v in x[:-1]:
            fwd = np.float32(fwd + v)
        for v in x[:-1][::-1]:
            rev = np.float32(rev + v)
        a = cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])]
        prod = np.float32(np.float32(int(np.sum(a["query_position"][:-1].astype(np.int64) - a["query_position"][1:].astype(np.int64) + 1))) * np.float32(BONUS))
        differs += bits(np.float32(prod - np.float32(fwd + x[-1]))) != bits(np.float32(prod - np.float32(rev + x[-1])))
    return n_cut, accepted, differs


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_fold_lanes_against_oracle_loop(eng, oracle, name, fused):
    cb, ref = _case(name, eng)
    eng.upload_events(cb.events)
    opt = ra.MapOpt(dtw_min_score=MIN_SCORE, dtw_match_bonus=BONUS, fused_score=bool(fused))
    b = ra.Batch(eng, opt, cb)
    assert b.verify_plan() is True  # the sync-free path took the batch: fold_mode 4 is k_fold_select
    b.run()
    score, keep, jc = b.fetch(with_job_costs=True)
    b.close()
    n_cut, accepted, differs = _check(oracle, cb, ref, score, keep, jc, fused)
    assert n_cut > 0 and len(accepted) > 0, (n_cut, len(accepted))  # both the early-cut path and the accept path were taken
    assert differs > 0
    if name == "counts":
        # scores that came back from memory reach the output (chains with parts that were not cut), the first place behind the cache
        # too (place FOLD_CACHE is the cache's last), and some of them are the new best
        n_parts = np.diff(cb.anchor_off.astype(np.int64)) - 1
        pos = np.arange(cb.n_chains) - np.repeat(cb.chain_off[:-1].astype(np.int64), np.diff(cb.chain_off.astype(np.int64)))
        uncut = pos[(n_parts >= 1) & (score != np.float32(-1e10))].tolist()
        assert sum(k > FOLD_CACHE for k in uncut) > 20 and uncut.count(FOLD_CACHE) == 3 and uncut.count(FOLD_CACHE + 1) == 3
        assert max(accepted) > 200 and sum(k > FOLD_CACHE for k in accepted) > 10 and accepted.count(FOLD_CACHE + 1) == 3
        assert np.diff(cb.chain_off.astype(np.int64)).tolist()[:6] == [0, 1, 2, FOLD_CACHE + 2, FOLD_CACHE + 3, 300]
    if name == "lengths":
        # every part count at every alignment of its first cost, as a first chain and behind one
        n_parts = np.diff(cb.anchor_off.astype(np.int64)) - 1
        pos = np.arange(cb.n_chains) - np.repeat(cb.chain_off[:-1].astype(np.int64), np.diff(cb.chain_off.astype(np.int64)))
        for behind in (0, 1):
            seen = {(int(p), int((a1 - 2) % 4)) for p, a1, k, s in zip(n_parts, cb.anchor_off[1:].astype(np.int64), pos, score)
                    if k == behind and (s != np.float32(-1e10) or p == 0)}
            assert seen >= {(p, res) for p in PARTS for res in range(4)}, behind


def test_fold_lanes_carried_round(eng, oracle):
    """A chunk round of two reads on top of the round before (rawdtw_batch_submit_carry): the fold walks the full lists' cost array
    that k_gather assembled, and the scores are the oracle's for round 2."""
    b1, b2 = _Builder(31), _Builder(31)
    spec = [[(40, True), (5, False)], [(np.array([2]), True), (20, True), (17, False)]]
    for rd in spec:
        b2.read(rd)
    cb2, ref = b2.batch(eng), b2.ref
    # round 1: every chain without its last `cut` parts (end-first: the list's first entries)
    cuts = [7, 2, 0, 3, 16]
    a1, off1 = [], [0]
    for c in range(cb2.n_chains):
        a = cb2.anchors[int(cb2.anchor_off[c]):int(cb2.anchor_off[c + 1])][cuts[c]:]
        a1.append(a); off1.append(off1[-1] + len(a))
    cb1 = CandidateBatch(cb2.events, cb2.chain_off, np.array(off1, np.uint64), np.concatenate(a1), cb2.ref_base, cb2.read_base)
    lib = eng.lib
    vp = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    arr2 = [np.ascontiguousarray(x) for x in (cb2.chain_off, cb2.anchor_off, cb2.anchors, cb2.ref_base, cb2.read_base)]
    arr1 = [np.ascontiguousarray(x) for x in (cb1.chain_off, cb1.anchor_off, cb1.anchors, cb1.ref_base, cb1.read_base)]
    prev_read = np.arange(cb2.n_reads, dtype=np.uint64)
    carry = np.zeros(cb2.n_chains, CARRY_DTYPE)
    new_off, new_anchors = np.zeros(cb2.n_chains + 1, np.uint64), np.zeros(len(cb2.anchors) + 1, ra.ANCHOR_DTYPE)
    assert lib.rawdtw_round_match_chains(cb2.n_reads, *[vp(x) for x in arr2], vp(prev_read), *[vp(x) for x in arr1], vp(carry), vp(new_off),
                                         vp(new_anchors)) == 0
    assert int(carry["parts"].sum()) > 50  # (stretches are taken over)
    eng.upload_events(cb2.events)
    for fused in (0, 1):
        opt = ra.MapOpt(dtw_min_score=MIN_SCORE, dtw_match_bonus=BONUS, fused_score=bool(fused))
        copt = opt.c_struct()
        r1 = ra.Batch(eng, opt, cb1)
        r1.run()
        r1.fetch()
        h = C.c_void_p()
        eng._check(lib.rawdtw_batch_submit_carry(eng._ctx, C.byref(copt), cb2.n_reads, vp(arr2[0]), vp(arr2[1]), vp(arr2[2]), vp(new_off), vp(new_anchors),
                                                 vp(arr2[3]), vp(arr2[4]), r1._h, vp(carry), C.byref(h)))
        n_jobs = int(np.sum(np.diff(cb2.anchor_off.astype(np.int64)) - 1))
        score, keep, jc = np.zeros(cb2.n_chains, np.float32), np.zeros(cb2.n_chains, np.uint8), np.zeros(n_jobs, np.float32)
        eng._check(lib.rawdtw_batch_fetch(eng._ctx, h, vp(score), vp(keep), vp(jc)))
        sc, ru = C.c_uint64(), C.c_uint64()
        eng._check(lib.rawdtw_batch_round_stats(eng._ctx, h, C.byref(sc), C.byref(ru)))
        lib.rawdtw_batch_destroy(h)
        r1.close()
        assert ru.value == int(carry["parts"].sum())  # the round ran carried, not from scratch
        n_cut, accepted, differs = _check(oracle, cb2, ref, score, keep, jc, fused)
        assert n_cut > 0 and len(accepted) >= 3 and differs > 0
