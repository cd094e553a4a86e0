"""Inputs of tests/test_batch_replay_gpu.py and tests/test_launch_options_gpu.py (no tests here): candidate batches with two sets of
arena contents -- "A", the one a batch is created over, and "B", fresh draws of the same lengths that a replay reads -- and what the
oracle makes of each, taken once a session.

A case's check() holds a fetched (score, keep, part costs) to the oracle value by value the first time it sees an (events, reference)
pair (tests/test_stream_path.py's _oracle_check: dtw.cpp:273-520 a part, rmap.cpp:248-306 a chain, rmap.cpp:515-524 a read), keeps
the arrays that passed, and holds every later result of that pair to those arrays, uint32 view against uint32 view.  So the oracle
runs once a pair, and every test compares against the same, unchanged reference."""
import functools

import numpy as np

import rawalign_amd as ra
from rawalign_amd.align import CandidateBatch
from tests.test_stream_path import _chains, _medium, _oracle_check, _sprinkled, _tiny, _wide
from tests.util import oracle_costs


def same_bits(got, want, what=""):
    """(score, keep, part costs) against (score, keep, part costs): no tolerance"""
    for name, g, w in zip(("score", "keep", "part cost"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        gv, wv = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        bad = np.nonzero(gv != wv)[0]
        assert len(bad) == 0, f"{what}: {len(bad)} of {len(g)} {name}s differ, first at {bad[:5]}: got {g[bad[:5]]} want {w[bad[:5]]}"


class SparseCase:
    """120 reads of sparse + banded chains over one sequence's two strand arrays"""

    min_score = 5.0

    def __init__(self, shapes, seed, n_reads=120, parts_range=(1, 40), ref_len=60000):
        rng = np.random.default_rng(seed)
        self.ref = {"A": [rng.normal(size=ref_len).astype(np.float32) for _ in range(2)]}
        events, self.chain_off, self.anchor_off, self.anchors, slot, self.read_base = _chains(rng, n_reads, ref_len, shapes, parts_range)
        self.strand_of = [1 if s == 0 else 0 for s in slot]  # slot 0 = forward array (strand 1, rmap.cpp:182-188)
        self.events = {"A": events, "B": rng.normal(size=len(events)).astype(np.float32)}
        self.ref["B"] = [rng.normal(size=ref_len).astype(np.float32) for _ in range(2)]
        self.opt = ra.MapOpt(dtw_min_score=self.min_score)
        self.accepted = {}

    def engine(self, **options):
        """a fresh context with `options` set and the A arenas uploaded"""
        eng = ra.Engine(0)
        for k, v in options.items():
            eng.set_option(k, v)
        self.upload(eng, "A", "A", first=True)
        return eng

    def upload(self, eng, ev, ref=None, first=False):
        if ref is not None:
            before = None if first else [eng.reference_offset(0, st) for st in (0, 1)]
            eng.upload_reference([self.ref[ref][0]], [self.ref[ref][1]])
            assert before is None or before == [eng.reference_offset(0, st) for st in (0, 1)]  # (same lengths: the batch's ref_base still hold)
        eng.upload_events(self.events[ev])

    def candidate_batch(self, eng, ev="A"):
        ref_base = np.array([eng.reference_offset(0, st) for st in self.strand_of], np.uint64)
        return CandidateBatch(self.events[ev], self.chain_off, self.anchor_off, self.anchors, ref_base, self.read_base)

    def batch(self, eng, **kw):
        return ra.Batch(eng, self.opt, self.candidate_batch(eng), **kw)

    def check(self, oracle, got, ev, ref="A", what="", jobs=None):
        key = (ev, ref)
        if key in self.accepted:
            same_bits(got, self.accepted[key], f"{what} {key}")
            return
        score, keep, jc = got
        cb = CandidateBatch(self.events[ev], self.chain_off, self.anchor_off, self.anchors, None, self.read_base)
        _oracle_check(oracle, cb, {1: self.ref[ref][0], 0: self.ref[ref][1]}, self.strand_of, score, keep, jc, self.opt)
        self.accepted[key] = tuple(np.array(x, copy=True) for x in got)

    def costs_differ_everywhere(self, key_a, key_b):
        """the oracle's part costs under two arena contents share no value at any index: a cost left over from one cannot pass for the
        other (a chain's score is cut to -1e10 under either when it cannot reach the read's best, rmap.cpp:265-268: scores may coincide)"""
        ja, jb = self.accepted[key_a][2], self.accepted[key_b][2]
        assert len(ja) > 0 and np.all(ja.view(np.uint32) != jb.view(np.uint32)), np.nonzero(ja.view(np.uint32) == jb.view(np.uint32))[0][:8]
        return True

    def costs_mostly_differ(self, key_a, key_b):
        """two event sets over ONE reference: a part whose event lies between two reference values under both costs the same under both
        (|e - r0| + |e - r1| = r1 - r0), the others differ -- a replay that left a launch's worth of costs behind still cannot pass"""
        ja, jb = self.accepted[key_a][2], self.accepted[key_b][2]
        assert len(ja) > 0 and np.count_nonzero(ja.view(np.uint32) != jb.view(np.uint32)) >= 0.99 * len(ja)
        return True


class FullCase:
    """48 reads of the synthetic mapper batch, border constraint global, fill method full: one full-matrix job a chain (rmap.cpp:220-246)"""

    def __init__(self, n_reads=48):
        from rawalign_amd import synth

        self.sref = synth.make_reference([120000], seed=77)
        self.n_reads = n_reads
        self.opt = ra.MapOpt(dtw_border_constraint=0, dtw_fill_method=0)
        self._cb = None
        self.accepted = {}

    def engine(self, **options):
        from rawalign_amd import synth

        eng = ra.Engine(0)
        for k, v in options.items():
            eng.set_option(k, v)
        eng.upload_reference(self.sref.forward, self.sref.reverse)
        self.offs = {(0, st): eng.reference_offset(0, st) for st in (0, 1)}
        if self._cb is None:
            self._cb, _ = synth.make_candidate_batch(self.sref, self.offs, synth.SynthParams(n_reads=self.n_reads, max_chunks=3, decoys_per_read=3.0), seed=1234)
            rng = np.random.default_rng(4321)
            self.events = {"A": self._cb.events, "B": rng.normal(size=len(self._cb.events)).astype(np.float32)}
        eng.upload_events(self.events["A"])
        return eng

    def upload(self, eng, ev, ref=None):
        assert ref in (None, "A")
        eng.upload_events(self.events[ev])

    def batch(self, eng, **kw):
        return ra.Batch(eng, self.opt, self._cb, **kw)

    def check(self, oracle, got, ev, ref="A", what="", jobs=None):
        from oracle.loader import OrcOpt
        from tests.golden_util import bits

        key = (ev, ref)
        if key in self.accepted:
            same_bits(got, self.accepted[key], f"{what} {key}")
            return
        score, keep, jc = got
        cb, events = self._cb, self.events[ev]
        arena = np.zeros(max(self.offs.values()) + len(self.sref.forward[0]), np.float32)
        arena[self.offs[(0, 1)]:][:len(self.sref.forward[0])] = self.sref.forward[0]
        arena[self.offs[(0, 0)]:][:len(self.sref.reverse[0])] = self.sref.reverse[0]
        want_jc = oracle_costs(oracle, jobs, events, arena)  # (DTW_global, dtw.cpp:37-66, a job)
        same_bits((jc,), (want_jc,), f"{what} {key} job costs against the oracle")
        oopt = OrcOpt(0, 0, self.opt.dtw_band_radius_frac, self.opt.dtw_match_bonus, self.opt.dtw_min_score, 1)
        arrays = {self.offs[(0, 1)]: self.sref.forward[0], self.offs[(0, 0)]: self.sref.reverse[0]}
        for r in range(cb.n_reads):
            best = np.float32(0.0)
            for c in range(int(cb.chain_off[r]), int(cb.chain_off[r + 1])):
                a = cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])]
                want = oracle.align_chain(a, arrays[int(cb.ref_base[c])], events[int(cb.read_base[c]):], oopt, float(best))
                assert bits(score[c]) == bits(want), (r, c, score[c], want)
                k = want >= np.float32(self.opt.dtw_min_score)
                assert bool(keep[c]) == bool(k)
                if k and want > best:
                    best = want
        self.accepted[key] = tuple(np.array(x, copy=True) for x in got)

    def costs_differ_everywhere(self, key_a, key_b):
        ja, jb = self.accepted[key_a][2], self.accepted[key_b][2]
        assert len(ja) > 0 and np.all(ja.view(np.uint32) != jb.view(np.uint32))
        return True


@functools.lru_cache(maxsize=None)
def random_job_cases():
    """the 3 000 jobs of test_planner_options_do_not_change_results: (a, b, band_radius, exclude_last) with the default radius of the
    read side three times in four and a radius of 0 .. 11 otherwise (every radius class of the planner), exclude_last alternating"""
    from tests.util import default_radius

    rng = np.random.default_rng(21)
    cases = []
    for t in range(3000):
        n = int(rng.integers(1, 110))
        m = max(1, int(round(n * rng.uniform(0.4, 1.5))))
        R0 = default_radius(n) if t % 4 else int(rng.integers(0, 12))
        cases.append((rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32), R0, t & 1))
    return cases


def _job_shapes():
    """parts of those jobs' shapes, one after the other (a part of n events holds n - 1 steps; at least one)"""
    sizes = [(max(1, len(a) - 1), max(1, len(b) - 1)) for a, b, _, _ in random_job_cases()]
    state = {"k": -1}

    def shapes(rng):
        state["k"] += 1
        return sizes[state["k"] % len(sizes)]
    return shapes


@functools.lru_cache(maxsize=None)
def case(name):
    """the session's one instance of a case: its oracle results are shared by every test that names it"""
    if name == "job_shapes":
        return SparseCase(_job_shapes(), 104)
    if name == "queue":  # some 120 000 tiny parts: several hundred passes when the tiles' image is small
        return SparseCase(_tiny, 105, n_reads=1500, parts_range=(20, 60), ref_len=200000)
    if name == "tiny":  # (radius 1 or 2 after the slant: nothing for the side list)
        return SparseCase(_tiny, 106)
    if name == "sprinkled":
        return SparseCase(_sprinkled, 101)
    if name == "wide":
        return SparseCase(_wide, 102)
    if name == "medium":
        return SparseCase(_medium, 103)
    if name == "full":
        return FullCase()
    raise KeyError(name)


def slanted_radius(n, m, r0):
    """dtw.cpp:298-300"""
    N, M = max(n, m), min(n, m)
    return r0 + ((N - M) * r0 + N - 1) // N


def expected_counts(oracle, jobs, tile_radius=None, tile_max_n=None):
    """(jobs, cells) of a job list as test_dry_run_cells_match_oracle counts them -- oracle.banded_cells a banded job, n * m a full one --
    and, with the tile class's limits given, the same pair for the jobs outside that class (the side list of a device-planned batch)"""
    n_all = c_all = n_side = c_side = 0
    for j in jobs:
        n, m, r0 = int(j["n"]), int(j["m"]), int(j["band_radius"])
        c = n * m if r0 < 0 else oracle.banded_cells(n, m, r0)
        n_all += 1
        c_all += c
        if tile_radius is not None and not (slanted_radius(n, m, r0) <= tile_radius and max(n, m) <= tile_max_n):
            n_side += 1
            c_side += c
    return (n_all, c_all) if tile_radius is None else (n_all, c_all, n_side, c_side)
