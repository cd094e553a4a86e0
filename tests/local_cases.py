"""The local border constraint (include/rawdtw.h, "local border"; border_constraint == 2) restated in numpy, the small synthetic mapper case
its tests share, the recorded fixture and a scorer for the Python mirror.  No tests here.

The definition, for a chain with anchors end-first, s = anchors[-1], e = anchors[0]: ONE job over the global branch's windows -- a = the
read's events s.q .. e.q, b = the strand's signals s.t .. e.t --, its cost DTW_semiglobal_slow(a, n, b, m, false) (the sentinel-free
recurrence of tests/semiglobal_cases.model, which ra.semiglobal_host restates in C), the global branch's early exit and final score, and
for the CIGAR DTW_semiglobal_tb's path with every element offset by (s.q, s.t).

tests/golden/local_ref.npz (scripts/make_golden_local.py) holds, for the chains of `make_case()`, the inputs and what the reference's own
compiled DTW_semiglobal_slow and DTW_semiglobal_tb answer on every chain's windows."""
from fractions import Fraction

import numpy as np

import rawalign_amd as ra
from rawalign_amd import synth
from rawalign_amd.align import CandidateBatch
from rawalign_amd.dtw import ANCHOR_DTYPE, JOB_DTYPE, DtwResult
from tests import semiglobal_cases as sc
from tests.golden_util import golden_path

FIXTURE = "local_ref.npz"
LOCAL, GLOBAL = 2, 0
CASE_SEQ_LEN, CASE_READS, CASE_SEED = 1500, 14, 2024
DISPLACE = (0, 2, 3, 5)      # reference positions an end anchor over-reaches by, chain c's start by DISPLACE[c % 4], its end by DISPLACE[(c // 4) % 4]
MODEL_CELLS = 6000           # the numpy recurrence (a Python loop a cell) is run for windows up to this many cells


# ---- arithmetic ----------------------------------------------------------------------------------------------------------------------
def round_f32(x: Fraction) -> np.float32:
    """the float32 nearest an exact value, ties to even"""
    c = np.float32(float(x))
    cands = [c, np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))]
    cands = [v for v in cands if np.isfinite(v)]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(np.float32(v).view(np.uint32)) & 1))


def final_score(n, bonus, cost, fused):
    """rmap.cpp:306: fused, one rounding of n * bonus - cost; else the product rounded, then the difference"""
    n32, b32, c32 = np.float32(n), np.float32(bonus), np.float32(cost)
    if fused:
        return round_f32(Fraction(float(n32)) * Fraction(float(b32)) - Fraction(float(c32)))
    return np.float32(np.float32(n32 * b32) - c32)


# ---- the definition --------------------------------------------------------------------------------------------------------------------
def windows(cb, arena, c):
    """chain c's (a, b, s, e): arena maps a ref_base to its strand's signal array"""
    a0, a1 = int(cb.anchor_off[c]), int(cb.anchor_off[c + 1])
    s, e = cb.anchors[a1 - 1], cb.anchors[a0]
    rb = int(cb.read_base[c])
    a = cb.events[rb + int(s["query_position"]):rb + int(e["query_position"]) + 1]
    b = arena[int(cb.ref_base[c])][int(s["target_position"]):int(e["target_position"]) + 1]
    return a, b, s, e


def jobs(cb):
    """(jobs, job_off): one job a chain with anchors, the global job with band_radius -1 and exclude_last 0"""
    nc = cb.n_chains
    job_off = np.zeros(nc + 1, np.uint64)
    out = []
    for c in range(nc):
        a0, a1 = int(cb.anchor_off[c]), int(cb.anchor_off[c + 1])
        job_off[c] = len(out)
        if a1 == a0:
            continue
        s, e = cb.anchors[a1 - 1], cb.anchors[a0]
        out.append((int(cb.ref_base[c]) + int(s["target_position"]), (int(cb.read_base[c]) + int(s["query_position"])) & 0xFFFFFFFF,
                    (int(e["query_position"]) - int(s["query_position"]) + 1) & 0xFFFFFFFF,
                    (int(e["target_position"]) - int(s["target_position"]) + 1) & 0xFFFFFFFF, -1, 0, 0))
    job_off[nc] = len(out)
    return np.array(out, JOB_DTYPE) if out else np.zeros(0, JOB_DTYPE), job_off


def cost(a, b):
    """the local cost of one window pair: the C restatement, and for small windows the numpy recurrence beside it"""
    c, _ = ra.semiglobal_host(a, b)
    if len(a) * len(b) <= MODEL_CELLS:
        assert sc.bits(c)[0] == sc.bits(sc.model(a, b)[0])[0]
    return np.float32(c)


def global_cost(a, b):
    """the full-matrix global cost (dtw.cpp's DTW_global recurrence: row 0 and column 0 running sums), fp32, a row at a time"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d0 = np.abs(a[0] - b).astype(np.float32)
    prev = np.empty(len(b), np.float32)
    acc = np.float32(0.0)
    for j in range(len(b)):
        acc = np.float32(acc + d0[j]) if j else d0[0]
        prev[j] = acc
    for i in range(1, len(a)):
        di = np.abs(a[i] - b).astype(np.float32)
        cur = np.empty_like(prev)
        cur[0] = prev[0] + di[0]
        best = np.minimum(prev[1:], prev[:-1])   # left and top-left; the top neighbour is sequential
        for j in range(1, len(b)):
            cur[j] = min(best[j - 1], cur[j - 1]) + di[j]
        prev = cur
    return np.float32(prev[-1])


def job_costs(cb, arena):
    """one local cost a chain with anchors, in chain order"""
    return np.array([cost(*windows(cb, arena, c)[:2]) for c in range(cb.n_chains) if cb.anchor_off[c + 1] > cb.anchor_off[c]], np.float32)


def fold(cb, costs, opt):
    """the global branch's early exit and final score, then gen_chains' sequential accept/cut (rmap.cpp:205-209, 306, 515-524): (score, keep)"""
    bonus, min_score = np.float32(opt.dtw_match_bonus), np.float32(opt.dtw_min_score)
    score, keep = np.zeros(cb.n_chains, np.float32), np.zeros(cb.n_chains, np.uint8)
    k = 0
    for r in range(cb.n_reads):
        best = np.float32(0.0)
        for c in range(int(cb.chain_off[r]), int(cb.chain_off[r + 1])):
            a0, a1 = int(cb.anchor_off[c]), int(cb.anchor_off[c + 1])
            if a1 == a0:
                s = np.float32(0.0)
            else:
                n = int(cb.anchors[a0]["query_position"]) - int(cb.anchors[a1 - 1]["query_position"]) + 1
                s = np.float32(-1e10) if np.float32(np.float32(n) * bonus) < best else final_score(n, bonus, costs[k], opt.fused_score)
                k += 1
            score[c] = s
            if s >= min_score:
                keep[c] = 1
                if s > best:
                    best = s
    return score, keep


def cigar(a, b, s):
    """DTW_semiglobal_tb(a, b) with every element offset by the start anchor: (cost, i, j, d, j0, end_j)"""
    (res, end_j) = ra.semiglobal_host(a, b, traceback=True)
    if len(a) * len(b) <= MODEL_CELLS:
        mc_, mej, mi, mj, md = sc.model(a, b)
        assert sc.bits(res.cost)[0] == sc.bits(mc_)[0] and mej == end_j and np.array_equal(mi, res.i) and np.array_equal(mj, res.j)
    return (np.float32(res.cost), res.i.astype(np.uint64) + np.uint64(s["query_position"]), res.j.astype(np.uint64) + np.uint64(s["target_position"]),
            res.difference, int(res.j[0]), int(end_j))


# ---- the shared case -------------------------------------------------------------------------------------------------------------------
class Case:
    """a small synthetic mapper case: one sequence, both strands, CASE_READS reads, and their candidate chains with end anchors displaced
    outwards on the reference by DISPLACE.  ref_base holds VIRTUAL offsets (forward at 0, reverse behind it): `rebased` puts an engine's in."""

    def __init__(self):
        self.ref = synth.make_reference([CASE_SEQ_LEN], seed=CASE_SEED)
        L = len(self.ref.forward[0])
        self.offs = {(0, 1): 0, (0, 0): L}   # (strand 1 selects forward_signals, rmap.cpp:183-188)
        cb, _ = synth.make_candidate_batch(self.ref, self.offs, synth.SynthParams(n_reads=CASE_READS, bases_per_chunk=70, max_chunks=2, decoys_per_read=1.2,
                                                                                 decoy_gap_median=6.0, decoy_gap_max=60), seed=CASE_SEED + 1)
        anchors = cb.anchors.copy()
        for c in range(cb.n_chains):
            a0, a1 = int(cb.anchor_off[c]), int(cb.anchor_off[c + 1])
            ds, de = DISPLACE[c % 4], DISPLACE[(c // 4) % 4]
            anchors[a1 - 1]["target_position"] = max(0, int(anchors[a1 - 1]["target_position"]) - ds)
            anchors[a0]["target_position"] = min(L - 1, int(anchors[a0]["target_position"]) + de)
        self.cb = CandidateBatch(cb.events, cb.chain_off, cb.anchor_off, anchors, cb.ref_base, cb.read_base)
        self.arena = {0: self.ref.forward[0], L: self.ref.reverse[0]}

    def rebased(self, engine):
        """(the batch with the engine's reference offsets, its arena map)"""
        cb, L = self.cb, len(self.ref.forward[0])
        fwd, rev = engine.reference_offset(0, 1), engine.reference_offset(0, 0)
        rb = np.where(cb.ref_base == 0, np.uint64(fwd), np.uint64(rev)).astype(np.uint64)
        return (CandidateBatch(cb.events, cb.chain_off, cb.anchor_off, cb.anchors, rb, cb.read_base), {int(fwd): self.ref.forward[0], int(rev): self.ref.reverse[0]})


_CASE = []


def make_case() -> Case:
    if not _CASE:
        _CASE.append(Case())
    return _CASE[0]


class Fixture:
    """local_ref.npz: the case's arrays, and per chain the bits of DTW_semiglobal_slow and DTW_semiglobal_tb's cost, j0, and the path as
    step bytes (bit 0: i advanced, bit 1: j advanced; the first element's is 0) with its differences"""

    def __init__(self):
        self.z = np.load(golden_path(FIXTURE))

    def same_inputs(self, case):
        z, cb = self.z, case.cb
        return (np.array_equal(z["events"].view(np.uint32), cb.events.view(np.uint32)) and np.array_equal(z["chain_off"], cb.chain_off) and
                np.array_equal(z["anchor_off"], cb.anchor_off) and z["anchors"].tobytes() == np.ascontiguousarray(cb.anchors, ANCHOR_DTYPE).tobytes() and
                np.array_equal(z["ref_base"], cb.ref_base) and np.array_equal(z["read_base"], cb.read_base) and
                np.array_equal(z["forward"].view(np.uint32), case.ref.forward[0].view(np.uint32)) and
                np.array_equal(z["reverse"].view(np.uint32), case.ref.reverse[0].view(np.uint32)))

    def path(self, c):
        """chain c's (i, j, d) inside its window"""
        z = self.z
        o, ln = int(z["path_off"][c]), int(z["path_len"][c])
        st = z["path_step"][o:o + ln]
        return np.cumsum(st & 1, dtype=np.uint64), np.cumsum(st >> 1, dtype=np.uint64) + np.uint64(z["j0"][c]), z["path_d"][o:o + ln]


# ---- the Python mirror's scorer ----------------------------------------------------------------------------------------------------------
class LocalScorer:
    """tests/util.OracleScorer's interface on the restatement above: mapper.map_reads runs the same control flow on the checker"""

    def __init__(self, ref):
        self.ref = ref

    def _arr(self, ch):
        return self.ref.forward[ch.reference_sequence_index] if ch.strand == 1 else self.ref.reverse[ch.reference_sequence_index]

    @staticmethod
    def _window(ch, arr, events):
        s, e = ch.anchors[len(ch.anchors) - 1], ch.anchors[0]
        return (np.ascontiguousarray(events[int(s["query_position"]):int(e["query_position"]) + 1], np.float32),
                np.ascontiguousarray(arr[int(s["target_position"]):int(e["target_position"]) + 1], np.float32), s)

    def score(self, reads, opt, read_keys=None):
        assert opt.dtw_border_constraint == LOCAL
        bonus, min_score = np.float32(opt.dtw_match_bonus), np.float32(opt.dtw_min_score)
        out = []
        for events, chains in reads:
            best, kept = np.float32(0.0), []
            for ch in chains:
                a, b, _ = self._window(ch, self._arr(ch), events)
                s = np.float32(-1e10) if np.float32(np.float32(len(a)) * bonus) < best else final_score(len(a), bonus, cost(a, b), opt.fused_score)
                ch.alignment_score = float(s)
                if s >= min_score:
                    if s > best:
                        best = s
                    kept.append(ch)
            out.append(kept)
        return out

    def callback(self, opt):
        """the same scoring as a rawdtw_mapper_set_scorer callback (CMapper.set_scorer): a scorer-only mapper's rounds on the restatement"""
        def fn(coff, aoff, anch, seq, strand, evs):
            base = np.concatenate([[0], np.cumsum([len(e) for e in evs])]).astype(np.int64)
            events = np.concatenate(list(evs) + [np.zeros(0, np.float32)]).astype(np.float32)
            nc = len(aoff) - 1
            read_of = np.repeat(np.arange(len(coff) - 1), np.diff(coff.astype(np.int64)))
            key = seq.astype(np.uint64) * np.uint64(2) + strand.astype(np.uint64)
            arena = {int(k): (self.ref.forward[int(k) // 2] if int(k) % 2 == 1 else self.ref.reverse[int(k) // 2]) for k in np.unique(key)}
            cb = CandidateBatch(events, coff, aoff, anch, key, base[read_of].astype(np.uint32) if nc else np.zeros(0, np.uint32))
            return fold(cb, job_costs(cb, arena), opt)
        return fn

    def align_cigar(self, chain, read_events, opt):
        a, b, s = self._window(chain, self._arr(chain), read_events)
        c, pi, pj, pd, _, _ = cigar(a, b, s)
        chain.alignment_score = float(final_score(len(a), opt.dtw_match_bonus, c, opt.fused_score))
        chain.dtw_result = DtwResult(c, pi, pj, pd)
        return chain
