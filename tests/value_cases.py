"""Seeded inputs beyond unit scale for every DTW body, and a batch whose accept/cut comparisons meet equality.

Value domains (one `draw(rng, size) -> float32` each).  The reference's banded DP (src/dtw.cpp:273-520) puts a literal 1e10
into every guarded or clipped neighbour; its full DPs (dtw.cpp:37-66, 595-667) have no sentinel.  Inputs of unit scale never
produce a cost near 1e10, a subnormal or a score on a threshold, so they cannot tell a body that keeps the reference's
operands from one that does not:
  s9 .. s30        normal * scale: costs below, around and far above the fill value (the largest stay finite over the
                   largest shape a test uses: tests assert it with `sums_stay_finite`)
  cross            normal * 3e8: costs pass 1e10 in the middle of a matrix of some tens of cells a side
  spike            normal, one element in sixteen replaced by +-uniform(1e9, 1e11)
  sub38 .. sub44   normal * 1e-38 / 1e-41 / 1e-44: inputs, distances and sums are subnormal
  zeros            constant windows of +0.0 and -0.0 mixed: every cost is +0.0
  ints             integers in {-2..2}: exact arithmetic, ties everywhere
tests/golden/dtw_ref_values.npz (scripts/make_golden_values.py) records the compiled reference's answers for `fixture_cases`
and the SHA-256 of those inputs, so a generator that drifts fails loudly.

The threshold batch (`threshold_batch`): integer signals and a match bonus of 0.5 make all of align_chain's arithmetic
(src/rmap.cpp:181-313) exact, so its three comparisons -- gate < best (rmap.cpp:206/265), score >= min_score (518),
score > best (519) -- meet equality often; `threshold_model` recomputes them in plain Python."""
import hashlib

import numpy as np

SCALES = {"s9": 1e9, "s3e9": 3e9, "s10": 1e10, "s12": 1e12, "s30": 1e30, "cross": 3e8, "sub38": 1e-38, "sub41": 1e-41, "sub44": 1e-44}


def _scaled(scale):
    def draw(rng, size):
        return (rng.normal(size=size) * scale).astype(np.float32)
    return draw


def _spike(rng, size):
    x = rng.normal(size=size)
    big = rng.uniform(1e9, 1e11, size=size) * rng.choice([-1.0, 1.0], size=size)
    return np.where(rng.integers(0, 16, size=size) == 0, big, x).astype(np.float32)


def _zeros(rng, size):
    return np.where(rng.integers(0, 2, size=size) == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)


def _ints(rng, size):
    return rng.integers(-2, 3, size=size).astype(np.float32)


DOMAINS = {name: _scaled(s) for name, s in SCALES.items()}
DOMAINS.update(spike=_spike, zeros=_zeros, ints=_ints)
DOMAIN_NAMES = ("s9", "s3e9", "s10", "s12", "s30", "cross", "spike", "sub38", "sub41", "sub44", "zeros", "ints")
assert sorted(DOMAIN_NAMES) == sorted(DOMAINS)
SENTINEL_DOMAINS = ("s3e9", "s10", "s12", "s30")  # scales >= 3e9: the sensitivity conditions of tests/test_value_domain.py


def domain_rng(name, salt=0):
    """a generator of its own for every (domain, use): adding a domain or a test moves no other's inputs"""
    return np.random.default_rng([DOMAIN_NAMES.index(name), salt, 20251])


def sums_stay_finite(arrays, n, m):
    """every cell of an n x m matrix is a sum of at most n + m - 1 distances, each at most twice the largest magnitude"""
    top = max(float(np.max(np.abs(x))) if len(x) else 0.0 for x in arrays)
    return (n + m) * 2.0 * top < float(np.finfo(np.float32).max)


FIXED_RADII = (0, 1, 2, 4, 8)
N_FIXTURE_CASES = 150
TB_EVERY = 3


def fixture_cases(name):
    """[(a, b, exclude_last)]: sides 1..60, the other side 0.4 .. 1.6 times the first (clipped to 1..60)"""
    rng = domain_rng(name)
    draw = DOMAINS[name]
    out = []
    for t in range(N_FIXTURE_CASES):
        n = int(rng.integers(1, 61))
        m = min(60, max(1, int(round(n * rng.uniform(0.4, 1.6)))))
        out.append((draw(rng, n), draw(rng, m), t & 1))
    return out


def fixture_radii(n):
    """the radii recorded for a case whose read side is n: rmap.cpp:214,276's default first, then the fixed ones"""
    return (max(1, int(np.float32(n) * np.float32(0.1))),) + FIXED_RADII


def inputs_sha256(all_cases) -> bytes:
    h = hashlib.sha256()
    for name in DOMAIN_NAMES:
        h.update(name.encode())
        for a, b, ex in all_cases[name]:
            h.update(np.array([len(a), len(b), ex], "<i8").tobytes())
            h.update(np.ascontiguousarray(a, "<f4").tobytes())
            h.update(np.ascontiguousarray(b, "<f4").tobytes())
    return h.digest()


# ------------------------------------------------------------------------------------------------
# thresholds met exactly
# ------------------------------------------------------------------------------------------------
THRESHOLD_SEED = 7
THRESHOLD_BONUS = 0.5
THRESHOLD_MIN_SCORE = 20.0
ANCHOR_DTYPE = np.dtype([("target_position", "<u4"), ("query_position", "<u4")])  # rawdtw_anchor_t


def threshold_batch(n_reads=600, seed=THRESHOLD_SEED):
    """600 reads of four chains.  Events in {-2..2}; a chain's anchors lie on the diagonal (query and target advance by the
    same 2..6), 8..15 parts; its stretch of the reference is a copy of its events with 0..7 errors of +-1.  Returns
    (events, ref, chain_off, anchor_off, anchors, read_base): every chain on the one reference array, end-first anchors."""
    rng = np.random.default_rng(seed)
    events, ref, chain_off, anchor_off, anchors, read_base = [], [], [0], [0], [], []
    ev_at = ref_at = 0
    for _ in range(n_reads):
        per, read_len = [], 0
        for _ in range(4):
            parts = int(rng.integers(8, 16))
            q = int(rng.integers(0, 5)) + np.concatenate([[0], np.cumsum(rng.integers(2, 7, parts))]).astype(np.int64)
            per.append(q)
            read_len = max(read_len, int(q[-1]) + 1)
        ev = _ints(rng, read_len)
        for q in per:
            seg = ev[int(q[0]):int(q[-1]) + 1].copy()
            for _ in range(int(rng.integers(0, 8))):
                seg[int(rng.integers(0, len(seg)))] += np.float32(rng.choice([-1.0, 1.0]))
            a = np.zeros(len(q), ANCHOR_DTYPE)
            a["query_position"] = q[::-1]
            a["target_position"] = (ref_at + q - q[0])[::-1]
            anchors.append(a)
            anchor_off.append(anchor_off[-1] + len(a))
            read_base.append(ev_at)
            ref.append(seg)
            ref_at += len(seg)
        chain_off.append(len(anchor_off) - 1)
        events.append(ev)
        ev_at += read_len
    return (np.concatenate(events), np.concatenate(ref), np.array(chain_off, np.uint64), np.array(anchor_off, np.uint64),
            np.concatenate(anchors), np.array(read_base, np.uint32))


def threshold_part_costs(oracle, batch, frac=0.1):
    """per chain, the costs of its parts in the order align_chain issues them (chain start first; every part but the last
    without its last cell's distance: rmap.cpp:270-277)"""
    events, ref, chain_off, anchor_off, anchors, read_base = batch
    out = []
    for c in range(len(anchor_off) - 1):
        a = anchors[int(anchor_off[c]):int(anchor_off[c + 1])]
        ev = events[int(read_base[c]):]
        parts = len(a) - 1
        costs = []
        for p in range(parts):
            s, e = a[parts - p], a[parts - p - 1]
            n = int(e["query_position"]) - int(s["query_position"]) + 1
            m = int(e["target_position"]) - int(s["target_position"]) + 1
            R0 = max(1, int(np.float32(n) * np.float32(frac)))
            costs.append(oracle.dtw_banded(ev[int(s["query_position"]):int(s["query_position"]) + n],
                                           ref[int(s["target_position"]):int(s["target_position"]) + m], R0, p != parts - 1))
        out.append(np.array(costs, np.float32))
    return out


def threshold_model(batch, part_costs, bonus=THRESHOLD_BONUS, min_score=THRESHOLD_MIN_SCORE):
    """The accept/cut loop in plain Python floats (every value is a multiple of 0.5 far below 2^24: float64 is exact, and so
    is float32, fused or not).  Per chain: dict(gate, best, cut, score, keep) -- `gate` what is attainable before the last
    DTW call (the smallest value rmap.cpp:265 tests: costs are not negative), `best` the running best it is tested against."""
    events, ref, chain_off, anchor_off, anchors, read_base = batch
    out = []
    for r in range(len(chain_off) - 1):
        best = 0.0
        for c in range(int(chain_off[r]), int(chain_off[r + 1])):
            a = anchors[int(anchor_off[c]):int(anchor_off[c + 1])]
            q = [int(x) for x in a["query_position"]]
            costs = [float(x) for x in part_costs[c]]
            assert all(x == int(x) and x >= 0 for x in costs) and len(costs) == len(q) - 1
            attainable = (q[0] - q[-1] + 1) * bonus
            gate = attainable - sum(costs[:-1])
            cut, total, aligned = False, 0.0, 0
            parts = len(q) - 1
            for p in range(parts):
                if attainable < best:
                    cut = True
                    break
                total += costs[p]
                attainable -= costs[p]
                aligned += q[parts - p - 1] - q[parts - p] + 1
            score = -1e10 if cut else aligned * bonus - total
            keep = score >= min_score
            out.append({"gate": gate, "best": best, "cut": cut, "score": score, "keep": keep})
            if keep and score > best:
                best = score
    return out
