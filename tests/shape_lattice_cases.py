"""Every part shape the DTW bodies can meet, at every band radius fraction: the inputs that tests/test_shape_lattice_cpu.py
derives and pins and tests/test_shape_lattice_gpu.py runs.  No tests in here.

A part of n read events and m reference signals has r0 = max(1, int(f32(n) f32(frac))) (rmap.cpp:276) and the slanted radius
R = r0 + ceil((N - M) r0 / N), N the longer side (dtw.cpp:298-300).  The device-planned batch path gives a part with N <= 73
and R <= 3 to a tile (k_runs: quad_dp_r3, lane_dp_r2, lane_dp_r1, lane_dp_gen) and every other part to the side list (k_wide).
The fraction decides which body a shape meets, and the default 0.10 opens little of the space: lane_dp_r1 runs no part longer
than 19 there, radius 3 none longer than 58.

  * the stream lattice: all (n, m) in [1, 80]^2, arranged as chains three ways for a given fraction (sorted, shuffled, singles),
    with a small `peaks` batch whose single chunk a class holds only parts of the class's longest side, and cut into reads of
    short chains over correlated signals for the fold;
  * the job-list lattice: (n, m, R0, exclude_last) with n, m in [1, 100], R0 in 0..9, and bands far wider than the matrix at
    the sizes where the group and micro bodies change."""
import ctypes as C

import numpy as np

import rawalign_amd as ra
from rawalign_amd._lib import AlignOpt
from rawalign_amd.align import CandidateBatch
from rawalign_amd.dtw import JOB_DTYPE
from tests.test_chunk_classes import REF_LEN, _batch

FRACS = (0.01, 0.04, 0.10, 0.25, 0.5, 1.0)
LANE_MAX_N, LANE_MAX_RADIUS = 73, 3   # kLaneMaxN, the tiles' radius limit
STREAM_SIDE = 80
STREAM_LATTICE = [(n, m) for n in range(1, STREAM_SIDE + 1) for m in range(1, STREAM_SIDE + 1)]

# what the issue's enumeration gives, per fraction: (pairs, longest N) of the tile parts of radius 1, 2 and 3, and the side
# list's pairs -- recomputed and asserted by tests/test_shape_lattice_cpu.py
TABLE = {
    0.01: ((73, 73), (5256, 73), (0, 0), 1071),
    0.04: ((49, 49), (3552, 73), (1008, 73), 1791),
    0.10: ((19, 19), (1378, 73), (375, 58), 4628),
    0.25: ((7, 7), (508, 73), (60, 22), 5825),
    0.5: ((3, 3), (218, 73), (15, 10), 6164),
    1.0: ((1, 1), (73, 73), (4, 4), 6322),
}
N_TILE_RECORDS = 6832   # distinct (N, M, R, swapped) over FRACS


def r0_of(n, frac):
    """rmap.cpp:276: the product in fp32, truncated; at least 1"""
    return max(1, int(np.float32(n) * np.float32(frac)))


def radius(n, m, frac):
    r0, N, M = r0_of(n, frac), max(n, m), min(n, m)
    return r0 + ((N - M) * r0 + N - 1) // N


def tile_record(n, m, frac):
    """(N, M, R, swapped) of a tile part -- what a pass's job record holds -- or None for a part of the side list"""
    N, M, R = max(n, m), min(n, m), radius(n, m, frac)
    return (N, M, R, int(n < m)) if N <= LANE_MAX_N and R <= LANE_MAX_RADIUS else None


def table_row(frac):
    """((pairs, longest N) for R = 1, 2, 3, side-list pairs) over the stream lattice"""
    per = {1: [0, 0], 2: [0, 0], 3: [0, 0]}
    side = 0
    for n, m in STREAM_LATTICE:
        t = tile_record(n, m, frac)
        if t is None:
            side += 1
        else:
            per[t[2]][0] += 1
            per[t[2]][1] = max(per[t[2]][1], t[0])
    return tuple(tuple(per[r]) for r in (1, 2, 3)) + (side,)


# ------------------------------------------------------------------------------------------------------------------------
# the job-list lattice
# ------------------------------------------------------------------------------------------------------------------------
JOB_SIDE, JOB_ARENA = 100, 4096
WIDE_SIDES = (1, 2, 7, 8, 9, 63, 64, 65, 100)
# the knob sets of the job-list runs; "device_plan" is the context's choice of path, not the planner's: the dry run has no such option
KNOB_SETS = [{}, {"micro_max_n": 0}, {"micro_max_n": 4}, {"grp8": 0}, {"grp16": 0}, {"lane_max_radius": 1}, {"lane_hi": 1}, {"lane_max_n": 20},
             {"device_plan": 0}]


def knob_id(k):
    return "-".join(f"{a}{b}" for a, b in k.items()) or "default"


def job_lattice():
    """(jobs, events, ref): ref_off relative to `ref`; windows drawn over two arenas of JOB_ARENA normal values"""
    s = np.arange(1, JOB_SIDE + 1)
    n, m, r0, ex = (x.ravel() for x in np.meshgrid(s, s, np.arange(10), np.arange(2), indexing="ij"))
    wide = [(a, b, r, e) for a in WIDE_SIDES for b in WIDE_SIDES for r in (a, a + b, 200) for e in (0, 1)]
    wn, wm, wr, we = (np.array(x) for x in zip(*wide))
    n, m, r0, ex = np.concatenate([n, wn]), np.concatenate([m, wm]), np.concatenate([r0, wr]), np.concatenate([ex, we])
    rng = np.random.default_rng(100)
    jobs = np.zeros(len(n), JOB_DTYPE)
    jobs["n"], jobs["m"], jobs["band_radius"], jobs["exclude_last"] = n, m, r0, ex
    jobs["read_off"] = (rng.random(len(n)) * (JOB_ARENA - n + 1)).astype(np.int64)
    jobs["ref_off"] = (rng.random(len(n)) * (JOB_ARENA - m + 1)).astype(np.int64)
    return jobs, rng.normal(size=JOB_ARENA).astype(np.float32), rng.normal(size=JOB_ARENA).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# the stream lattice's arrangements: lists of batches, a batch = (chains, chains a read or None for one read); a chain =
# its parts (n, m) in anchor-list order, as tests/test_chunk_classes.py:_batch takes them
# ------------------------------------------------------------------------------------------------------------------------
CHAIN_PARTS = 500
SORTED_OPTS = {"tile_lds_floats": 16384, "pass_pool": 4096}   # a tile of 512 parts of N = 73 fits five passes; slots for all of them
SINGLES_OPTS = {"pass_pool": 4096}                            # a chain a part = a run a part: 32 parts a pass


def _cut(parts, size=CHAIN_PARTS):
    return [parts[k:k + size] for k in range(0, len(parts), size)]


def sorted_parts(frac):
    """tile parts first, then the side list's; each by radius, then by the longer side, descending"""
    def key(p):
        t = tile_record(p[0], p[1], frac)
        return (t is None, radius(p[0], p[1], frac), -max(p), p)
    return sorted(STREAM_LATTICE, key=key)


def shuffled_parts(frac):
    rng = np.random.default_rng(int(round(frac * 100)))
    return [STREAM_LATTICE[i] for i in rng.permutation(len(STREAM_LATTICE))]


def peak_parts(frac):
    """per radius the lattice reaches: up to eight tile parts of the table's longest side (one chunk a class in one pass)"""
    out = []
    for R in (1, 2, 3):
        longest = TABLE[frac][R - 1][1]
        out.append([p for p in STREAM_LATTICE if (tile_record(p[0], p[1], frac) or (0, 0, 0))[2] == R and max(p) == longest][:8])
    return [c for c in out if c]


def arrangement(name, frac):
    if name == "sorted":   # batches of six chains: the side list holds min(na, na / 4 + 4096) parts of a batch of na anchors, and at 0.25 and
        chains = _cut(sorted_parts(frac))   # above more of the lattice than that is the side list's ("sorted_whole": declined)
        return [(chains[k:k + 6], None) for k in range(0, len(chains), 6)]
    if name == "sorted_whole":
        return [(_cut(sorted_parts(frac)), None)]
    if name == "shuffled":   # two batches: the default pool of pass slots (4 a tile + 64) holds either half's passes
        p = shuffled_parts(frac)
        h = len(p) // 2
        return [(_cut(p[:h]), None), (_cut(p[h:]), None)]
    if name == "singles":
        return [([[p] for p in shuffled_parts(frac)], 100)]
    if name == "peaks":
        return [(peak_parts(frac), None)]
    raise KeyError(name)


ARRANGEMENT_OPTS = {"sorted": SORTED_OPTS, "sorted_whole": SORTED_OPTS, "shuffled": {}, "singles": SINGLES_OPTS, "peaks": {}}


def fold_chains(frac):
    """the shuffled lattice cut into chains of 1..120 parts, reads of 3..12 chains: (chains, chain_off)"""
    rng = np.random.default_rng(1000 + int(round(frac * 100)))
    p = shuffled_parts(frac)
    chains, at = [], 0
    while at < len(p):
        k = int(rng.integers(1, 121))
        chains.append(p[at:at + k])
        at += k
    off = [0]
    while off[-1] < len(chains):
        off.append(min(len(chains), off[-1] + int(rng.integers(3, 13))))
    return chains, np.array(off, np.uint64)


def reference():
    rng = np.random.default_rng(20240611)
    return [rng.normal(size=REF_LEN).astype(np.float32), rng.normal(size=REF_LEN).astype(np.float32)]


REF_PAD = (REF_LEN + 3) & ~3
REF_OFFSET = {1: 0, 0: REF_PAD}   # Engine.reference_offset(0, strand) after upload_reference of one sequence (asserted on the GPU)


def reference_arena(ref):
    arena = np.zeros(2 * REF_PAD, np.float32)
    arena[:REF_LEN], arena[REF_PAD:REF_PAD + REF_LEN] = ref[0], ref[1]
    return arena


class Case:
    """a batch's arrays: the CandidateBatch, every chain's strand, and the strand arrays"""

    def __init__(self, cb, strand_of, ref):
        self.cb, self.strand_of, self.ref = cb, strand_of, ref
        self.ref_arrays = {1: ref[0], 0: ref[1]}


def make_case(chains, ref, chains_per_read=None, chain_off=None, events=None, read_base=None):
    ev, c_off, anchor_off, anchors, slot, rbase = _batch(chains)
    if chains_per_read:
        c_off = np.array(list(range(0, len(chains), chains_per_read)) + [len(chains)], np.uint64)
    if chain_off is not None:
        c_off = np.asarray(chain_off, np.uint64)
    strand_of = [1 if s == 0 else 0 for s in slot]   # slot 0 = forward array (strand 1, rmap.cpp:182-188)
    ref_base = np.array([REF_OFFSET[st] for st in strand_of], np.uint64)
    cb = CandidateBatch(ev if events is None else events, c_off, anchor_off, anchors, ref_base, rbase if read_base is None else read_base)
    return Case(cb, strand_of, ref)


def expected_parts(chains, frac):
    """(n, m, r0, exclude_last) of every part in job order (rmap.cpp:251-276: from the chain's start, i.e. the list backwards;
    every part but the chain's last leaves its last cell out)"""
    rows = [(n, m, r0_of(n, frac), int(i != 0)) for parts in chains for i, (n, m) in reversed(list(enumerate(parts)))]
    return tuple(np.array(x, np.int64) for x in zip(*rows))


# ------------------------------------------------------------------------------------------------------------------------
# the fold cases' signals
# ------------------------------------------------------------------------------------------------------------------------
NOISE = (0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.55, 0.8, 1.1)   # per chain, by a seeded draw: the chains of a read differ in score
FOLD_FRACS = (0.04, 0.25)
FOLD_PARAMS = [(b, s, f) for b in (0.4, 0.6) for s in (-1e9, 5.0, 60.0) for f in (True, False)]


def fold_reference():
    """the fold cases' strand arrays: normal noise under a 64-sample Hann window, unit variance -- neighbours differ by a few
    hundredths, so that a window resampled to a very different length (n = 80 on m = 3) still aligns at a small cost and the
    chain's noise level decides its score"""
    rng = np.random.default_rng(20240612)
    w = np.hanning(64)
    out = []
    for _ in range(2):
        x = np.convolve(rng.normal(size=REF_LEN + 63), w, mode="valid")
        out.append((x / x.std()).astype(np.float32))
    return out


def fold_cases(frac, ref):
    """[(Case, chains)]: the fraction's reads in two batches (at 0.25 the side list's parts of the whole lattice are more than a batch's
    side list holds).  Every chain reads events of its own: its reference windows (`ref`: fold_reference()) resampled part by
    part to the part's n (linear interpolation; consecutive parts share their anchor's event), plus normal noise of the chain's level"""
    chains, chain_off = fold_chains(frac)
    off = chain_off.astype(np.int64)
    r_mid = (len(off) - 1) // 2
    out = []
    for half, (r0, r1) in enumerate(((0, r_mid), (r_mid, len(off) - 1))):
        sub = chains[off[r0]:off[r1]]
        out.append((_fold_case(sub, off[r0:r1 + 1] - off[r0], ref, 77 + 2 * int(round(frac * 100)) + half), sub))
    return out


def _fold_case(chains, chain_off, ref, seed):
    base = make_case(chains, ref, chain_off=chain_off)
    cb = base.cb
    rng = np.random.default_rng(seed)
    events, read_base = [], []
    at = 0
    level = []   # every other read takes its levels loudest first: its scores tend to rise chain by chain, and the running best with them
    for r in range(cb.n_reads):
        lv = rng.integers(0, len(NOISE), int(cb.chain_off[r + 1]) - int(cb.chain_off[r]))
        level += list(np.sort(lv)[::-1] if r % 2 == 0 else lv)
    for c in range(cb.n_chains):
        a = cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])]
        arr = base.ref_arrays[base.strand_of[c]]
        q, t = a["query_position"].astype(np.int64)[::-1], a["target_position"].astype(np.int64)[::-1]   # ascending
        ev = np.zeros(int(q[-1]) + 1, np.float64)
        ev[:int(q[0])] = rng.normal(size=int(q[0]))
        for k in range(len(q) - 1):
            n, m = int(q[k + 1] - q[k]) + 1, int(t[k + 1] - t[k]) + 1
            x = np.linspace(0.0, m - 1.0, n) if n > 1 else np.zeros(1)
            ev[q[k]:q[k] + n] = np.interp(x, np.arange(m), arr[t[k]:t[k] + m])
        ev += rng.normal(size=len(ev)) * NOISE[int(level[c])]
        events.append(ev.astype(np.float32))
        read_base.append(at)
        at += len(ev)
    cb = CandidateBatch(np.concatenate(events), cb.chain_off, cb.anchor_off, cb.anchors, cb.ref_base, np.array(read_base, np.uint32))
    return Case(cb, base.strand_of, ref)


# ------------------------------------------------------------------------------------------------------------------------
# expectations
# ------------------------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def build_jobs(lib, cb, opt):
    """rawdtw_batch_build_jobs on a CandidateBatch: (jobs, job_off); no device"""
    copt = opt.c_struct() if hasattr(opt, "c_struct") else opt
    a = [np.ascontiguousarray(cb.anchor_off, np.uint64), np.ascontiguousarray(cb.anchors, ra.ANCHOR_DTYPE),
         np.ascontiguousarray(cb.ref_base, np.uint64), np.ascontiguousarray(cb.read_base, np.uint32)]
    job_off = np.zeros(cb.n_chains + 1, np.uint64)
    nj = C.c_uint64()
    assert lib.rawdtw_batch_build_jobs(C.byref(copt), cb.n_chains, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(job_off), None, 0, C.byref(nj)) == 0
    jobs = np.zeros(nj.value, JOB_DTYPE)
    assert lib.rawdtw_batch_build_jobs(C.byref(copt), cb.n_chains, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(job_off), _p(jobs), len(jobs),
                                       C.byref(nj)) == 0
    return jobs, job_off


def oracle_expect(oracle, case, jobs, opt, arena=None, threads=8):
    """(score, keep, part costs) as the reference computes them: the parts' costs in one oracle.batch_costs call on the library's job
    list, the chains by oracle.align_chain under the read's running best (gen_chains, rmap.cpp:515-524)"""
    from oracle.loader import OrcOpt

    cb = case.cb
    arena = reference_arena(case.ref) if arena is None else arena
    costs = oracle.batch_costs(jobs, cb.events, arena, nthreads=threads)
    oopt = OrcOpt(1, 1, opt.dtw_band_radius_frac, opt.dtw_match_bonus, opt.dtw_min_score, int(opt.fused_score))
    score, keep = np.zeros(cb.n_chains, np.float32), np.zeros(cb.n_chains, np.uint8)
    for r in range(cb.n_reads):
        best = np.float32(0.0)
        for c in range(int(cb.chain_off[r]), int(cb.chain_off[r + 1])):
            a = cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])]
            s = oracle.align_chain(a, case.ref_arrays[case.strand_of[c]], cb.events[int(cb.read_base[c]):], oopt, float(best))
            score[c] = s
            keep[c] = s >= np.float32(opt.dtw_min_score)
            if keep[c] and s > best:
                best = s
    return score, keep, costs


def full_fold(oracle, case, opt):
    """every chain's score with no cut at all (align_chain's own default for its bound, -1e10)"""
    from oracle.loader import OrcOpt

    cb = case.cb
    oopt = OrcOpt(1, 1, opt.dtw_band_radius_frac, opt.dtw_match_bonus, opt.dtw_min_score, int(opt.fused_score))
    return np.array([oracle.align_chain(cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])], case.ref_arrays[case.strand_of[c]],
                                        cb.events[int(cb.read_base[c]):], oopt) for c in range(cb.n_chains)], np.float32)


def align_opt(frac, bonus=0.4, min_score=5.0, fused=True):
    return AlignOpt(1, 1, frac, bonus, min_score, int(fused))
