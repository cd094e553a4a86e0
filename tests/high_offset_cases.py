"""Arena offsets past 2^30, 2^31 and 2^32: the builder that tests/test_high_offsets_cpu.py pins and tests/test_high_offsets_gpu.py runs.
No tests here; nothing here needs a device or builds anything of an arena's size on the host.

Two arenas, REF_FLOATS and EV_FLOATS long, hold one finite constant (FILL) and a few copies of one small SEGMENT each (`ref_segment`,
`ev_segment`).  A PLACE is where a copy's first float goes: offset 0, one copy that straddles 2^30, one that straddles the arena's
next mark (2^32 for the reference, 2^31 for the events -- an event offset is a uint32_t) and one that ends with the arena.  Every job
list and candidate batch is built as its LOW TWIN, with offsets inside a segment at place 0; `shifted` moves a twin's windows to other
places.  What a job must answer never depends on its place, so every expected value is computed from the low twin on arrays of a
segment's size.

DECOYS make a truncated address a certain mismatch instead of a read of whatever the arena held: wherever `p mod W` (p a place, W one
of 2^30, 2^31, 2^32) is another offset, lies inside the arena and touches neither a planted copy nor an earlier decoy, a segment of
OTHER content (`ref_decoy`, `ev_decoy`) lies there.  A body that forms a byte offset in 32 bits (W = 2^30 elements), passes an
element offset through int (2^31) or through uint32_t (2^32) then reads valid memory that holds different signals.  Where the wrapped
offset falls into a planted copy instead (the two straddling copies overlap modulo 2^30), the body reads the right content at another
offset, which is a mismatch as well for random signals.

The direction-byte counters restate the three tracebacks' formulas (tests/traceback_cases.dir_bytes_for, tests/banded_tb_cases.dir_bytes
and rawdtw_semiglobal.h's semi_dir_bytes) and their sub-batch cut, and choose for each the smallest cyclic job list over seven windows
whose 256-rounded direction bytes pass 2^32 + 2^28 inside one sub-batch of the default 16 GiB budget."""
import functools

import numpy as np

from rawalign_amd.align import CandidateBatch
from rawalign_amd.dtw import ANCHOR_DTYPE, JOB_DTYPE
from tests import banded_tb_cases as bc
from tests import planted_path_cases as pc
from tests import traceback_cases as tc

MARK_30, MARK_31, MARK_32 = 1 << 30, 1 << 31, 1 << 32
MODULI = (MARK_30, MARK_31, MARK_32)
REF_FLOATS = MARK_32 + (1 << 27)   # tests/test_gpu_parity.py::test_human_scale_reference_offsets' arena
EV_FLOATS = MARK_31 + (1 << 27)    # 9.1 GB; rawdtw_set_events_device admits up to 2^32 - 1 floats
SEG_REF, SEG_EV = 200000, 50000
FILL = np.float32(0.5)
RANDOM_REF, RANDOM_EV = 190000, 42000   # a segment's random part; behind it lie the planted-path signals of `banded_cases`

# begins below its mark, ends above it, at an offset that is no multiple of 4
REF_PLACES = (0, MARK_30 - 100001, MARK_32 - 60003, REF_FLOATS - SEG_REF)
EV_PLACES = (0, MARK_30 - 25001, MARK_31 - 15003, EV_FLOATS - SEG_EV)
REF_MARKS = (None, MARK_30, MARK_32, None)   # what a place straddles
EV_MARKS = (None, MARK_30, MARK_31, None)
DIR_FLOOR = MARK_32 + (1 << 28)    # what one sub-batch's direction bytes must pass
N_WINDOWS = 7


def decoys(places, seg, arena):
    """the decoys' first floats, ascending"""
    taken = [(p, p + seg) for p in places]
    out = []
    for p in places:
        for w in MODULI:
            q = p % w
            if q == p or q in out or q + seg > arena or any(q < hi and lo < q + seg for lo, hi in taken):
                continue
            out.append(q)
            taken.append((q, q + seg))
    return sorted(out)


REF_DECOYS = decoys(REF_PLACES, SEG_REF, REF_FLOATS)
EV_DECOYS = decoys(EV_PLACES, SEG_EV, EV_FLOATS)


def alias_of(p, w, places, decoy_list, seg):
    """what lies at p mod w: ("same", 0), ("decoy", 0) or ("planted", shift): a planted copy that begins `shift` floats before p mod w"""
    q = p % w
    if q == p:
        return "same", 0
    if q in decoy_list:
        return "decoy", 0
    for r in places:
        if r <= q < r + seg:
            return "planted", q - r
    return "none", 0


# ---- the segments ----------------------------------------------------------------------------------------------------------------------
BANDED_NAMES = ("one_chunk", "three_chunks", "past_1024")   # bands of 1, 3 and 17 chunks: the small members of planted_path_cases.BANDED


def banded_entries():
    return [e for e in pc.banded_list() if e[0] in BANDED_NAMES]


@functools.lru_cache(maxsize=None)
def _segments():
    rng = np.random.default_rng(12)
    ref = rng.normal(size=SEG_REF).astype(np.float32)
    ev = (ref[:SEG_EV] + rng.normal(scale=0.2, size=SEG_EV)).astype(np.float32)
    cases, _ = pc.banded_jobs(banded_entries())
    eo, ro, where = RANDOM_EV, RANDOM_REF, []
    for a, b, R, ex in cases:
        ev[eo:eo + len(a)], ref[ro:ro + len(b)] = a, b
        where.append((ro, eo, len(a), len(b), R, ex, 0))
        eo, ro = eo + len(a) + 3, ro + len(b) + 5
    assert eo <= SEG_EV and ro <= SEG_REF
    drng = np.random.default_rng(912)
    dref = drng.normal(size=SEG_REF).astype(np.float32)
    dev = (dref[:SEG_EV] + drng.normal(scale=0.2, size=SEG_EV)).astype(np.float32)
    for x in (ref, ev, dref, dev):
        x.setflags(write=False)
    return ref, ev, dref, dev, np.array(where, JOB_DTYPE)


def ref_segment():
    return _segments()[0]


def ev_segment():
    return _segments()[1]


def ref_decoy():
    return _segments()[2]


def ev_decoy():
    return _segments()[3]


# ---- twins -----------------------------------------------------------------------------------------------------------------------------
def round_robin(count):
    """(index of the reference place, index of the event place) of item k: all sixteen pairs in every sixteen items in a row, in an
    order drawn anew for every sixteen, so that no stride of a job list (every 5th job full, every 8th large) ties a kind to a place"""
    rng = np.random.default_rng(1211)
    pair = np.concatenate([rng.permutation(16) for _ in range((count + 15) // 16)])[:count]
    return pair % 4, pair // 4


def shifted(jobs_or_batch, ref_place, ev_place, back=False):
    """The twin of a job list or CandidateBatch: every job's (chain's) reference window moved by ref_place and its event window by
    ev_place, scalars or one value an item; back=True undoes it.  A CandidateBatch keeps its events array: device batches read the arena."""
    sign = -1 if back else 1
    x = jobs_or_batch
    if isinstance(x, CandidateBatch):
        rb = (x.ref_base.astype(np.int64) + sign * np.asarray(ref_place, np.int64)).astype(np.uint64)
        eb = x.read_base.astype(np.int64) + sign * np.asarray(ev_place, np.int64)
        assert eb.min() >= 0 and eb.max() < MARK_32
        return CandidateBatch(x.events, x.chain_off, x.anchor_off, x.anchors, rb, eb.astype(np.uint32))
    out = np.array(x, JOB_DTYPE)
    out["ref_off"] = (out["ref_off"].astype(np.int64) + sign * np.asarray(ref_place, np.int64)).astype(np.uint64)
    eo = out["read_off"].astype(np.int64) + sign * np.asarray(ev_place, np.int64)
    assert len(out) == 0 or (eo.min() >= 0 and eo.max() < MARK_32)
    out["read_off"] = eo.astype(np.uint32)
    return out


def spread(jobs, copies=1):
    """(low twin with every job `copies` times in a row, its twin over the places round-robin)"""
    low = np.repeat(np.array(jobs, JOB_DTYPE), copies)
    ri, ei = round_robin(len(low))
    return low, shifted(low, np.array(REF_PLACES, np.int64)[ri], np.array(EV_PLACES, np.int64)[ei])


def windows(jobs, ev=None, ref=None):
    """[(a, b, band_radius, exclude_last)] of a LOW job list on the segments (or on decoy content)"""
    ev = ev_segment() if ev is None else ev
    ref = ref_segment() if ref is None else ref
    return [(ev[int(j["read_off"]):int(j["read_off"]) + int(j["n"])], ref[int(j["ref_off"]):int(j["ref_off"]) + int(j["m"])],
             int(j["band_radius"]), int(j["exclude_last"])) for j in jobs]


# ---- low twins of the job lists ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def score_jobs():
    """test_human_scale_reference_offsets' 400-job mix (lane, group, wave, full, multi-strip and the wide banded body), windows drawn
    from the segments' random parts"""
    rng = np.random.default_rng(1212)
    jobs = []
    for k in range(400):
        n = int(rng.integers(2, 70)) if k % 8 else int(rng.integers(200, 1500))
        m = max(2, int(n * rng.uniform(0.6, 1.3)))
        eo = int(rng.integers(0, RANDOM_EV - n))
        so = int(rng.integers(0, RANDOM_REF - m))
        R0 = -1 if k % 5 == 0 else max(1, int(np.float32(n) * np.float32(0.1)))
        jobs.append((so, eo, n, m, R0, k & 1, 0))
    return np.array(jobs, JOB_DTYPE)


CLASS_K = (8, 16, 64, 65, 257, 1025, 2049)


@functools.lru_cache(maxsize=None)
def class_jobs():
    """banded jobs of K = radius + 1 slots that the mix's radii (at most 149) never reach: the 8-lane and 16-lane groups, the register
    bodies of 1, 2, 8 and 32 chunks of 64 slots, and beyond 2 048 slots the body that keeps its antidiagonals in LDS (k_band_wave);
    tests/test_gpu_parity.py::test_random_wave_band's shapes"""
    rng = np.random.default_rng(1218)
    jobs = []
    for K in CLASS_K:
        n = int(K * 1.6) + 7
        jobs.append((int(rng.integers(0, RANDOM_REF - n)), int(rng.integers(0, RANDOM_EV - n)), n, n, K - 1, K & 1, 0))
    return np.array(jobs, JOB_DTYPE)


CLASS_N = (1, 64, 65, 128, 129, 256, 257, 512, 513, 1025, 1537)   # tests/test_local_gpu.CLASS_N


@functools.lru_cache(maxsize=None)
def semiglobal_jobs():
    """n at every class and strip edge of the semiglobal kernels, m = 65 and 2 n; exclude_last alternates"""
    rng = np.random.default_rng(1213)
    jobs = []
    for n in CLASS_N:
        for m in (65, 2 * n):
            jobs.append((int(rng.integers(0, RANDOM_REF - m)), int(rng.integers(0, RANDOM_EV - n)), n, m, -1, len(jobs) & 1, 0))
    return np.array(jobs, JOB_DTYPE)


def banded_jobs():
    """the planted-path jobs of BANDED_NAMES, both orientations, where `_segments` laid their signals"""
    return _segments()[4].copy()


TB_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (30, 20), (64, 64), (65, 100), (130, 129), (260, 300), (513, 600), (600, 513), (900, 1100),
             (1500, 1300), (1100, 2600))   # tests/test_traceback_arena_gpu.SHAPES


@functools.lru_cache(maxsize=None)
def traceback_jobs():
    rng = np.random.default_rng(1214)
    return np.array([(int(rng.integers(0, RANDOM_REF - m)), int(rng.integers(0, RANDOM_EV - n)), n, m, -1, int(k % 3 == 1), 0)
                     for k, (n, m) in enumerate(TB_SHAPES)], JOB_DTYPE)


# ---- low twins of the candidate batches --------------------------------------------------------------------------------------------------
N_CHAINS, CHAINS_A_READ = 48, 4


@functools.lru_cache(maxsize=None)
def candidate_batch():
    """48 chains of 2 .. 59 anchors, four to a read, over the segments' random parts; ref_base 0, a read's read_base 0 .. 9.  The event
    segment is the reference segment's head plus noise, so two chains in three follow the events' own positions (they score and are
    kept) and every third lies anywhere (cut)."""
    rng = np.random.default_rng(1215)
    anchors, anchor_off = [], [0]
    for c in range(N_CHAINS):
        na = int(rng.integers(2, 60))
        q = np.cumsum(rng.integers(3, 14, na)) + int(rng.integers(100, 20000))
        if c % 3:
            t = q + (c // CHAINS_A_READ) % 10 + np.cumsum(rng.integers(-1, 2, na))
        else:
            t = np.cumsum(rng.integers(2, 12, na)) + int(rng.integers(0, 100000))
        a = np.zeros(na, ANCHOR_DTYPE)
        a["query_position"], a["target_position"] = q[::-1], t[::-1]
        anchors.append(a)
        anchor_off.append(anchor_off[-1] + na)
    chain_off = np.arange(0, N_CHAINS + 1, CHAINS_A_READ, dtype=np.uint64)
    read_base = np.repeat(np.arange(N_CHAINS // CHAINS_A_READ, dtype=np.uint32) % 10, CHAINS_A_READ)
    return CandidateBatch(ev_segment(), chain_off, np.array(anchor_off, np.uint64), np.concatenate(anchors), np.zeros(N_CHAINS, np.uint64), read_base)


def batch_places():
    """one reference place a chain and one event place a read (a read's chains share its events), round-robin"""
    ri, _ = round_robin(N_CHAINS)
    ei = (np.arange(N_CHAINS) // CHAINS_A_READ + 1) % 4
    return np.array(REF_PLACES, np.int64)[ri], np.array(EV_PLACES, np.int64)[ei]


# ---- direction bytes -----------------------------------------------------------------------------------------------------------------------
BUDGET = tc.DEFAULT_BUDGET


def al256(x):
    return (x + 255) & ~255


def semi_class(n, m, full_wg=True):
    """rawdtw_semiglobal.h"""
    c = 0 if n <= 64 else 1 if n <= 128 else 2 if n <= 256 else 3
    if c == 3 and n > 1024 and full_wg and m < (1 << 21) and (n + 511) // 512 < (1 << 11):
        return 4
    return c


def semi_dir_bytes(n, m, full_wg=True):
    """rawdtw_semiglobal.h: [strip][block][lane][step in block], blocks of 16 bytes a lane"""
    cls = semi_class(n, m, full_wg)
    rpl = 8 if cls >= 3 else 1 << cls
    strips = (n + 64 * rpl - 1) // (64 * rpl)
    spb = 8 if rpl == 8 else 16
    return strips * ((m + 63 + spb - 1) // spb) * 64 * 16


DIR_BYTES = {
    "full": lambda j: tc.dir_bytes_for(int(j["n"]), int(j["m"])),
    "semiglobal": lambda j: semi_dir_bytes(int(j["n"]), int(j["m"])),
    "banded": lambda j: bc.dir_bytes(int(j["n"]), int(j["m"]), int(j["band_radius"])),
}


def direction_total(kind, jobs):
    """the direction workspace of one sub-batch holding `jobs`: every job's bytes rounded up to 256"""
    return sum(al256(DIR_BYTES[kind](j)) for j in jobs)


def sub_batches(kind, jobs, budget=BUDGET):
    """job counts of the sub-batches: rawdtw_traceback.cpp and rawdtw_semiglobal.cpp charge bytes + 256 a job, rawdtw_band_tb.cpp the
    bytes rounded up to 256; a job joins unless that passes the budget, a job over the budget goes alone"""
    out, cur, used = [], 0, 0
    for j in jobs:
        b = al256(DIR_BYTES[kind](j)) if kind == "banded" else DIR_BYTES[kind](j) + 256
        if cur and used + b > budget:
            out.append(cur)
            cur, used = 0, 0
        cur += 1
        used += b
    return out + ([cur] if cur else [])


# seven windows a traceback: (n, m, band_radius).  Full and semiglobal: the shorter side in every rows-per-lane class, one to four strips;
# a long side near 30 000 keeps a job's directions in the megabytes and the whole list at a few hundred jobs.  Banded: 8 192 x 8 192 at
# bands of 3 to 65 chunks, the mapper's radius (819) among them.
DIR_SHAPES = {
    "full": ((64, 30001, -1), (128, 29903, -1), (256, 30007, -1), (512, 29989, -1), (513, 30011, -1), (1025, 30013, -1), (1537, 29999, -1)),
    "semiglobal": ((64, 30001, -1), (128, 29903, -1), (256, 30007, -1), (512, 29989, -1), (513, 30011, -1), (1025, 30013, -1), (1537, 29999, -1)),
    "banded": ((8192, 8192, 150), (8192, 8100, 819), (8000, 8192, 1030), (8192, 8192, 2047), (8191, 8192, 2048), (8192, 8192, 3000), (8192, 8189, 4100)),
}


@functools.lru_cache(maxsize=None)
def direction_windows(kind):
    """the seven distinct low jobs of a traceback"""
    rng = np.random.default_rng([1216, sorted(DIR_SHAPES).index(kind)])
    return np.array([(int(rng.integers(0, RANDOM_REF - m)), int(rng.integers(0, RANDOM_EV - n)), n, m, R, k & 1, 0)
                     for k, (n, m, R) in enumerate(DIR_SHAPES[kind])], JOB_DTYPE)


@functools.lru_cache(maxsize=None)
def direction_jobs(kind):
    """(low twin, high twin, window index of every job): the windows in a cycle, cut at the first job that takes the summed direction
    bytes past DIR_FLOOR -- no shorter prefix of the cycle passes it"""
    win = direction_windows(kind)
    sizes = [al256(DIR_BYTES[kind](j)) for j in win]
    count, total = 0, 0
    while total <= DIR_FLOOR:
        total += sizes[count % N_WINDOWS]
        count += 1
    which = np.arange(count) % N_WINDOWS
    low = win[which]
    ri, ei = round_robin(count)
    return low, shifted(low, np.array(REF_PLACES, np.int64)[ri], np.array(EV_PLACES, np.int64)[ei]), which


# ---- expected values of a low candidate batch ---------------------------------------------------------------------------------------------
def batch_jobs(cb, opt):
    """the batch's job list as the library's host code builds it (rawdtw_batch_build_jobs; no device): (jobs, job_off)"""
    import ctypes as C

    from rawalign_amd._lib import load_library

    lib = load_library()
    arrs = [np.ascontiguousarray(cb.anchor_off, np.uint64), np.ascontiguousarray(cb.anchors, ANCHOR_DTYPE),
            np.ascontiguousarray(cb.ref_base, np.uint64), np.ascontiguousarray(cb.read_base, np.uint32)]
    job_off = np.zeros(cb.n_chains + 1, np.uint64)
    copt, nj = opt.c_struct(), C.c_uint64()
    args = (C.byref(copt), cb.n_chains) + tuple(C.c_void_p(a.ctypes.data) for a in arrs) + (C.c_void_p(job_off.ctypes.data),)
    assert lib.rawdtw_batch_build_jobs(*args, None, 0, C.byref(nj)) == 0
    jobs = np.zeros(nj.value, JOB_DTYPE)
    assert lib.rawdtw_batch_build_jobs(*args, C.c_void_p(jobs.ctypes.data), len(jobs), C.byref(nj)) == 0
    return jobs, job_off


def batch_expected(oracle, cb, opt, ev=None, ref=None):
    """(score, keep, job costs) of a low batch under a sparse or global MapOpt: the oracle's sequential align_chain loop
    (rmap.cpp:515-524) and its cost of every job of the library's job list"""
    from oracle.loader import OrcOpt

    from tests.util import oracle_costs

    ev = ev_segment() if ev is None else ev
    ref = ref_segment() if ref is None else ref
    oopt = OrcOpt(opt.dtw_border_constraint, opt.dtw_fill_method, opt.dtw_band_radius_frac, opt.dtw_match_bonus, opt.dtw_min_score, int(opt.fused_score))
    score, keep = np.zeros(cb.n_chains, np.float32), np.zeros(cb.n_chains, np.uint8)
    for r in range(cb.n_reads):
        best = np.float32(0.0)
        for c in range(int(cb.chain_off[r]), int(cb.chain_off[r + 1])):
            a = cb.anchors[int(cb.anchor_off[c]):int(cb.anchor_off[c + 1])]
            s = oracle.align_chain(a, ref[int(cb.ref_base[c]):], ev[int(cb.read_base[c]):], oopt, float(best))
            score[c] = s
            if s >= np.float32(opt.dtw_min_score):
                keep[c] = 1
                if s > best:
                    best = s
    jobs, _ = batch_jobs(cb, opt)
    return score, keep, oracle_costs(oracle, jobs, ev, ref)


def local_expected(cb, opt, ev=None, ref=None):
    """(score, keep, job costs) of a low batch under the local border constraint: tests/local_cases.py's restatement"""
    from tests import local_cases as lc

    ev = ev_segment() if ev is None else ev
    ref = ref_segment() if ref is None else ref
    low = CandidateBatch(ev, cb.chain_off, cb.anchor_off, cb.anchors, cb.ref_base, cb.read_base)
    costs = lc.job_costs(low, {0: ref})
    score, keep = lc.fold(low, costs, opt)
    return score, keep, costs
