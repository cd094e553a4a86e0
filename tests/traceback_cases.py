"""Case lists for the traceback's sub-batch pipeline (rawdtw_tb_driver.cpp: tb_run) and the walk kernel's edges
(k_full_wave<., true, .>, k_tb_walk_wave<RPL>, k_tb_finish), shared by tests/test_traceback_cases.py (CPU: the lists have the
properties they are there for) and tests/test_traceback_pipeline_gpu.py (the device against the oracle, bit for bit).

Also a plain-Python model of how the driver cuts a full-matrix batch into sub-batches, so that the GPU tests can say how many
sub-batches a call must have had ("tb_sub_batches") and which jobs sit where."""
import numpy as np

MIB = 1 << 20
DEFAULT_BUDGET = 16 << 30  # tb_budget_bytes without "tb_workspace_mb" and without RAWDTW_TB_WORKSPACE_MB


# ---- the split, restated from rawdtw_capi.h (full_rpl, dir_bytes_for), rawdtw_traceback.cpp (full_job_dir_bytes) and
# rawdtw_tb_layout.h (split) -------------------------------------------------------------------------------------------
def full_rpl(ny):
    """rows of the shorter side a lane of k_full_wave holds"""
    return 1 if ny <= 64 else 2 if ny <= 128 else 4 if ny <= 256 else 8


def dir_bytes_for(n, m):
    """bytes of a job's direction buffer: [strip][16-byte block][lane]"""
    nx, ny = max(n, m), min(n, m)
    rpl = full_rpl(ny)
    strips = (ny + 64 * rpl - 1) // (64 * rpl)
    spb = 8 if rpl == 8 else 16  # steps per 16-byte block
    return strips * ((nx + 63 + spb - 1) // spb) * 64 * 16


def split(shapes, budget_bytes):
    """[(first job, job count)] of every sub-batch: a job costs its direction bytes plus 256, and joins the current
    sub-batch unless that would pass the budget and the sub-batch is not empty (so a job over the budget goes alone)"""
    out, begin = [], 0
    while begin < len(shapes):
        end, used = begin, 0
        while end < len(shapes):
            b = dir_bytes_for(*shapes[end]) + 256
            if end > begin and used + b > budget_bytes:
                break
            used += b
            end += 1
        out.append((begin, end - begin))
        begin = end
    return out


def shapes_of(cases):
    return [(len(a), len(b)) for a, b, _, _ in cases]


# ---- the lists: (a, b, band_radius = -1, exclude_last) as tests.util.make_arena_jobs takes them ---------------------
_cache = {}


def _normal(rng, n):
    return rng.normal(size=n).astype(np.float32)


PIPE_LARGE = (0, 61, 122)  # where PIPE's three large jobs sit


def pipe_cases():
    """120 jobs with both sides in 150..700, a 3 000 x 2 049 job in front, one after the 60th and a 2 049 x 3 000 one
    last; exclude_last on every third.  At a budget of 1 MiB every large job is over the budget alone and the small ones
    fill a dozen sub-batches: both slots of every buffer, the k >= 2 branch, sb.begin and sb.lo all matter."""
    if "pipe" not in _cache:
        rng = np.random.default_rng(51)
        sides = rng.integers(150, 701, size=(120, 2))
        shapes = [(int(n), int(m)) for n, m in sides]
        shapes = [(3000, 2049)] + shapes[:60] + [(3000, 2049)] + shapes[60:] + [(2049, 3000)]
        assert [k for k, s in enumerate(shapes) if max(s) == 3000] == list(PIPE_LARGE)
        _cache["pipe"] = [(_normal(rng, n), _normal(rng, m), -1, int(k % 3 == 0)) for k, (n, m) in enumerate(shapes)]
    return _cache["pipe"]


EDGE_IDENTICAL = (64, 65, 127, 128, 192)
BORDER_RUN = 200


def edge_cases():
    """The walk kernel's and the fill kernel's edges: shorter sides on every rows-per-lane and strip boundary in both
    orientations, one-row and one-column jobs around the 64-step flush, pure diagonals of chosen lengths, long runs along
    a border (no direction block is loaded there), and a few of several strips.  exclude_last alternates."""
    if "edge" not in _cache:
        rng = np.random.default_rng(52)
        pairs = []
        for s in (64, 128, 256, 512, 1024):
            pairs += [(s, s), (s + 1, s), (s, s + 1), (s + 1, s + 1)]  # (the last: the shorter side just past the boundary)
        ones = [(1, 63), (1, 64), (1, 65), (1, 127), (1, 128), (1, 129)]
        pairs += [(1, 1)] + ones + [(m, n) for n, m in ones]
        pairs += [(2, 5000), (5000, 2)]
        ab = [(_normal(rng, n), _normal(rng, m)) for n, m in pairs]
        for n in EDGE_IDENTICAL:  # identical and integer-valued: cost 0 on the diagonal, which wins every tie
            x = rng.integers(-40, 41, n).astype(np.float32)
            ab.append((x, x.copy()))
        a = np.array([0] * BORDER_RUN + [10] * 50, np.float32)
        b = np.array([0] + [10] * 50, np.float32)
        ab += [(a, b), (b.copy(), a.copy())]  # the path stays at j == 0 (at i == 0) for its first BORDER_RUN elements
        ab += [(_normal(rng, n), _normal(rng, m)) for n, m in ((1500, 1300), (1100, 2600), (3000, 2049), (2049, 3000))]
        _cache["edge"] = [(a, b, -1, k & 1) for k, (a, b) in enumerate(ab)]
    return _cache["edge"]


def big_cases():
    """The benchmark's traceback_8192 shape, one long side against a short one in both orientations, and eight strips
    plus one row.  The first job's direction buffer is 16 908 288 bytes: over a budget of 16 MiB alone."""
    if "big" not in _cache:
        rng = np.random.default_rng(53)
        shapes = [(8192, 8192), (8192, 300), (300, 8192), (4097, 4096)]
        _cache["big"] = [(_normal(rng, n), _normal(rng, m), -1, k & 1) for k, (n, m) in enumerate(shapes)]
    return _cache["big"]


CASES = {"pipe": pipe_cases, "edge": edge_cases, "big": big_cases}


def oracle_paths(oracle, name):
    """[(cost, i, j, difference)] of a list from oracle.dtw_global_tb (exclude_last's pop included), computed once a
    session and never changed"""
    key = ("want", name)
    if key not in _cache:
        out = []
        for a, b, _, ex in CASES[name]():
            c, pi, pj, pd = oracle.dtw_global_tb(a, b, ex)
            for x in (pi, pj, pd):
                x.setflags(write=False)
            out.append((c, pi, pj, pd))
        _cache[key] = out
    return _cache[key]
