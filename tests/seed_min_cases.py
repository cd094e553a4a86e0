"""The cases of tests/golden/seed_min_ref.npz: the REFERENCE's minimizer sketch (ri_sketch_min, src/rsketch.c:146-221) and its hits
on inputs that put equal hashes into one window -- which the random chunks of seed_ref.npz almost never do, so that the tie branches
of rsketch.c:194-214 were pinned by nothing recorded.  Recorded by scripts/make_golden_seed_min.py.

Shared by the generator, tests/test_seed_min_host.py and tests/test_seed_min_gpu.py.  The inputs are seeded and regenerated anywhere;
the fixture carries their SHA-256, the sketches in full, the hit offsets, and the hit rows (or, above MAX_ROWS, their SHA-256)."""
import hashlib
import os

import numpy as np

from rawalign_amd.seeding import SeedParams
from tests import seed_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "seed_min_ref.npz")
SEED = 20261018
MAX_ROWS = 20000
MASK_SIGNAL = sc.MASK_SIGNAL

LEVELS = np.array([-4, -2, -1, -0.5, 0.5, 1, 2, 4], np.float32)   # eight distinct codes at q = 9, lq = 3; neighbours 0.5 or more apart
ALPHA_SETS = [(2, 3, 3, 40), (2, 5, 4, 60), (3, 4, 3, 60), (3, 8, 4, 80), (4, 12, 3, 90), (2, 255, 3, 300)]   # e, w, levels, events
ALPHA_CHUNKS = 200
MOTIF_W = [11, 12, 13, 24, 100, 255]
MOTIF_TILES = 40
LEN_E, LEN_W = 6, 5
LENGTHS = [0, 1, LEN_E - 1, LEN_E, LEN_E + 1, LEN_E + LEN_W - 2, LEN_E + LEN_W - 1, LEN_E + LEN_W, 64, 65, 256, 257, 700]

ALPHA_CASES = ["alpha_e%d_w%d_a%d" % s[:3] for s in ALPHA_SETS]
MOTIF_CASES = ["motif_w%d" % w for w in MOTIF_W]
CASES = ALPHA_CASES + MOTIF_CASES + ["lengths", "long_w255", "values"]


def all_kept(n, rng):
    """n events, every one more than 0.3 from the one before it (all kept by the rule)"""
    x = np.zeros(n, np.float32)
    for i in range(1, n):
        step = np.float32(rng.uniform(0.4, 1.5)) * (1 if x[i - 1] < 0 else -1)
        x[i] = np.float32(x[i - 1] + step)
    assert n < 2 or np.abs(np.diff(x)).min() > 0.35
    return x


def mask_mid_chunk(fwd):
    """an exact copy of the reference with RI_MASK_SIGNAL put between two of its events mid-chunk: (events, where).  Under the
    w = 0 rule the mask is dropped and the e-mers across it are the reference's own (a full window of them: one is a minimizer and
    a key); kept and coded, it is part of every e-mer across it and none of those is a key."""
    ev = np.concatenate([fwd[0][500:560], [MASK_SIGNAL], fwd[0][560:620]]).astype(np.float32)
    return ev, 60


def build_case(name):
    """(forward, reverse, SeedParams, [chunk events])"""
    rng = np.random.default_rng(SEED + sum(name.encode()))
    if name in ALPHA_CASES:
        e, w, a, n = ALPHA_SETS[ALPHA_CASES.index(name)]
        fwd, rev = [LEVELS[rng.integers(0, a, 120)]], [LEVELS[rng.integers(0, a, 120)]]   # every e-mer is a key with a list
        return fwd, rev, SeedParams(w=w, e=e), [LEVELS[rng.integers(0, a, n)] for _ in range(ALPHA_CHUNKS)]
    if name in MOTIF_CASES:
        m = sc.motif()
        fwd = [np.concatenate([rng.normal(0, 1, 100), np.tile(m, 20), rng.normal(0, 1, 100)]).astype(np.float32)]
        rev = [rng.normal(0, 1, len(fwd[0])).astype(np.float32)]
        return fwd, rev, SeedParams(w=int(name[7:]), e=6), [np.tile(m, MOTIF_TILES)]
    if name in ("lengths", "long_w255"):
        far = all_kept(700, rng)
        fwd, rev = [far.copy()], [all_kept(700, rng)]   # the chunks are prefixes of the forward strand: every e-mer hits
        if name == "lengths":
            return fwd, rev, SeedParams(w=LEN_W, e=LEN_E), [far[:n].copy() for n in LENGTHS]
        return fwd, rev, SeedParams(w=255, e=LEN_E), [far.copy()]
    if name == "values":
        fwd, rev = sc.mapping_reference()
        first = np.concatenate([[MASK_SIGNAL], fwd[1][700:800]]).astype(np.float32)
        nan_in = fwd[2][300:400].copy()
        nan_in[50] = np.nan
        return fwd, rev, SeedParams(w=LEN_W, e=LEN_E), [first, mask_mid_chunk(fwd)[0], nan_in, sc.special_chunk(fwd), sc.threshold_chunk(fwd)]
    raise KeyError(name)


def rows_sha256(rows) -> bytes:
    return hashlib.sha256(np.ascontiguousarray(rows, "<u4").tobytes()).digest()


class Fixture:
    def __init__(self, z=None):
        self.z = np.load(FIXTURE) if z is None else z

    def sha(self, name):
        return self.z[name + "/sha256"].tobytes()

    def sketch(self, name, c):
        off = self.z[name + "/sk_off"]
        return self.z[name + "/sk_hash"][int(off[c]):int(off[c + 1])].astype(np.uint32), self.z[name + "/sk_pos"][int(off[c]):int(off[c + 1])].astype(np.uint32)

    def hit_off(self, name):
        return self.z[name + "/hit_off"].astype(np.uint64)

    def check_rows(self, name, rows):
        """the hit rows of all the case's chunks against what is recorded: the rows themselves, or their digest"""
        rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, 4)
        if name + "/hits" in self.z:
            return np.array_equal(rows, self.z[name + "/hits"].astype(np.uint32).reshape(-1, 4))
        return rows_sha256(rows) == self.z[name + "/hits_sha256"].tobytes()
