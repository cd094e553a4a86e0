"""The cases of tests/golden/seed_ref.npz: the answers of the REFERENCE's own seeding (ri_sketch, and ri_sketch + ri_idx_get as
gen_chains calls them: oracle/_ref/libref_map{0,1}.so) recorded by scripts/make_golden_seed.py.

Shared by the generator and by tests/test_seed_host.py / tests/test_seed_gpu.py, so that both draw the same inputs.  The inputs
are seeded and regenerated anywhere; the fixture carries their SHA-256, the sketches and the hits."""
import hashlib
import os

import numpy as np

from rawalign_amd import synth
from rawalign_amd.seeding import SeedParams

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "seed_ref.npz")
SEED = 20241016
MASK_SIGNAL = np.float32(3.402823466e+32)   # RI_MASK_SIGNAL, rsketch.h:8
DIFF = np.float32(0.3)                      # LAST_SIG_DIFF, rsketch.h:10

PARAM_SETS = {"e6": (6, 9, 3), "e4": (4, 9, 3), "e8": (8, 7, 2), "e5": (5, 10, 4)}   # e, q, lq


def mapping_reference():
    from tests import map_ref_cases as mc

    ref = mc.make_reference()
    return ref.forward, ref.reverse


def small_reference():
    """a few hundred events: with e = 2 the 44 k-event reference gives a chunk 143 418 hits"""
    ref = synth.make_reference((300,), seed=SEED + 1)
    return ref.forward, ref.reverse


MOTIF_TILES = 1100


def motif():
    """12 events, every neighbour more than 0.3 apart (all kept by the rule)"""
    return np.array([-1.6, 0.9, -0.4, 1.7, 0.2, -1.1, 1.2, -0.7, 0.5, -1.9, 1.5, -0.1], np.float32)


def motif_reference():
    """one sequence whose forward array is a motif tiled MOTIF_TILES times between two random flanks: every e-mer of the motif
    is a key with more than a thousand positions"""
    rng = np.random.default_rng(SEED + 2)
    fwd = np.concatenate([rng.normal(0, 1, 500), np.tile(motif(), MOTIF_TILES), rng.normal(0, 1, 500)]).astype(np.float32)
    rev = rng.normal(0, 1, len(fwd)).astype(np.float32)
    return [fwd], [rev]


def _stretches(fwd, rev, rng, n, length, sd=0.05):
    out = []
    for k in range(n):
        s = int(rng.integers(0, len(fwd)))
        arr = fwd[s] if k % 2 else rev[s]
        lo = int(rng.integers(0, max(1, len(arr) - length)))
        seg = arr[lo:lo + length]
        out.append((seg + rng.normal(0, sd, len(seg))).astype(np.float32))
    return out


def threshold_chunk(fwd):
    """a stretch of the reference, then neighbours whose fp32 difference is just below, exactly at and just above 0.3F (the
    subtraction is exact for these values), each group behind a far value so that the base is kept, then reference again"""
    base = np.float32(0.25)
    at = np.float32(base + DIFF)
    assert np.float32(at - base) == DIFF
    below, above = np.nextafter(at, np.float32(0)), np.nextafter(at, np.float32(1))
    assert np.float32(below - base) < DIFF < np.float32(above - base)
    groups = []
    # ... and below the base: exactly 0.3F under it, one step of 0.3F less than that, and a value one step of ITS OWN (eight times
    # finer) nearer, whose exact difference lies under 0.3F but rounds to it in fp32: kept, because the subtraction is fp32
    under = np.float32(base - DIFF)
    less = np.float32(base - np.nextafter(DIFF, np.float32(0)))
    near = np.nextafter(under, np.float32(1))
    assert np.float32(base - under) == DIFF and np.float32(base - less) < DIFF and float(base) - float(near) < float(DIFF) == float(np.float32(base - near))
    for y in (below, at, above, under, less, near):
        groups += [np.float32(-2.0), base, y, np.float32(2.0)]
    return np.concatenate([fwd[0][100:160], np.array(groups, np.float32), fwd[0][160:220]]).astype(np.float32)


def special_chunk(fwd):
    """RI_MASK_SIGNAL, +-0, +-inf between reference stretches; a NaN in front of a tail (a NaN is kept, and so is the event behind it)"""
    sp = np.array([MASK_SIGNAL, 0.0, -0.0, MASK_SIGNAL, np.inf, 1.0, -np.inf, -1.0, MASK_SIGNAL, MASK_SIGNAL], np.float32)
    tail = np.repeat(fwd[1][300:330], 2)   # doubled events: every second one dropped by the rule
    return np.concatenate([sp[:4], fwd[1][200:260], sp[4:], fwd[1][260:300], tail, np.array([np.nan], np.float32), tail]).astype(np.float32)


def mask_first_chunks(fwd, rev, rng):
    """chunks whose event 0 is RI_MASK_SIGNAL: it is skipped, l_sigpos stays 0 and what follows is compared with the mask value
    itself (rsketch.c:233,243) -- so the next event is kept whatever it is.  The stretches behind the masks are exact copies of
    the reference that begin within 0.3 of 0: a filter that compared with 0 instead would drop their first events, and their
    e-mers are keys of the index, so the hits tell."""
    out = []
    for k in range(12):
        arr = (fwd, rev)[k % 2][k % len(fwd)]
        kept, last = np.zeros(len(arr), bool), 0   # the array's own sketch keeps these: a copy from a kept event on has its e-mers
        kept[0] = True
        for i in range(1, len(arr)):
            if not abs(np.float32(arr[i] - arr[last])) < DIFF:
                kept[i], last = True, i
        near0 = np.nonzero(kept[:-80] & (np.abs(arr[:-80]) < 0.25))[0]
        p = int(near0[rng.integers(0, len(near0))])
        out.append(np.concatenate([np.full(1 + k % 3, MASK_SIGNAL, np.float32), arr[p:p + 70]]).astype(np.float32))
    return out


def build_case(name):
    """(forward, reverse, SeedParams, [chunk events])"""
    rng = np.random.default_rng(SEED + sum(name.encode()))
    if name in PARAM_SETS:
        e, q, lq = PARAM_SETS[name]
        fwd, rev = mapping_reference()
        n, length = (4, 400) if name in ("e6", "e5") else (2, 150)
        return fwd, rev, SeedParams(e=e, q=q, lq=lq), _stretches(fwd, rev, rng, n, length)
    if name == "e9":
        fwd, rev = mapping_reference()
        return fwd, rev, SeedParams(e=9), _stretches(fwd, rev, rng, 4, 400, sd=0.02)
    if name == "e2":
        fwd, rev = small_reference()
        return fwd, rev, SeedParams(e=2), _stretches(fwd, rev, rng, 2, 60)
    if name.startswith("w"):
        fwd, rev = mapping_reference()
        return fwd, rev, SeedParams(w=int(name[1:])), _stretches(fwd, rev, rng, 2, 400)
    if name == "motif":
        fwd, rev = motif_reference()
        m = motif()
        return fwd, rev, SeedParams(), [m.copy(), np.concatenate([rng.normal(0, 1, 30).astype(np.float32), m[3:], m[:5]])]
    if name == "maskfirst":
        fwd, rev = mapping_reference()
        return fwd, rev, SeedParams(), mask_first_chunks(fwd, rev, rng)
    if name == "edges":
        fwd, rev = mapping_reference()
        e = 6
        seg = fwd[2][1000:1400]
        keep = [0]
        for i in range(1, len(seg)):
            if abs(float(seg[i]) - float(seg[keep[-1]])) > 0.4:
                keep.append(i)
        far = seg[keep]   # every event more than 0.3 from the one before it: all kept
        short = [far[:0], far[:1], far[:e - 1], far[:e], far[:e + 1]]
        return fwd, rev, SeedParams(e=e), short + [threshold_chunk(fwd), special_chunk(fwd), np.full(40, MASK_SIGNAL, np.float32),
                                                   np.full(30, 0.5, np.float32)]
    raise KeyError(name)


CASES = ["e6", "e4", "e8", "e5", "e9", "e2", "w1", "w5", "w10", "w255", "motif", "edges", "maskfirst"]
DEVICE_CASES = [c for c in CASES if not c.startswith("w")]


def case_sha256(fwd, rev, chunks) -> bytes:
    h = hashlib.sha256()
    for x in list(fwd) + list(rev) + list(chunks):
        h.update(np.ascontiguousarray(x, "<f4").tobytes())
        h.update(np.array([len(x)], "<i8").tobytes())
    return h.digest()


def flat(chunks):
    """(events, event_off) of a list of chunks"""
    off = np.zeros(len(chunks) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in chunks])
    return np.concatenate(list(chunks) + [np.zeros(0, np.float32)]).astype(np.float32), off


class Fixture:
    def __init__(self, z=None):
        self.z = np.load(FIXTURE) if z is None else z

    def sha(self, name):
        return self.z[name + "/sha256"].tobytes()

    def sketch(self, name, c):
        off = self.z[name + "/sk_off"]
        return self.z[name + "/sk_hash"][int(off[c]):int(off[c + 1])], self.z[name + "/sk_pos"][int(off[c]):int(off[c + 1])]

    def hit_off(self, name):
        return self.z[name + "/hit_off"].astype(np.uint64)

    def hits(self, name):
        """rows (sequence, strand, target, query in the chunk) of all the case's chunks, in order"""
        return self.z[name + "/hits"].astype(np.uint32)


def hit_rows(h):
    """HIT_DTYPE records as the fixture's rows"""
    return np.stack([h["ref_seq"], h["strand"].astype(np.uint32), h["target_position"], h["query_position"]], 1).astype(np.uint32).reshape(-1, 4)
