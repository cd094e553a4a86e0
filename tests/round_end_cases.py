"""Inputs of the round-end tests (tests/test_round_end_host.py, tests/test_round_end_gpu.py): the fixture rounds of
tests/golden/map_ref_rounds.npz as flat arrays, seeded random rounds, constructed edges and constructed declines -- and, from the host
restatement alone, which reads the device forms must decline (include/rawdtw.h: more than 64 chains taking part, two of them equal on all
seven keys, a NaN score, a quotient that is not finite or comp_mapq's product outside int)."""
import functools

import numpy as np

import rawalign_amd as ra
from rawalign_amd._lib import SelectOpt
from rawalign_amd.dtw import CHAIN_REC_DTYPE, NO_PRIMARY, ROUND_DECLINED, ROUND_HIGH  # noqa: F401
from tests import map_ref_cases as K

f32 = np.float32
COUNTS = (0, 1, 2, 3, 16, 17, 32, 33, 63, 64, 65)
ROUND_SIZES = (1, 63, 64, 65, 1000)
# (min_bestmap_ratio, min_meanmap_ratio, min_chain_anchor): the defaults of roptions.c:25-31 and others
SELECT_SETS = ((1.2, 5.0, 2), (1.05, 1.5, 3), (4.0, 1.5, 4), (2.0, 0.75, 1))


def select_opt(evaluate, k=0):
    b, m, a = SELECT_SETS[k]
    return SelectOpt(int(bool(evaluate)), b, m, a)


class Round:
    """one round's arrays as rawdtw_round_end takes them"""

    def __init__(self, reads, evaluate, sel=0, names=None):
        """reads: per read a list of (alignment_score, chaining_score, n_anchors, strand, seq, start, end, keep)"""
        n = sum(len(r) for r in reads)
        self.chain_off = np.zeros(len(reads) + 1, np.uint64)
        self.chain_off[1:] = np.cumsum([len(r) for r in reads])
        self.recs, self.score, self.keep = np.zeros(n, CHAIN_REC_DTYPE), np.zeros(n, np.float32), np.zeros(n, np.uint8)
        flat = [c for r in reads for c in r]
        if flat:
            a = np.array([[float(x) for x in c] for c in flat], np.float64)
            self.score[:] = np.array([c[0] for c in flat], np.float32)
            self.recs["chaining_score"] = np.array([c[1] for c in flat], np.float32)
            self.recs["n_anchors"], self.recs["key"] = a[:, 2], a[:, 4] * 2 + a[:, 3]
            self.recs["start_position"], self.recs["end_position"], self.keep[:] = a[:, 5], a[:, 6], a[:, 7]
        self.evaluate, self.sel = bool(evaluate), sel
        self.opt = select_opt(evaluate, sel)
        self.names = names

    @property
    def n_reads(self):
        return len(self.chain_off) - 1

    def host(self):
        return ra.round_end_host(self.opt, self.chain_off, self.recs, self.score, self.keep)

    def read(self, r):
        c0, c1 = int(self.chain_off[r]), int(self.chain_off[r + 1])
        return self.recs[c0:c1], self.score[c0:c1], self.keep[c0:c1]


# ---- the fixture's rounds -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    return K.Fixture()


@functools.lru_cache(maxsize=None)
def fixture_round(name, form):
    """Every (read, round) of an option set and build that ran gen_chains, as one Round: the candidates rebuilt as tests/test_map_ref.py
    does (K.host_candidates on the stored hits, re-seeded with the fixture's chains of the round before) and matched one by one to CAND_REC
    by their anchors' digest, with the reference's score; and per read the fixture's chains and stop-rule answer to compare with.
    Returns (Round, [(read, round, candidates, fixture chains, mapped)])."""
    from tests.test_map_ref import replay

    fx = fixture()
    opt, _ = K.project_opts(name, form)
    evaluate = bool(opt.flag & K.EVAL)
    reads, want = [], []
    for r, rnd, cands, _ in replay(fx, name, form):
        if cands is None:   # a chunk below min_events: no gen_chains, the chains stay (rmap.cpp:569-572)
            continue
        rec = fx.candidates(name, form, r, rnd)
        assert len(rec) == len(cands), (name, form, r, rnd)
        rows = []
        for c, k in zip(cands, rec):
            assert bytes(K.anchors_digest(c.anchors)) == bytes(k["digest"]) and int(K.bits(c.chaining_score)) == int(k["chaining"])
            s = np.uint32(k["score"]).view(np.float32)
            rows.append((s, f32(c.chaining_score), c.n_anchors, c.strand, c.reference_sequence_index, c.start_position, c.end_position,
                         int(s >= f32(opt.dtw_min_score))))   # rmap.cpp:518
        reads.append(rows)
        chains, mapped = fx.chains(name, form, r, rnd)
        want.append((r, rnd, cands, chains, mapped))
    return Round(reads, evaluate), want


def check_fixture_round(rd, want, out, primary, what):
    """out / primary of a fixture Round against the reference's answers: kept sequence, strand, start, end, n_anchors, mapq, the stop rule"""
    for i, (r, rnd, cands, chains, mapped) in enumerate(want):
        c0 = int(rd.chain_off[i])
        assert int(out[i]["n_primary"]) == len(chains), (what, r, rnd, out[i], len(chains))
        assert not int(out[i]["flags"]) & ROUND_DECLINED, (what, r, rnd)
        for k, ch in enumerate(chains):
            c = cands[int(primary[c0 + k])]
            got = (c.reference_sequence_index, c.strand, c.start_position, c.end_position, c.n_anchors)
            assert got == (int(ch["seq"]), int(ch["strand"]), int(ch["start"]), int(ch["end"]), int(ch["n_anchors"])), (what, r, rnd, k, got, ch)
        if len(chains):
            assert int(out[i]["mapq"]) == int(chains[0]["mapq"]), (what, r, rnd, out[i], chains[0])
        assert bool(int(out[i]["flags"]) & ROUND_HIGH) == mapped, (what, r, rnd)


# ---- random rounds --------------------------------------------------------------------------------------------------------------
def random_read(rng, n, evaluate, style):
    """n candidates.  style 0: scores and positions drawn from small sets, so that the comparator runs down its keys (records equal on
    all seven are told apart by their end); 1: scores spread over decades; 2: a read whose keep mask leaves nothing (evaluate) / whose
    alignment scores are all cut (-1e10)"""
    rows = []
    for _ in range(n):
        if style == 0:
            a, c = f32(rng.choice((22.5, 31.0, 31.0, 40.25, 57.0))), f32(rng.choice((12.0, 18.0, 18.0, 25.0)))
            na, key = int(rng.integers(2, 5)), int(rng.integers(0, 6))
            start = int(rng.integers(0, 12)) * 100
            end = start + int(rng.choice((60, 99, 100, 250)))
        else:
            a, c = f32(np.exp(rng.uniform(0, 6))), f32(np.exp(rng.uniform(0, 5)))
            na, key = int(rng.integers(2, 40)), int(rng.integers(0, 14))
            start = int(rng.integers(0, 30000))
            end = start + int(rng.integers(1, 600))
        keep = int(rng.random() < 0.7)
        if style == 2:
            keep, a = (0, a) if evaluate else (keep, f32(-1e10))
        elif not evaluate and rng.random() < 0.2:
            a = f32(-1e10)   # (a chain align_chain cut: it stays in the list without EVALUATE_CHAINS, rmap.cpp:525)
        rows.append([a, c, na, key & 1, key >> 1, start, end, keep])
    seen = {}
    for row in rows:   # no two records equal on all seven keys (constructed_declines has those)
        k = tuple(float(x) for x in row[:7])
        seen[k] = seen.get(k, 0) + 1
        row[6] += (seen[k] - 1) * 1000
    return [tuple(r) for r in rows]


def random_round(n_reads, evaluate, sel, seed):
    """Per-read chain counts drawn from COUNTS; a round of 63 reads or more starts with every count, empty reads between full ones.  A read
    of 65 chains is declined when they all take part, so only that one is certain (fewer than one read in sixty)."""
    rng = np.random.default_rng(seed)
    head = [64, 0, 65, 0, 63, 0, 33, 32, 0, 17, 16, 3, 2, 1]
    counts = [64] if n_reads == 1 else head + [int(rng.choice(COUNTS[:-1])) for _ in range(n_reads - len(head))]
    reads = [random_read(rng, n, evaluate, 2 if (i % 17 == 5) else int(rng.integers(0, 2))) for i, n in enumerate(counts)]
    return Round(reads, evaluate, sel)


@functools.lru_cache(maxsize=None)
def random_rounds():
    """(id, Round): every round size with both evaluate_chains values; the option sets rotate"""
    out = []
    for i, n in enumerate(ROUND_SIZES):
        for ev in (1, 0):
            out.append(("n%d-eval%d-sel%d" % (n, ev, (i + ev) % len(SELECT_SETS)), random_round(n, ev, (i + ev) % len(SELECT_SETS), 1000 + 10 * n + ev)))
    return tuple(out)


# ---- constructed reads ----------------------------------------------------------------------------------------------------------
def _c(a, c=10.0, na=3, strand=0, seq=0, start=0, end=100, keep=1):
    return (f32(a), f32(c), na, strand, seq, start, end, keep)


def constructed_edges():
    """(name, evaluate, select set, read, expected (n_primary, mapq or None, high or None, first primary or None)): none may decline"""
    third = f32(30.0) / f32(3.0)
    below = np.nextafter(third, f32(0), dtype=np.float32)
    r12 = f32(1.2)
    e = []
    # ties on each proper prefix of (alignment_score, chaining_score, n_anchors, strand, sequence, start, end): the greater next key first
    base = [30.0, 10.0, 3, 0, 0, 100, 200]
    for p in range(1, 7):
        hi = list(base)
        hi[p] = base[p] + 1
        for order in (0, 1):
            rows = [_c(*base), _c(*hi)]
            e.append(("tie-prefix-%d-order-%d" % (p, order), 1, 0, rows[::-1] if order else rows, (None, None, None, 1 - order)))
    e.append(("exactly-a-third-stays", 1, 0, [_c(30, seq=0), _c(third, seq=1)], (2, None, None, 0)))
    e.append(("one-ulp-below-a-third-ends", 1, 0, [_c(30, seq=0), _c(below, seq=1)], (1, 60, None, 0)))
    e.append(("break-before-a-later-free-chain", 1, 0, [_c(8, seq=2), _c(30, seq=0), _c(9, seq=1)], (1, 60, None, 1)))
    e.append(("overlap-keeps-the-bar", 1, 0, [_c(30, seq=0), _c(25, seq=0, start=50, end=150), _c(11, seq=1), _c(3.5, seq=2)], (2, None, None, 0)))
    e.append(("touching-intervals-overlap", 1, 0, [_c(30, start=100, end=200), _c(20, start=200, end=300)], (1, 60, None, 0)))
    e.append(("one-apart-do-not", 1, 0, [_c(30, start=100, end=200), _c(20, start=201, end=300)], (2, None, None, 0)))
    e.append(("same-interval-other-sequence", 1, 0, [_c(30, seq=0), _c(20, seq=1)], (2, None, None, 0)))
    e.append(("same-sequence-other-strand-overlaps", 1, 0, [_c(30, strand=0), _c(20, strand=1)], (1, 60, None, 0)))
    e.append(("best-ratio-exactly-met", 1, 0, [_c(r12, seq=0), _c(1.0, seq=1)], (2, None, True, 0)))
    e.append(("best-ratio-one-ulp-short", 1, 0, [_c(np.nextafter(r12, f32(0), dtype=np.float32), seq=0), _c(1.0, seq=1)], (2, None, False, 0)))
    e.append(("mean-ratio-exactly-met", 1, 2, [_c(3.0, seq=0), _c(1.0, seq=1)], (2, None, True, 0)))      # 4.0 > 3 / 1; 1.5 * mean(3, 1) == 3
    e.append(("mean-ratio-missed", 1, 2, [_c(3.0, seq=0), _c(1.5, seq=1)], (2, None, False, 0)))           # 1.5 * mean(3, 1.5) = 3.375
    e.append(("anchors-at-the-minimum", 1, 1, [_c(30, na=3)], (1, 60, True, 0)))
    e.append(("anchors-one-short", 1, 1, [_c(30, na=2)], (1, 60, False, 0)))
    e.append(("no-anchors", 1, 0, [_c(30, na=0, seq=0), _c(20, na=5, seq=1)], (2, None, False, 0)))
    e.append(("mapq-equal-scores-0", 1, 0, [_c(30, seq=1), _c(30, seq=0)], (2, 0, None, 0)))
    # without EVALUATE_CHAINS the order is the alignment scores' and the walk reads the chaining scores: quotients outside [1/3, 1]
    e.append(("mapq-clamped-at-0", 0, 0, [_c(50, c=10, seq=0), _c(40, c=30, seq=1)], (2, 0, None, 0)))
    e.append(("mapq-clamped-at-60", 0, 0, [_c(50, c=-10, seq=0), _c(40, c=20, seq=1)], (2, 60, None, 0)))
    e.append(("mapq-26", 1, 0, [_c(30, seq=0), _c(third, seq=1)], (2, 26, None, 0)))
    e.append(("denormal-scores", 1, 0, [_c(3e-39, seq=0), _c(2e-39, seq=1), _c(1.5e-39, seq=2)], (3, 13, None, 0)))
    e.append(("keep-mask-empties-the-read", 1, 0, [_c(30, keep=0), _c(20, keep=0, seq=1)], (0, 0, False, None)))
    e.append(("keep-mask-ignored-without-evaluate", 0, 0, [_c(30, c=20, keep=0), _c(20, c=10, keep=0, seq=1)], (2, None, None, 0)))
    e.append(("sixty-four-on-one-spot", 1, 0, [_c(100 + k, c=k) for k in range(64)], (1, 60, None, 63)))
    e.append(("sixty-four-in-a-row", 1, 0, [_c(100 - 0.25 * k, seq=k) for k in range(64)], (64, None, None, 0)))
    e.append(("sixty-five-listed-sixty-four-kept", 1, 0, [_c(100 + k, seq=k, keep=int(k != 7)) for k in range(65)], (64, None, None, 64)))
    return e


def constructed_declines():
    """(name, evaluate, read): each must be declined"""
    nan = f32(np.nan)
    return [
        ("two-equal-records", 1, [_c(30, seq=1), _c(20, seq=2), _c(20, seq=2)]),
        ("two-equal-records-signed-zero", 0, [_c(0.0, c=5, seq=1), _c(-0.0, c=5, seq=1), _c(7, seq=3)]),
        ("zero-best-score", 1, [_c(0.0, seq=0), _c(0.0, seq=1)]),
        ("nan-alignment-score", 1, [_c(30, seq=0), _c(nan, seq=1)]),
        ("nan-chaining-score", 0, [_c(30, c=nan, seq=0), _c(20, seq=1)]),
        ("sixty-five-chains", 0, [_c(100 + k, seq=k) for k in range(65)]),
        ("sixty-five-kept-of-seventy", 1, [_c(100 + k, seq=k, keep=int(k >= 5)) for k in range(70)]),
        ("mapq-product-outside-int", 0, [_c(50, c=1, seq=0), _c(40, c=1e9, seq=1)]),
        ("mapq-quotient-overflows", 0, [_c(50, c=1e-30, seq=0), _c(40, c=1e30, seq=1)]),
        ("stop-rule-divides-by-zero", 0, [_c(50, c=-1, seq=0), _c(40, c=0.0, seq=1)]),
    ]


def edges_round(sel_evaluate):
    """the constructed edges of one (evaluate, select set) as a Round, and their entries"""
    ev, sel = sel_evaluate
    es = [x for x in constructed_edges() if (x[1], x[2]) == (ev, sel)]
    return Round([x[3] for x in es], ev, sel, [x[0] for x in es]), es


def edge_groups():
    return sorted({(x[1], x[2]) for x in constructed_edges()})


def declines_round(evaluate):
    ds = [x for x in constructed_declines() if x[1] == evaluate]
    reads = []
    for x in ds:   # an ordinary read on either side of each: a declined read never declines the round
        reads += [[_c(30, seq=0), _c(20, seq=1)], x[2]]
    reads.append([_c(30, seq=0)])
    return Round(reads, evaluate, 0, [None if i % 2 == 0 else ds[i // 2][0] for i in range(len(reads))])


# ---- which reads the device must decline, from the host's results alone ---------------------------------------------------------
def must_decline(rd: Round, out, primary):
    """bool per read: one of the four stated conditions holds.  The first three are read off the inputs; the fourth off the host's
    primaries (which are defined whenever the first three do not hold)."""
    want = np.zeros(rd.n_reads, bool)
    for r in range(rd.n_reads):
        recs, score, keep = rd.read(r)
        part = np.nonzero(keep != 0)[0] if rd.evaluate else np.arange(len(recs))
        if len(part) > 64:
            want[r] = True
            continue
        a, c = score[part], recs["chaining_score"][part]
        if np.isnan(a).any() or np.isnan(c).any():
            want[r] = True
            continue
        # (float keys compared as values: +0 and -0 are equal, as in the comparator)
        keys = {(float(a[i]) + 0.0, float(c[i]) + 0.0, int(recs["n_anchors"][k]), int(recs["key"][k]), int(recs["start_position"][k]), int(recs["end_position"][k]))
                for i, k in enumerate(part)}
        if len(keys) < len(part):
            want[r] = True
            continue
        n = int(out[r]["n_primary"])
        if n < 2:
            continue
        c0 = int(rd.chain_off[r])
        p0, p1 = int(primary[c0]), int(primary[c0 + 1])
        s = score if rd.evaluate else recs["chaining_score"]
        with np.errstate(all="ignore"):
            q = f32(s[p1]) / f32(s[p0])
            prod = f32(40) * (f32(1) - q)
            if not np.isfinite(q) or not (prod >= f32(-2147483648.0) and prod < f32(2147483648.0)):
                want[r] = True
            elif int(recs["n_anchors"][p0]) != 0 and not np.isfinite(f32(s[p0]) / f32(s[p1])):
                want[r] = True
    return want


def assert_equal_except_declined(rd: Round, got, want, what):
    """a device form's (out, primary) against the host's, bit for bit; declined exactly where must_decline says, and void there"""
    (g_out, g_prim), (w_out, w_prim) = got, want
    decl = must_decline(rd, w_out, w_prim)
    g_decl = (g_out["flags"] & ROUND_DECLINED) != 0
    assert np.array_equal(g_decl, decl), (what, "declined", np.nonzero(g_decl != decl)[0][:10])
    ok = ~decl
    for f in ("n_primary", "mapq", "flags"):
        assert np.array_equal(g_out[f][ok], w_out[f][ok]), (what, f, np.nonzero(ok & (g_out[f] != w_out[f]))[0][:10])
    owner = np.repeat(np.arange(rd.n_reads), np.diff(rd.chain_off).astype(np.int64))
    live = ok[owner]
    assert np.array_equal(g_prim[live], w_prim[live]), (what, "primary", np.nonzero(live & (g_prim != w_prim))[0][:10])
    return decl
