"""The lanes of the chaining DP's predecessor loop (chain_step in rawalign_amd/csrc/rawdtw_chain.hip, rmap.cpp:452-484): constructed reads
that put the loop's exit, its winner, the skip counter it carries from 64 candidates to the next, exact ties and the value edges of the
scoring and of the end filter where the inputs of the other chaining tests never put them, and a tracer that says where they are.  No tests
in here: tests/test_chain_lattice_cpu.py pins the cases and their coverage on the host, tests/test_chain_lattice_gpu.py runs them.

A PROBE READ is one (sequence, strand) list whose last anchor A = (T, Q) is the probe.  The candidates behind it are laid down by their
OFFSET d = ai - 1 - pi (block d // 64, lane d % 64 of chain_step) at targets T - (300 + d), and by kind at queries chosen so that no two
of them chain with each other: every one but A scores e = 1 000 (asserted by the CPU module), A scores e + (300 + w) for its winner at
offset w, and the read reports the one chain [A, winner] -- or none, when the loop has to end before any improver.

  kind  query        towards A                                               towards the others (a pair is at most 279 targets apart)
  I     Q - 1 400    improver: cur = e + min(300 + d, 1 400, e), rising in d  each other: same query, passed over
  S     Q - 3 000    skipper: gap = |300 + d - 3 000| >= 2 000, cur = 0       query difference >= 1 600 over <= 279 targets: scale >= 5
  P1    Q            passed over (same query)
  P2    Q-3 001-d    passed over (same target T; offsets from 0 only)         every other query is higher: qd < 0
  P3    Q + 1 400    passed over (qd < 0)                                     1 400 / 279 > 5 towards P1
  T     Q-(300+x)    equal to the improver at offset x < d: e + 300 + x       (only in the short tie probes)
  G     Q + 1 400    target T - 5 001: ends the loop (rmap.cpp:460)           far-away fillers behind it share its query

The skip counter of a probe is the number of S (and losing T) less the number of I so far.  Every probe says what it expects (`want`);
the CPU module asserts that the tracer finds exactly that."""
import numpy as np

from rawalign_amd import mapping as M
from tests.test_device_chain import SEED_DTYPE
from tests.test_mapping_host import f32, py_chain

E = 1000
T0, Q0, A0 = 1_000_000, 10_000, 300
Q_I, Q_S, Q_P2, Q_P3 = 1400, 3000, 3001, 1400
BLOCKS = 3
SKIP_ROUNDS = (0, 1, 2, 3, 25)
BANDS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193)
RESIDUES = (0, 1, 31, 62, 63)
RESIDUE_OFFSETS = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192)   # exits there, winners right in front: lane 0, lane 63, either side of a boundary
TIE_LANES = (15, 31, 47, 62, 63)          # the nearer candidate's offset; the farther one is the next (63 / 64: across the boundary)
CARRIES_25 = (-100, -64, -17, -16, -15, -2, -1, 0, 1, 24, 25)
FRONT_LIST = 37                           # anchors of the list in front of a band or residue probe's: g0 is no multiple of 64


def chain_opt(max_skips=25, band=5000, nbest=3, min_score=10.0, e=E, max_gap=2000, max_tgap=5000, min_anchors=2):
    return M.ChainOpt(max_gap, max_tgap, band, max_skips, min_anchors, nbest, min_score, e, 0)


def py_kwargs(copt):
    return dict(e=copt.e, max_gap=copt.max_gap_length, max_tgap=copt.max_target_gap_length, band=copt.chaining_band_length,
                max_skips=copt.max_num_skips, min_anchors=copt.min_num_anchors, nbest=copt.num_best_chains, min_score=copt.min_chaining_score)


# ------------------------------------------------------------------------------------------------------------------------
# the tracer: py_chain over a read's lists as the mapper runs them (running maximum across the lists), tracing the probe
# ------------------------------------------------------------------------------------------------------------------------
def sorted_lists(seeds):
    order = np.lexsort((seeds["query_position"], seeds["target_position"], seeds["key"]))
    s = seeds[order]
    return [(int(key), s[s["key"] == key]) for key in np.unique(s["key"])]


def trace_read(seeds, copt, probe_only=True):
    """-> (chains [(score, key, [(target, query) ...])] as generated, running maximum, the trace of the last list's anchors -- of its last
    anchor alone when probe_only --, the DP values of the last list)"""
    chains, maxs, tr, dp = [], 0.0, [], []
    lists = sorted_lists(seeds)
    for k, (key, g) in enumerate(lists):
        last = k == len(lists) - 1
        tr, dp = [], []
        got, maxs = py_chain(g, maxs=maxs, dp_out=dp, trace=tr if last else None, trace_from=len(g) - 1 if probe_only else 0, **py_kwargs(copt))
        for score, idx in got:
            chains.append((f32(score), key, [(int(g[i]["target_position"]), int(g[i]["query_position"])) for i in idx]))
    return chains, maxs, tr, dp


# ------------------------------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------------------------------
def lay(seq, fillers=0, front=0, rng=None):
    """seq[d]: the kind of the candidate at offset d ("I", "S", "P1", "P2", "P3", "G", or ("T", x)); `fillers` far-away anchors behind a
    closing G; `front` anchors of another list in front of the probe's.  -> the read's seeds, shuffled"""
    rows = [(1, T0, Q0)]
    for d, kind in enumerate(seq):
        a = A0 + d
        if kind == "P2":
            assert all(k == "P2" for k in seq[:d])
            rows.append((1, T0, Q0 - Q_P2 - d))
        elif kind == "G":
            assert d == len(seq) - 1
            rows.append((1, T0 - 5001, Q0 + Q_P3))
        elif isinstance(kind, tuple):
            rows.append((1, T0 - a, Q0 - (A0 + kind[1])))
        else:
            rows.append((1, T0 - a, Q0 + {"I": -Q_I, "S": -Q_S, "P1": 0, "P3": Q_P3}[kind]))
    if fillers:
        assert seq and seq[-1] == "G"
    rows += [(1, T0 - 10000 - 6000 * i, Q0 + Q_P3) for i in range(fillers)]
    rows += [(0, 500 + 7000 * i, 5) for i in range(front)]   # one query, more than max_target_gap_length apart: no chain, maximum e
    s = np.array(rows, dtype=np.int64)
    out = np.zeros(len(rows), SEED_DTYPE)
    out["key"], out["target_position"], out["query_position"] = s[:, 0], s[:, 1], s[:, 2]
    return out[rng.permutation(len(out))] if rng is not None else out


def fill(length, actives):
    """`length` candidates: `actives` {offset: kind} among pass-over candidates of all three kinds (P2 only in front of the first active one)"""
    first = min(actives) if actives else length
    n_p2 = min(length % 4, first)
    seq = []
    for d in range(length):
        seq.append(actives[d] if d in actives else ("P2" if d < n_p2 else ("P1", "P3")[d % 2]))
    return seq


def spread(n_slots, kinds):
    """the kinds in order at evenly spread offsets of [0, n_slots)"""
    assert len(kinds) <= n_slots
    pos = [int(x) for x in np.floor(np.linspace(0, n_slots - 1, len(kinds)))] if len(kinds) > 1 else [n_slots - 1] * len(kinds)
    assert len(set(pos)) == len(pos)
    return dict(zip(pos, kinds))


def skip_exit_seq(d, m):
    """the loop ends by the skip counter at offset d under max_num_skips = m (d >= m).  With room: a low improver, m + 1 skippers (the counter
    stands at m), the winner, a skipper (m again), and the one at d (m + 1): a loop that ends one skipper early loses the winner, one that
    goes on takes the bait behind d."""
    assert d >= m
    if d >= m + 5:
        act = spread(d, ["I"] + ["S"] * (m + 1) + ["I", "S"])
    elif d >= m + 2:
        act = {0: "I", **{d - 1 - i: "S" for i in range(m + 1)}}
    else:
        act = {d - 1 - i: "S" for i in range(m)}
    winner = max([o for o, k in act.items() if k == "I"], default=None)
    return fill(d, act) + ["S", "I", "G"], winner


def gap_exit_actives(d, m):
    """candidates in front of an exit at offset d that is not the skip counter's: the winner right in front of it (a loop that ends one
    early loses it), behind a lower improver in block 0 once the winner is in block 1 or 2, and up to two skippers"""
    act = {}
    if d >= 1:
        act[d - 1] = "I"
    if d - 1 >= 64:
        act[(d * 7) % 64] = "I"
    for o in (d // 3, (2 * d) // 3)[:min(m, 2)]:
        if o not in act and o < d:
            act[o] = "S"
    return act, (d - 1 if d >= 1 else None)


def carry_seq(m, c, boundary):
    """the skip counter is c on entry to block `boundary`: a run of -c improvers up to the boundary and three more across it, or c skippers;
    then skippers up to m, a winner, a skipper, the skipper that ends the loop, and the bait.  c == m: the exit is lane 0 of that block."""
    base = 64 * boundary
    act, cc = {}, c
    assert -base <= c <= m
    if c < 0:
        for i in range(-c):
            act[base - 1 - i] = "I"
        for i in range(3):
            act[base + i] = "I"
        cc, at = c - 3, base + 3
    else:
        for i in range(c):
            act[base - 1 - i] = "S"
        at = base
    if cc < m:
        for _ in range(m - cc):
            act[at] = "S"
            at += 1
        act[at], act[at + 1] = "I", "S"
        winner, at = at, at + 2
    else:
        winner = max([o for o, k in act.items() if k == "I"], default=None)
    return fill(at, act) + ["S", "I", "G"], at, winner


def residue_fillers(seq, residue):
    """so many fillers behind the closing G that the probe's index in its read is `residue` modulo 64"""
    return (residue - len(seq)) % 64


def probe(family, name, seeds, **want):
    return {"family": family, "name": name, "seeds": seeds, "want": want}


def lattice_round(m, rng):
    """every probe of one max_num_skips"""
    out = []
    for d in range(64 * BLOCKS):
        if d >= m:
            seq, w = skip_exit_seq(d, m)
            out.append(probe("exit_skip", "skip m=%d d=%d" % (m, d), lay(seq, rng=rng), exit="skip", exit_off=d, last=w))
        if m in (0, 25):
            act, w = gap_exit_actives(d, m)
            out.append(probe("exit_gap", "gap m=%d d=%d" % (m, d), lay(fill(d, act) + ["G"], rng=rng), exit="gap", exit_off=d, last=w))
            out.append(probe("exit_start", "start m=%d d=%d" % (m, d), lay(fill(d, act), rng=rng), exit="band", exit_off=d, last=w))
    # the carried counter
    carries = CARRIES_25 if m == 25 else tuple(range(-1, m + 1))
    for c in carries:
        for boundary in (1, 2):
            if -c > 64 * boundary:
                continue
            seq, d, w = carry_seq(m, c, boundary)
            out.append(probe("carry", "carry m=%d c=%d block=%d" % (m, c, boundary), lay(seq, rng=rng), exit="skip", exit_off=d, last=w,
                             carry=(boundary, c)))
    # the long path's residues: exits and winners at lane 0, lane 63 and either side of the block boundaries
    if m == 25:
        for d in RESIDUE_OFFSETS:
            for res in RESIDUES:
                act, w = gap_exit_actives(d, m)
                seq = fill(d, act) + ["G"]
                out.append(probe("residue", "gap d=%d index=%d mod 64" % (d, res), lay(seq, fillers=residue_fillers(seq, res), rng=rng),
                                 exit="gap", exit_off=d, last=w, residue=res))
                out.append(probe("residue", "start d=%d index=%d mod 64" % (d, res), lay(fill(d, act), front=(res - d) % 64 or 64, rng=rng),
                                 exit="band", exit_off=d, last=w, residue=res))
                if d >= 30:
                    seq, w = skip_exit_seq(d, m)
                    out.append(probe("residue", "skip d=%d index=%d mod 64" % (d, res), lay(seq, fillers=residue_fillers(seq, res), rng=rng),
                                     exit="skip", exit_off=d, last=w, residue=res))
        # exact ties: the improver at x and a candidate of the same value at x + 1 -- the nearer wins, the farther is a skip
        for x in TIE_LANES:
            act = {3: "I", x: "I", x + 1: ("T", x), x + 2: "S"}
            out.append(probe("tie", "tie %d/%d" % (x, x + 1), lay(fill(x + 3, act) + ["G"], rng=rng), exit="gap", exit_off=x + 3, last=x, tie=(x, x + 1)))
    if m == 3:
        # ... and the farther one's skip is the one past max_num_skips: low improver -1, four skippers 3, the improver 2, a skipper 3, the tie 4
        for x in (20, 62):
            act = {0: "I", 2: "S", 5: "S", 9: "S", 12: "S", x: "I", x + 1: "S", x + 2: ("T", x)}
            out.append(probe("tie", "tie %d/%d ends the loop" % (x, x + 2), lay(fill(x + 2, act) + [("T", x), "I", "G"], rng=rng),
                             exit="skip", exit_off=x + 2, last=x, tie=(x, x + 2)))
    return out


def band_round(band, rng):
    """the band's true end at offset `band`, in a list that is not the read's first (lo is list-relative): the winner is the last candidate
    inside, the bait the first one outside"""
    out = []
    for extra in (1, 5):
        act, w = gap_exit_actives(band, 25)
        seq = fill(band, act) + ["I"] + ["P3"] * (extra - 1)
        out.append(probe("exit_band", "band %d + %d" % (band, extra), lay(seq, front=FRONT_LIST, rng=rng), exit="band", exit_off=band, last=w))
    return out


# ---- value edges --------------------------------------------------------------------------------------------------------
def pair_read(td, qd, rng, t=50_000, q=20_000):
    """the probe and one candidate td targets and qd queries in front of it"""
    s = np.zeros(2, SEED_DTYPE)
    s["target_position"], s["query_position"] = (t, t + td), (q, q + qd)
    return s[rng.permutation(2)]


# (td, qd, scores) at e = 1 000, max_gap_length 2 000, max_target_gap_length 5 000
VALUE_EDGES = [
    ("gap == max_gap_length - 1", 1000, 2999, True), ("gap == max_gap_length", 1000, 3000, False),
    ("scale == 0.75", 400, 300, False), ("scale just above 0.75", 400, 301, True), ("scale == 5", 100, 500, False), ("scale just below 5", 100, 499, True),
    ("td 1 qd 1", 1, 1, True), ("td 2 qd 3", 2, 3, True), ("td 5 qd 4", 5, 4, True), ("td e-1 qd e-1", E - 1, E - 1, True), ("td e qd e", E, E, True),
    ("td e+1 qd e", E + 1, E, True),
    ("pt + max_target_gap_length == ct", 5000, 4500, True), ("pt + max_target_gap_length == ct - 1", 5001, 4500, False),
]
# ... the gap's edge from the other side (qd < td): with scale > 0.75 that needs td > 7 996, so max_target_gap_length is 20 000 in this round
VALUE_EDGES_WIDE = [("gap == max_gap_length - 1, qd < td", 12000, 10001, True), ("gap == max_gap_length, qd < td", 12000, 10000, False),
                    ("pt + max_target_gap_length == ct, wide", 20000, 18500, True), ("pt + max_target_gap_length == ct - 1, wide", 20001, 18500, False)]
# the rounding pair (max_gap_length = max_target_gap_length = 2^30): td = 4k, qd = 3k + 1 with k above 2^23 -- the true ratio is above 0.75, its
# fp32 quotient is 0.75f (no score); qd = 3k + 3 gives the next float up (a score).  A kernel that compared qd with 0.75 td would score both.
ROUND_K = (1 << 23) + 1
ROUND_TD, ROUND_QD_FLAT, ROUND_QD_UP = 4 * ROUND_K, 3 * ROUND_K + 1, 3 * ROUND_K + 3
assert all(int(f32(x)) == x for x in (ROUND_TD, ROUND_QD_FLAT, ROUND_QD_UP))   # (the conversions are exact: the quotient alone rounds)
assert ROUND_QD_FLAT * 4 > 3 * ROUND_TD
assert f32(f32(ROUND_QD_FLAT) / f32(ROUND_TD)) == f32(0.75)
assert f32(f32(ROUND_QD_UP) / f32(ROUND_TD)) == np.nextafter(f32(0.75), f32(1))


def value_round(rng, edges=VALUE_EDGES):
    return [probe("value", name, pair_read(td, qd, rng), scores=sc, td=td, qd=qd) for name, td, qd, sc in edges]


def rounding_round(rng):
    return [probe("value", "rounding pair: quotient 0.75f", pair_read(ROUND_TD, ROUND_QD_FLAT, rng, t=7, q=3), scores=False, td=ROUND_TD, qd=ROUND_QD_FLAT),
            probe("value", "rounding pair: next float up", pair_read(ROUND_TD, ROUND_QD_UP, rng, t=7, q=3), scores=True, td=ROUND_TD, qd=ROUND_QD_UP)]


def value_round_e6(rng):
    """matching < e at the default e = 6: two anchors on a diagonal (12) in front of the candidate pair, so that the probe passes min_chaining_score"""
    out = []
    for td, qd in ((1, 1), (3, 4), (5, 5), (6, 6), (7, 6), (7, 7)):
        s = np.zeros(3, SEED_DTYPE)
        s["target_position"], s["query_position"] = (1000, 1006, 1006 + td), (100, 106, 106 + qd)
        out.append(probe("value", "e=6 td %d qd %d" % (td, qd), s[rng.permutation(3)], score=12 + min(td, qd, 6)))
    return out


# ---- the end filter and the traceback's break -------------------------------------------------------------------------
def diagonal(key, t0, n, step=6):
    s = np.zeros(n, SEED_DTYPE)
    s["key"], s["target_position"], s["query_position"] = key, t0 + step * np.arange(n), 10 + step * np.arange(n)
    return s


def end_filter_reads(rng):
    """e = 6, min_chaining_score 18: a diagonal of n anchors six apart scores 6 n.  -> [(name, seeds, {num_best_chains: chain scores as generated})]"""
    sh = lambda parts: (lambda s: s[rng.permutation(len(s))])(np.concatenate(parts))
    return [
        # list 0 sets the maximum, 48; list 1's best is 24 == 48 / 2: not an end
        ("best == maxs / 2", sh([diagonal(0, 1000, 8), diagonal(1, 1000, 4)]), {1: [48.0], 50: [48.0]}),
        # ... and one e above: an end
        ("best == maxs / 2 + e", sh([diagonal(0, 1000, 8), diagonal(1, 1000, 5)]), {1: [48.0, 30.0], 50: [48.0, 30.0]}),
        ("best == min_chaining_score", sh([diagonal(0, 1000, 3)]), {1: [18.0], 50: [18.0]}),
        ("best == min_chaining_score - e", sh([diagonal(0, 1000, 2)]), {1: [], 50: []}),
        # one list, three diagonals more than max_target_gap_length apart: 18, 24, 48.  Ends by (score, index) descending: the 48's anchors down
        # to 24 == maxs / 2 (no break), the 24 diagonal's end (a chain, no break), the 48's anchor of 18 (used; below half: break) -- the 18
        # diagonal, an end, is never reached.  With one best chain only the 48 is.
        ("traceback break", sh([diagonal(0, 1000, 3), diagonal(0, 9000, 4), diagonal(0, 17000, 8)]), {1: [48.0], 50: [48.0, 24.0]}),
    ]


# ------------------------------------------------------------------------------------------------------------------------
# the rounds: (name, options, probes)
# ------------------------------------------------------------------------------------------------------------------------
def rounds():
    rng = np.random.default_rng(20261020)
    out = [("skips %d" % m, chain_opt(max_skips=m), lattice_round(m, rng)) for m in SKIP_ROUNDS]
    out += [("band %d" % b, chain_opt(band=b), band_round(b, rng)) for b in BANDS]
    out.append(("values", chain_opt(), value_round(rng)))
    out.append(("values wide", chain_opt(max_tgap=20000), value_round(rng, VALUE_EDGES_WIDE)))
    out.append(("rounding", chain_opt(max_gap=1 << 30, max_tgap=1 << 30), rounding_round(rng)))
    out.append(("values e=6", chain_opt(e=6), value_round_e6(rng)))
    ef = end_filter_reads(rng)
    for nbest in (1, 50):
        out.append(("end filter, %d best" % nbest, chain_opt(e=6, min_score=18.0, nbest=nbest),
                    [probe("end", name, seeds, chain_scores=want[nbest]) for name, seeds, want in ef]))
    return out


# cells of the coverage table that no input can reach, by name
UNREACHABLE = {
    "exit_skip": "under max_num_skips = m the counter passes m at the (m + 1)-th non-improver at the earliest: no exit by skip at an offset below m "
                 "(offsets 0 .. m - 1 of block 0 in the rounds with m = 1, 2, 3, 25; the round with m = 0 has them all)",
    "exit_band multiple of 64": "a band or list that ends after a multiple of 64 candidates ends the kernel's loop by its bound (base < lo), not on a lane: "
                                "offsets 64, 128 and 192 are run and traced, and are lane 0 of no block",
    "gap late": "a loop that missed the exit by max_target_gap_length at one candidate meets it at the next: every farther candidate's target is lower "
                "still, or its query is the probe's; only an early exit shows, by the winner right in front of the gap anchor",
}
