"""Inputs of the kept-chains tests (tests/test_round_keep_host.py, tests/test_round_keep_gpu.py): constructed rounds as flat arrays the
way a device-chained round and its round end leave them -- chain_off, recs, anchor_off, anchors, out, primary -- and a plain-Python
restatement of what such a round keeps as the next round's previous seeds (rawalign_amd/csrc/rawdtw_mapper.cpp: write_seeds over a read's
primary chains, best first, each chain's anchors in the order they lie)."""
import functools

import numpy as np

from rawalign_amd.dtw import ANCHOR_DTYPE, CHAIN_REC_DTYPE, NOT_KEPT, ROUND_DECLINED, ROUND_HIGH, ROUND_OUT_DTYPE, SEED_DTYPE

CAP = 300   # the constructed rounds' seeds a half


class KeepRound:
    def __init__(self, reads, seed):
        """reads: per read (chains: a list of n_anchors, primary: indices into it, best first, declined: bool)"""
        rng = np.random.default_rng(seed)
        sizes = [n for ch, _, _ in reads for n in ch]
        self.chain_off = np.zeros(len(reads) + 1, np.uint64)
        self.chain_off[1:] = np.cumsum([len(ch) for ch, _, _ in reads])
        nc = len(sizes)
        self.anchor_off = np.zeros(nc + 1, np.uint64)
        self.anchor_off[1:] = np.cumsum(sizes)
        self.recs = np.zeros(nc, CHAIN_REC_DTYPE)
        self.recs["n_anchors"] = sizes
        self.recs["key"] = rng.integers(0, 14, nc)
        self.recs["chaining_score"] = rng.integers(10, 200, nc)
        na = int(self.anchor_off[-1])
        self.anchors = np.zeros(na, ANCHOR_DTYPE)
        self.anchors["target_position"] = rng.integers(0, 2 ** 31, na)   # (every anchor its own value: a misplaced copy shows)
        self.anchors["query_position"] = np.arange(na, dtype=np.uint32)[::-1]
        self.out = np.zeros(len(reads), ROUND_OUT_DTYPE)
        self.primary = np.full(nc, 0xFFFFFFFF, np.uint32)
        for r, (ch, prim, declined) in enumerate(reads):
            c0 = int(self.chain_off[r])
            self.out[r] = (len(prim), 60 if prim else 0, (ROUND_DECLINED if declined else 0) | (ROUND_HIGH if r % 3 == 0 and not declined else 0))
            self.primary[c0:c0 + len(prim)] = prim

    @property
    def n_reads(self):
        return len(self.chain_off) - 1

    def arrays(self):
        return self.chain_off, self.recs, self.anchor_off, self.anchors, self.out, self.primary


def restate(rd: KeepRound, cap):
    """plain Python: (kept_count per read, per read its seed list as SEED_DTYPE, or None where nothing is kept)"""
    kept, lists = np.zeros(rd.n_reads, np.uint32), []
    for r in range(rd.n_reads):
        c0 = int(rd.chain_off[r])
        rows = []
        for p in range(int(rd.out[r]["n_primary"])):
            c = c0 + int(rd.primary[c0 + p])
            a0 = int(rd.anchor_off[c])
            for k in range(int(rd.recs[c]["n_anchors"])):
                rows.append((int(rd.recs[c]["key"]), int(rd.anchors[a0 + k]["target_position"]), int(rd.anchors[a0 + k]["query_position"])))
        if int(rd.out[r]["flags"]) & ROUND_DECLINED or len(rows) > cap:
            kept[r] = NOT_KEPT
            lists.append(None)
        else:
            kept[r] = len(rows)
            lists.append(np.array(rows, SEED_DTYPE) if rows else np.zeros(0, SEED_DTYPE))
    return kept, lists


def edge_reads():
    """(name, chains, primary, declined) with CAP seeds a half"""
    return [
        ("no-chain-at-all", [], [], False),
        ("chains-but-no-primary", [5, 7], [], False),
        ("one-primary-of-one-anchor", [1], [0], False),
        ("one-primary-among-three", [4, 9, 2], [1], False),
        ("two-primaries-not-in-chain-order-63-64", [64, 12, 63], [2, 0], False),
        ("one-chain-of-65", [65, 3], [0], False),
        ("one-chain-of-200", [200], [0], False),
        ("thirty-two-primaries-shuffled", [1 + (k * 5) % 9 for k in range(32)], [(k * 13 + 5) % 32 for k in range(32)], False),
        ("exactly-the-cap", [100, 17, 200], [2, 0], False),
        ("one-above-the-cap", [200, 101], [0, 1], False),
        ("one-chain-above-the-cap", [CAP + 1, 2], [0], False),
        ("declined", [30, 20], [], True),
        ("declined-with-primaries-listed", [30, 20], [1, 0], True),
        ("sixty-four-primaries-of-four", [4] * 64, list(range(63, -1, -1)), False),
        ("last-read-one-anchor", [1, 1], [1, 0], False),
    ]


@functools.lru_cache(maxsize=None)
def rounds():
    """{name: KeepRound}: the constructed edges as one round, a round of 1 read, and a round of 70 reads drawn at random"""
    out = {"edges": KeepRound([(c, p, d) for _, c, p, d in edge_reads()], 1)}
    out["one-read"] = KeepRound([([64, 12, 63], [2, 0], False)], 2)
    rng = np.random.default_rng(3)
    reads = []
    for r in range(70):
        n = int(rng.choice((0, 1, 2, 3, 8, 32)))
        chains = [int(rng.choice((1, 2, 5, 40, 63, 64, 65, 120))) for _ in range(n)]
        k = int(rng.integers(0, n + 1)) if n else 0
        prim = [int(x) for x in rng.permutation(n)[:k]]
        reads.append((chains, prim, bool(rng.random() < 0.1)))
    out["seventy"] = KeepRound(reads, 4)
    return out


# ---- whole reads: from a host-path run alone, which reads the device round end must decline, and what a read's primary chains hold ------
class _Recording:
    """tests.util.OracleScorer that notes every round's candidates as a round_end_cases.Round"""

    def __init__(self, inner, evaluate):
        self.inner, self.evaluate, self.rounds = inner, evaluate, []

    def __getattr__(self, k):
        return getattr(self.inner, k)

    def score(self, reads, opt):
        from tests import round_end_cases as R

        kept = self.inner.score(reads, opt)
        rows = []
        for (_, chains), k in zip(reads, kept):
            ids = {id(c) for c in k}
            rows.append([(np.float32(c.alignment_score), np.float32(c.chaining_score), c.n_anchors, c.strand, c.reference_sequence_index, c.start_position,
                          c.end_position, int(id(c) in ids)) for c in chains])
        self.rounds.append(R.Round(rows, self.evaluate))
        return kept


@functools.lru_cache(maxsize=None)
def whole_reads_host_run(name, form):
    """The Python mirror over tests/golden/map_ref_reads.npz with the oracle's scorer (no device): (reads the device round end would have to
    decline over the run -- round_end_cases.must_decline: more than 64 chains taking part, two equal on all seven keys, a NaN, a quotient
    that is not finite --, every (read, round)'s total of primary-chain anchors after a round that chained)"""
    from oracle.loader import Oracle
    from rawalign_amd import mapper
    from rawalign_amd.mapping import StopOpt
    from tests import map_ref_cases as K
    from tests import round_end_cases as R
    from tests.util import OracleScorer

    wr = K.WholeReads(form)
    opt, copt = K.whole_project_opts(name, form)
    rec = _Recording(OracleScorer(Oracle(), wr.ref), bool(opt.flag & K.EVAL))
    totals = []
    mapper.map_reads(wr, list(range(wr.n_reads)), rec, opt, StopOpt(), chain_opt=copt, output_chains=True,
                     on_round=lambda rnd, chains: totals.extend(sum(c.n_anchors for c in ch) for ch in chains.values()))
    declined = 0
    for rd in rec.rounds:
        out, primary = rd.host()
        declined += int(R.must_decline(rd, out, primary).sum())
    return declined, totals
