"""Inputs of the tests that turn the opt-in device paths on together (tests/test_optins_together_gpu.py, tests/test_optins_cases_cpu.py):
the caps on seeds a read that put some (read, round) pairs of the fixtures on each side of a threshold, the per-(read, round) seed counts
they were read from -- computed on the host alone --, and the option setters the GPU cases share.  No tests here.

A read's seed count in a round is what rawdtw_chain_round_begin* sees as its seed_off stretch: the anchors of the primary chains the round
before left (write_seeds, rawdtw_mapper.cpp) plus the chunk's hits; a read whose chunk is below min_events sits the round out and is not
chained.  A count above RAWDTW_CHAIN_MAX_SEEDS goes to k_chain_long with "chain_long_seeds" on, and makes the whole round fall back to the
host with it off."""
import numpy as np

import rawalign_amd as ra
from rawalign_amd import mapper, seeding, synth
from rawalign_amd.events import detect_events_host
from rawalign_amd.mapping import StopOpt
from rawalign_amd.rawsig import detect_events_raw_host
from tests import map_ref_cases as mc

ALL_ON = dict(device_round_end=1, resident_chains=4096, chain_long_seeds=65536)
A_SETS = ("default", "global_full", "frac025")

# ---- the caps and what they cut.  Measured by tests/test_optins_cases_cpu.py, which prints the figures and fails when a generator drifts. ----
# whole reads, w = 0 index, default stop rule -- the three sets of case A chain the same lists: 14 (read, round) pairs of 3 .. 162 seeds
# (build 1: 3 .. 157), per-round maxima 140, 111, 162 (140, 109, 157)
L_MIX = 107     # their median, and one read's count exactly: 7 pairs above it, 7 at or below
L_ALL = 60      # the value tests/test_chain_long_mapper_gpu.py uses: all but the 4 pairs of under 60 seeds (reads from nowhere) are long
# per build: pairs chained, pairs above (L_MIX, L_ALL), per round the reads that enter it with previous anchors and those anchors
WHOLE = {0: dict(pairs=14, above=[7, 10], prev_reads=[0, 1, 1], prev_seeds=[0, 51, 77]),
         1: dict(pairs=14, above=[7, 10], prev_reads=[0, 1, 1], prev_seeds=[0, 46, 72])}
# whole reads, w = 5 index, default stop rule: 14 pairs of 0 .. 42 seeds (build 1: 0 .. 41), per-round maxima 40, 30, 42 (40, 30, 41)
L_MIX5 = 26
WHOLE5 = {0: dict(pairs=14, above=[7], prev_reads=[0, 1, 1], prev_seeds=[0, 11, 17]),
          1: dict(pairs=14, above=[7], prev_reads=[0, 1, 1], prev_seeds=[0, 10, 16])}
# whole reads (build 0), w = 0 index, a stop rule that never fires: per-round maxima 140, 191, 280, 267
C_FB = 270      # rounds 1, 2 and 4 at or below it, round 3 above: resident, resident, a fall-back, resident
FB_MAXIMA = [140, 191, 280, 267]
FB_FALLS_BACK = [False, False, True, False]
FB_PREVIOUS = [(0, 0), (4, 311), (6, 644), (1, 243)]   # per round (reads with previous anchors, those anchors)
# the int16 flow of tests/test_signal_round_gpu.py, default stop rule: 43 pairs of 364 .. 734 seeds, per-round maxima 734, 649, 722, 494 -- above
# every count of the whole reads, so the flow has a cap of its own
L_MIX_FLOW = 505
FLOW = dict(pairs=43, above=[21], prev_reads=[0, 0, 0, 0], prev_seeds=[0, 0, 0, 0])
# ... and the same flow under SIT_STOP with read SITTER's second window cut to 300 samples: 61 pairs of 364 .. 778 seeds, maxima 734, 778, 740, 688
SITTER, SITTER_ANCHORS = 0, 65
SIT_STOP = dict(min_bestmap_ratio=1e9, min_meanmap_ratio=1e9, min_chain_anchor=100)   # a read stops on a sole primary chain of 100 anchors
FLOW_SIT = dict(pairs=61, above=[35], prev_reads=[0, 6, 6, 5], prev_seeds=[0, 412, 452, 256])


def flow_with_a_sitter(flow):
    """the flow with read SITTER's second window cut to 300 samples (about 30 events, below min_events): under SIT_STOP it sits round 2 out
    holding the chains round 1 left it"""
    sref, si, chan, window, counts = flow
    return sref, si, chan, lambda r, c: window(r, c)[:300] if (r, c) == (SITTER, 1) else window(r, c), counts


def all_on(e, **more):
    """every opt-in of the fast flow on the engine's context; -> the engine"""
    for k, v in dict(ALL_ON, **more).items():
        e.set_option(k, v)
        assert e.get_option(k) == v, k
    return e


class HostChunks:
    """The Python mirror's view of reads given as windows of samples: chunk(r, c) -> (the window's events from the host's detection, the
    events' hits from seeding.seed_hits_host as (sequence, strand, target, query) tuples), computed once.  windows[r][c]: float32 pA samples, or
    with `chan` int16 DAC samples."""

    def __init__(self, si, windows, seq_lens, jobs, event_opt=None, chan=None):
        self.si, self.lens, self.jobs, self.n_reads = si, np.asarray(seq_lens), jobs, len(windows)
        flat = [w for ws in windows for w in ws]
        first = np.concatenate([[0], np.cumsum([len(ws) for ws in windows])])
        off = np.concatenate([[0], np.cumsum([len(w) for w in flat])]).astype(np.uint64)
        if chan is None:
            eoff, ev = detect_events_host(np.concatenate(flat + [np.zeros(0, np.float32)]).astype(np.float32), off, event_opt, threads=8)
        else:
            raw = np.concatenate(flat + [np.zeros(0, np.int16)]).astype(np.int16)
            _, eoff, ev = detect_events_raw_host(raw, off, chan, event_opt, threads=8)
        hoff, hits = seeding.seed_hits_host(si, ev, eoff, threads=8)
        tup = list(zip(hits["ref_seq"].tolist(), hits["strand"].tolist(), hits["target_position"].tolist(), hits["query_position"].tolist()))
        self._chunks = [[(ev[int(eoff[k]):int(eoff[k + 1])], tup[int(hoff[k]):int(hoff[k + 1])]) for k in range(first[r], first[r + 1])]
                        for r in range(self.n_reads)]

    def n_chunks(self, r):
        return len(self._chunks[r])

    def chunk(self, r, c):
        return self._chunks[r][c]

    def read_job(self, r):
        j = self.jobs[r]
        return mapper.ReadJob(j.name, qlen=j.qlen, n_chunks_available=j.n_chunks_available)


def whole_chunks(si, wr, raws, form):
    """the whole reads' pA windows (mc.raw_chunks) as HostChunks, for one build"""
    return HostChunks(si, [mc.raw_chunks(sig) for sig in raws], wr.lens, [wr.read_job(r) for r in range(wr.n_reads)],
                      ra.EventOptions(contracted=bool(form)))


def flow_chunks(flow, n_reads, n_chunks):
    """tests/test_signal_round_gpu.py's int16 flow as HostChunks"""
    sref, si, chan, window, _ = flow
    jobs = [mapper.ReadJob("read_%d" % r, qlen=4000 * n_chunks, n_chunks_available=n_chunks) for r in range(n_reads)]
    return HostChunks(si, [[window(r, c) for c in range(n_chunks)] for r in range(n_reads)], [len(sref.forward[0])], jobs, chan=chan)


def seed_counts(src, oracle, ref, opt, copt, stop):
    """(per round {read: (previous primary-chain anchors, the chunk's hits)} over the reads the round chains, the reads the device's round end
    would have to decline over the run) -- the anchors from the Python mirror with the oracle's scorer, the hits from the host's seeding, the
    declines from round_end_cases.must_decline on the mirror's candidates.  All reads start together: a read's chunk in round k is its k-th."""
    from tests import round_end_cases as R
    from tests.round_keep_cases import _Recording
    from tests.util import OracleScorer

    prev, rounds = {r: 0 for r in range(src.n_reads)}, []

    def on_round(rnd, chains):
        row = {}
        for r, ch in chains.items():
            ev, hits = src.chunk(r, rnd - 1)
            if len(ev) >= stop.min_events:
                row[r] = (prev[r], len(hits))
            prev[r] = sum(c.n_anchors for c in ch)
        rounds.append(row)

    rec = _Recording(OracleScorer(oracle, ref), bool(opt.flag & mc.EVAL))
    mapper.map_reads(src, list(range(src.n_reads)), rec, opt, stop, chain_opt=copt, output_chains=True, on_round=on_round)
    declined = 0
    for rd in rec.rounds:
        out, primary = rd.host()
        declined += int(R.must_decline(rd, out, primary).sum())
    return rounds, declined


def maxima(rounds):
    return [max(p + h for p, h in row.values()) if row else 0 for row in rounds]


def flat_counts(rounds):
    return sorted(p + h for row in rounds for p, h in row.values())


def above(rounds, cap):
    """the (read, round) pairs whose seed count is above a cap: what rawdtw_chain_round_stats counts as long_reads"""
    return sum(c > cap for c in flat_counts(rounds))


def with_previous(rounds):
    """per round (reads chained that have previous anchors, those anchors): what rawdtw_mapper_kept_stats counts, from either source"""
    return [(sum(1 for p, _ in row.values() if p), sum(p for p, _ in row.values())) for row in rounds]


def candidate_counts(src, oracle, ref, opt, copt, stop):
    """per round {read: the candidate chains its chaining leaves} (0 for a read that sits out), from the Python mirror"""
    from tests.round_keep_cases import _Recording
    from tests.util import OracleScorer

    order = []
    rec = _Recording(OracleScorer(oracle, ref), bool(opt.flag & mc.EVAL))
    mapper.map_reads(src, list(range(src.n_reads)), rec, opt, stop, chain_opt=copt, output_chains=True, on_round=lambda rnd, chains: order.append(list(chains)))
    return [{r: int(rd.chain_off[i + 1] - rd.chain_off[i]) for i, r in enumerate(reads)} for reads, rd in zip(order, rec.rounds)]


# ---- a read the chaining's end declines: more than 32 candidate chains in one round ----
class EventReads(mapper.IndexSeeds):
    """mapper.IndexSeeds (reads as lists of chunks of events, hits from the host's seeding) with every chunk's hits computed once"""

    def __init__(self, seed_index, reads, seq_lens):
        super().__init__(seed_index, reads, seq_lens)
        self.n_reads = len(self.reads)
        self._chunks = [[mapper.IndexSeeds.chunk(self, r, c) for c in range(len(ch))] for r, ch in enumerate(self.reads)]

    def n_chunks(self, r):
        return len(self.reads[r])

    def chunk(self, r, c):
        return self._chunks[r][c]


DECLINER, DECLINED_ROUND = 0, 1   # the read, and the round (0-based) in which it has 34 candidate chains
# measured (a stop rule that never fires): per-round maxima of the seed counts 115, 725, 254, 273; every other (read, round) has one candidate chain
DECLINE_MAXIMA = [115, 725, 254, 273]
DECLINE_PREVIOUS = [(0, 0), (3, 267), (4, 378), (4, 486)]   # per round (reads with previous anchors, those anchors)
DECLINE_CANDIDATES = 34


def decline_case():
    """Six sequences of 3 000 events that carry the same stretch three times on either strand's array, and four reads of four chunks.  Read
    DECLINER's second chunk is 150 events of that stretch: up to three chains on each of twelve (sequence, strand) lists, 34 candidate chains
    -- above the 32 the device chaining keeps a read, so rawdtw_chain_round_end declines the round.  Every other chunk comes from a
    stretch that occurs once.  -> (reference, per read its chunks of events)"""
    base = synth.make_reference([3000] * 6, seed=4242)
    stretch = synth.make_reference([400], seed=4243).forward[0].copy()
    fwd, rev = [x.copy() for x in base.forward], [x.copy() for x in base.reverse]
    for s in range(6):
        for arr in (fwd[s], rev[s]):
            for at in (200, 1200, 2200):
                arr[at:at + len(stretch)] = stretch
    rng = np.random.default_rng(4244)

    def noisy(x):
        return (x + rng.normal(0, 0.05, len(x))).astype(np.float32)

    reads = [[noisy(fwd[1][1020:1100]), noisy(stretch[:150]), noisy(fwd[1][1650:2050]), noisy(fwd[1][2650:2950])]]
    for s in (2, 3, 4):
        reads.append([noisy(fwd[s][650:1050]), noisy(fwd[s][1050:1200]), noisy(fwd[s][1650:2050]), noisy(fwd[s][2650:2950])])
    return synth.Reference(fwd, rev, base.names), reads


def never():
    return StopOpt(**mc.NEVER)
