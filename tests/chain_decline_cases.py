"""Inputs of the tests of "chain_decline_reads" (tests/test_chain_decline_gpu.py; checked on the host alone by
tests/test_chain_decline_cases_cpu.py): rounds in which some reads are above the device chaining's caps and the others are not.

THE ROUND-LEVEL CASE, under a cap of SEED_CAP = 128 seeds a read (RAWDTW_CHAIN_MAX_SEEDS): ten reads --
    0  one seed                      5  a read of 33 lists with one chain each (99 seeds): more than 32 chains
    1  128 seeds, at the cap         6  an ordinary read
    2  129 seeds, just above it      7  a read of 17 lists with one chain each (102 seeds), two of the chains with equal scores
    3  300 seeds                     8  an ordinary read
    4  an ordinary read              9  no seed
Reads 2 and 3 decline for their seeds (reason 1) and are adjacent; read 5 for its chains (2, and 4: its chains are all equal), read 7 for the
order only std::sort knows (4).  With "chain_max_chains" = 8 the caps are 8 chains and no tie rule: reads 5 and 7 decline with reason 2.
Three orders: as given; ROTATED by two, so that a declined read is first; and that list REVERSED, so that a declined read is last.
Two more rounds: one where every read is above the cap on seeds, one where none declines.  Everything is made from fixed seeds."""
import numpy as np

from tests.test_device_chain import SEED_DTYPE, random_read

SEED_CAP = 128
N_KEYS = 40
MANY = 8            # "chain_max_chains" of the second run
DECLINED = {0: {2: 1, 3: 1, 5: 6, 7: 4}, MANY: {2: 1, 3: 1, 5: 2, 7: 2}}   # read -> reason, as given; pinned by the CPU test


def one_chain_lists(steps_of_list):
    """a list (key) for each entry: a chain of len(steps) + 1 anchors on one diagonal, the given steps apart -- its score is e + sum(min(step, e))"""
    out = []
    for key, steps in enumerate(steps_of_list):
        pos = np.concatenate([[0], np.cumsum(steps)])
        s = np.zeros(len(pos), SEED_DTYPE)
        s["key"], s["target_position"], s["query_position"] = key, 100 + pos, 5 + pos
        out.append(s)
    return np.concatenate(out)


def thirty_three_chains():
    return one_chain_lists([[6, 6]] * 33)


def seventeen_chains_two_equal():
    """17 lists of six anchors: scores 6 + 13 .. 6 + 28 (five steps of 1 .. 6), all distinct, and the last list's equal to the fourth's"""
    def steps(total):   # five steps of 1 .. 6 with this sum
        st = [1] * 5
        for i in range(5):
            add = min(5, total - sum(st))
            st[i] += add
        assert sum(st) == total
        return st
    return one_chain_lists([steps(13 + i) for i in range(16)] + [steps(13 + 3)])


def round_reads():
    rng = np.random.default_rng(2024)
    shuffle = lambda s: s[rng.permutation(len(s))]   # noqa: E731  (the seeds come unsorted)
    return [random_read(rng, 1, 2, 100), random_read(rng, SEED_CAP, 2, 4000), random_read(rng, SEED_CAP + 1, 2, 4000), random_read(rng, 300, 3, 9000),
            random_read(rng, 60, 2, 2000), shuffle(thirty_three_chains()), random_read(rng, 100, 2, 3000), shuffle(seventeen_chains_two_equal()),
            random_read(rng, 40, 1, 1500), np.zeros(0, SEED_DTYPE)]


def orders():
    """name -> the case's read indices in that order"""
    given = list(range(10))
    rotated = given[2:] + given[:2]
    return dict(given=given, rotated=rotated, reversed=rotated[::-1])


def all_above():
    rng = np.random.default_rng(2025)
    return [random_read(rng, n, 2, 6000) for n in (129, 300, 200, 130, 257)]


def none_above():
    rng = np.random.default_rng(2026)
    return [random_read(rng, n, 2, 3000) for n in (0, 1, 128, 64, 65, 100, 17)] + [one_chain_lists([[6, 6]] * 16)]


# ---- the mapper-level cases: tests/optins_cases.py's inputs under caps at which some (read, round) pairs decline.  The figures are computed on the
# host alone by tests/test_chain_decline_cases_cpu.py (optins_cases.seed_counts / candidate_counts against the caps) and recorded here, next to
# optins_cases.C_FB and L_MIX_FLOW which they rest on; a generator that drifts fails there.  Per case: the cap on seeds a read (None: the
# device's own 2 048), the (read, round) pairs chained, per round the reads declined, the reads declined by reason, the other reads of the
# rounds with declines (per round; a mapper with two read groups counts them per group), the declined reads' seeds, and per round (reads, seeds) taken from the store / sent up from the host as previous
# seeds -- a declined read is not kept, so it alone is seeded from the host in the round after. ----
WHOLE_CAP = 110     # whole reads, default stop rule: counts 3 .. 162; five pairs above it, read 4 in rounds 2 and 3
MAPPER_CASES = {
    "whole_fb": dict(cap=270, pairs=23, declined=[[], [], [0], []], by_seeds=1, by_chains=0, chained_device=5, declined_seeds=280,
                     from_device=[(0, 0), (4, 311), (6, 644), (0, 0)], from_host=[(0, 0), (0, 0), (0, 0), (1, 243)]),
    "whole_default": dict(cap=WHOLE_CAP, pairs=14, chained=[[0, 1, 2, 3, 4, 5, 6, 7, 8], [4, 5, 6, 8], [4]], declined=[[0, 1, 7], [4], [4]], by_seeds=5, by_chains=0, chained_device=9, declined_seeds=664,
                          from_device=[(0, 0), (1, 51), (0, 0)], from_host=[(0, 0), (0, 0), (1, 77)]),
    "decline_case": dict(cap=None, pairs=16, declined=[[], [0], [], []], by_seeds=0, by_chains=1, chained_device=3, declined_seeds=725,
                         from_device=[(0, 0), (3, 267), (3, 357), (4, 486)], from_host=[(0, 0), (0, 0), (1, 21), (0, 0)]),
    # the int16 flow under optins_cases.L_MIX_FLOW: 21 of 43 pairs above the cap in rounds 1 .. 3, none in round 4; no read enters a round with chains
    "flow": dict(cap=505, pairs=43, declined=None, by_seeds=21, by_chains=0, chained_device=20, declined_seeds=None, from_device=[(0, 0)] * 4,
                 from_host=[(0, 0)] * 4, rounds_with_declines=3),
}


def mapper_figures(rounds, cands, cap, max_chains=32, tie_free=16):
    """a case's figures from optins_cases.seed_counts' rows ({read: (previous anchors, hits)} a round) and candidate_counts' ({read: chains}):
    a read declines for its seeds above the cap, else for more than max_chains chains (no read of these cases has more than tie_free chains
    otherwise, which the caller asserts: ties cannot decline).  A declined read is seeded from the host in its next round."""
    cap = 2048 if cap is None else cap
    declined, by_seeds, by_chains, chained, dseeds, from_dev, from_host, lost = [], 0, 0, 0, 0, [], [], set()
    for row, cnd in zip(rounds, cands):
        d_seeds = sorted(r for r, (p, h) in row.items() if p + h > cap)
        d_chains = sorted(r for r in row if r not in d_seeds and cnd.get(r, 0) > max_chains)
        assert all(cnd.get(r, 0) <= tie_free for r in row if r not in d_seeds and r not in d_chains)
        dcl = sorted(d_seeds + d_chains)
        declined.append(dcl)
        by_seeds += len(d_seeds)
        by_chains += len(d_chains)
        chained += len(row) - len(dcl) if dcl else 0
        dseeds += sum(sum(row[r]) for r in dcl)
        from_dev.append((sum(1 for r, (p, _) in row.items() if p and r not in lost), sum(p for r, (p, _) in row.items() if r not in lost)))
        from_host.append((sum(1 for r, (p, _) in row.items() if p and r in lost), sum(p for r, (p, _) in row.items() if r in lost)))
        lost = (lost - set(row)) | set(dcl)   # (a read that sits a round out keeps its state)
    return dict(pairs=sum(len(row) for row in rounds), chained=[sorted(row) for row in rounds], declined=declined, by_seeds=by_seeds, by_chains=by_chains, chained_device=chained, declined_seeds=dseeds,
                from_device=from_dev, from_host=from_host)
