"""Inputs of the tests of "chain_max_chains" (tests/test_chain_many_gpu.py; checked on the host alone by tests/test_chain_many_cases_cpu.py): reads
with more than 16 and more than 32 candidate chains, most of them with equal scores -- what a reference of many sequences gives every
round, num_best_chains chains on each (sequence, strand) list with scores that are sums of small integers.  No tests here.

  mixed_round      constructed lists: 50 reads of 20 .. 120 lists of one chain of 2 .. 6 anchors each, among 50 random reads
  seeded_round     real seeding: 60 reads of 400 events on 48 sequences of 10 000 events, hits from seeding.seed_hits_host
  mapper_reads     24 reads of three chunks on the same reference, as a source for mapper.map_reads_c"""
import functools

import numpy as np

from rawalign_amd import mapper, seeding, synth
from tests.test_device_chain import SEED_DTYPE, host_chains, random_read

N_SEQ, SEQ_LEN, REF_SEED = 48, 10_000, 77
MIXED_KEYS = 128


def counts(lib, copt, per_read):
    """per read (its candidate chains, whether two of them have equal scores), from the host's chaining; and the chains themselves"""
    chains = [host_chains(lib, copt, s) for s in per_read]
    return [(len(c), len({float(x[0]) for x in c}) < len(c)) for c in chains], chains


def tied_above(cnt, k):
    return sum(1 for n, tie in cnt if n > k and tie)


def above(cnt, k):
    return sum(1 for n, _ in cnt if n > k)


def read_of_little_chains(rng, n_lists):
    """n_lists (sequence, strand) lists with one chain of 2 .. 6 anchors each, steps of 5, 6 or 10 in target and query: scores 6 + (anchors - 1)
    * 5 or 6, a handful of integers.  The lists' keys are drawn from all MIXED_KEYS, the seeds shuffled."""
    keys = rng.permutation(MIXED_KEYS)[:n_lists]
    parts = []
    for key in keys:
        n, step = int(rng.integers(2, 7)), int(rng.choice([5, 6, 10]))
        s = np.zeros(n, SEED_DTYPE)
        s["key"] = key
        s["target_position"] = int(rng.integers(0, 50_000)) + step * np.arange(n)
        s["query_position"] = int(rng.integers(0, 300)) + step * np.arange(n)
        parts.append(s)
    s = np.concatenate(parts)
    return s[rng.permutation(len(s))]


@functools.lru_cache(maxsize=None)
def _mixed():
    rng = np.random.default_rng(1701)
    many = [read_of_little_chains(rng, int(rng.integers(20, 121))) for _ in range(50)]
    few = [random_read(rng, int(rng.integers(20, 300)), 4, 5000) for _ in range(50)]
    order = rng.permutation(100)
    return [(many + few)[k] for k in order]


def mixed_round():
    return [s.copy() for s in _mixed()]


@functools.lru_cache(maxsize=None)
def reference():
    return synth.make_reference([SEQ_LEN] * N_SEQ, seed=REF_SEED)


@functools.lru_cache(maxsize=None)
def seed_index():
    ref = reference()
    return seeding.SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)


def event_reads(n_reads, n_events, seed):
    """event-level reads: a stretch of a sequence's forward or reverse array with noise of sd 0.05 .. 0.3; every tenth read from nowhere"""
    ref, rng = reference(), np.random.default_rng(seed)
    reads = []
    for r in range(n_reads):
        if r % 10 == 9:
            reads.append(rng.normal(0, 1, n_events).astype(np.float32))
            continue
        arr = (ref.forward, ref.reverse)[int(rng.integers(0, 2))][int(rng.integers(0, N_SEQ))]
        at = int(rng.integers(0, len(arr) - n_events))
        reads.append((arr[at:at + n_events] + rng.normal(0, rng.uniform(0.05, 0.3), n_events)).astype(np.float32))
    return reads


@functools.lru_cache(maxsize=None)
def _seeded():
    reads = event_reads(60, 400, 4801)
    off = np.arange(len(reads) + 1, dtype=np.uint64) * 400
    hoff, hits = seeding.seed_hits_host(seed_index(), np.concatenate(reads), off, threads=4)
    per_read = []
    for r in range(len(reads)):
        h = hits[int(hoff[r]):int(hoff[r + 1])]
        s = np.zeros(len(h), SEED_DTYPE)
        s["key"] = h["ref_seq"].astype(np.uint32) * 2 + h["strand"].astype(np.uint32)
        s["target_position"], s["query_position"] = h["target_position"], h["query_position"]
        per_read.append(s)
    return reads, per_read


def seeded_round():
    """(the reads' events, per read its seeds: key = sequence * 2 + strand)"""
    reads, per_read = _seeded()
    return reads, [s.copy() for s in per_read]


MAPPER_READS, MAPPER_CHUNKS = 24, 3


@functools.lru_cache(maxsize=None)
def mapper_reads():
    """24 reads of three chunks of 400 events on the 48 sequences, behind mapper.IndexSeeds with every chunk's hits computed once"""
    from tests.optins_cases import EventReads

    whole = event_reads(MAPPER_READS, 400 * MAPPER_CHUNKS, 4802)
    chunks = [[x[400 * c:400 * (c + 1)] for c in range(MAPPER_CHUNKS)] for x in whole]
    return EventReads(seed_index(), chunks, [SEQ_LEN] * N_SEQ)
