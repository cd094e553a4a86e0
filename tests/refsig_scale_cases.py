"""Seeded inputs and references of the index build's scale tests (tests/test_refsig_scale_cpu.py, tests/test_refsig_scale_gpu.py): inputs
past the sizes at which rawdtw_refsig.hip, rawdtw_seed_build.hip and rawdtw_index.cpp change what they do, and a numpy restatement of
ri_seq_to_sig (src/rsig.cpp:7-41) that shares nothing with the library but tests.refsig_cases.levels.  The CPU module holds the host
restatement and the host's own counts to these inputs; the GPU module holds the device to both.  Nothing here reads the reference."""
import functools
import math
from fractions import Fraction

import numpy as np

from tests import refsig_cases as rc

STAGE_BYTES = 8_388_608          # rawdtw_refsig.hip, rawdtw_reference_from_bases: `const size_t CH = 8u << 20`, bytes a staging buffer
GRID_STRIDE_ELEMS = 1024 * 256   # rawdtw_refsig.hip `gy = min((max_s_len + 255) / 256, 1024)` and rawdtw_seed_build.hip the same on max_n: blocks of 256
MERGE_SORT_LIMIT = 1_048_576     # rocprim/device/detail/device_radix_sort_config.hpp:50 `merge_sort_limit = 1024 * 1024`: onesweep only above it
INDEX_STAGE_FLOATS = 16_777_216  # rawdtw_index.cpp, rawdtw_index_upload: `const size_t CH = 16u << 20`, floats a staging buffer

SMALL_KS = (1, 2, 7, 12)         # kModelLdsMaxK = 6: 7 is the first model in global memory; kMaxK = 12: a 24-bit k-mer; 1 and 2: the shortest
SMALL_S_LENS = (1, 63, 64, 65, 4097)


def np_seq_to_sig(seq, pore, k: int, strand: int, contracted: bool) -> np.ndarray:
    """ri_seq_to_sig of one strand: the two sums strictly in order (np.cumsum is sequential; np.sum is pairwise and would not do)"""
    v = rc.levels(seq, pore, k, strand)
    n = len(v)
    if n == 0:
        return np.zeros(0, np.float32)
    x = v.astype(np.float64)
    s, s2 = float(np.cumsum(x)[-1]), float(np.cumsum(x * x)[-1])  # (a float's square is exact in double)
    mean, q = s / n, s2 / n
    with np.errstate(all="ignore"):
        if contracted and math.isfinite(mean) and math.isfinite(q):
            var = float(Fraction(q) - Fraction(mean) ** 2)  # fma(-mean, mean, q): the exact value, rounded once (correctly, by float())
            sd = np.float64(math.sqrt(var)) if var >= 0 else np.float64(np.nan)
        else:
            sd = np.sqrt(np.float64(q) - np.float64(mean) * np.float64(mean))
        return ((x - mean) / sd).astype(np.float32)


def _around_stage_multiples(s: bytearray):
    """lower case and N within three bases on either side of every multiple of STAGE_BYTES the sequence reaches"""
    for m in range(STAGE_BYTES, len(s) + 4, STAGE_BYTES):
        for at in range(m - 3, m + 4):
            if 0 <= at < len(s):
                s[at] = ord("N") if (at - m) % 3 == 0 else ord(bytes([s[at]]).lower())


LONG_NAMES = ("split_tail", "split_exact", "split_three")


def release():
    """drop what the cached generators hold (a module calls it when it is done: the long cases are tens of megabytes)"""
    for f in (long_cases, small_k_cases, table_genome):
        f.cache_clear()


def long_case(name):
    return [c for c in long_cases() if c[0] == name][0]


@functools.lru_cache(maxsize=1)
def long_cases():
    """split_tail: one piece; a sequence in two pieces, the second of 5 bytes and the first to wait for a buffer; a fourth piece that waits
    again; base_off not 0.  split_exact: a sequence that is exactly one piece (no empty piece, nothing lost), then one shorter than k.
    split_three: one sequence in three pieces -- only from the third piece on does it matter that the place in the sequence adds up."""
    from rawalign_amd.synth import make_pore_model

    rng = np.random.default_rng(20261020)
    pore = make_pore_model(6)
    out = []
    for name, lens in (("split_tail", [1000, STAGE_BYTES + 5, 70]), ("split_exact", [STAGE_BYTES, 3]),
                       ("split_three", [2 * STAGE_BYTES + 1000])):
        seqs = []
        for n in lens:
            s = bytearray(rc._bases(rng, n))
            _around_stage_multiples(s)
            seqs.append(bytes(s))
        out.append((name, seqs, pore, 6))
    assert tuple(c[0] for c in out) == LONG_NAMES
    return out


@functools.lru_cache(maxsize=1)
def small_k_cases():
    """k below and above what the suite had (3, 6, 9): s_len around a step of 64 and many steps, an empty sequence, one of k - 1 bases"""
    from rawalign_amd.synth import make_pore_model

    rng = np.random.default_rng(20261021)
    out = []
    for k in SMALL_KS:
        pore = make_pore_model(k, seed=100 + k)  # (k = 12: 64 MiB, made once)
        seqs = [b"", rc._bases(rng, k - 1)] + [rc._bases(rng, n + k - 1) for n in SMALL_S_LENS]
        out.append((f"small_k{k}", seqs, pore, k))
    return out


TABLE_LENS = (400_000,) + (40_000,) * 8


@functools.lru_cache(maxsize=1)
def table_genome():
    """(forward arrays, reverse arrays) of nine sequences: with the default parameters more than MERGE_SORT_LIMIT entries in all and more
    than GRID_STRIDE_ELEMS from one strand of the long one (the CPU module asserts both from the host's own counts); nine sequences are
    seq_bits = 4 with id 8 in the top bit"""
    from rawalign_amd import refsig
    from rawalign_amd.synth import make_pore_model

    rng = np.random.default_rng(20261022)
    pore = make_pore_model(6)
    seqs = [rc._bases(rng, n) for n in TABLE_LENS]
    return ([refsig.seq_to_sig(s, pore, 6, 1) for s in seqs], [refsig.seq_to_sig(s, pore, 6, 0) for s in seqs])


def table_genome_cut():
    """the long sequence and one short one: n_seq = 2, seq_bits = 1"""
    fwd, rev = table_genome()
    return fwd[:2], rev[:2]
