"""The reference from bases on the host (rawdtw_refsig_host.cpp, rawalign_amd/refsig.py): ri_seq_to_sig (src/rsig.cpp:7-41) restated,
against the fixture recorded from the reference's own function in both builds (scripts/make_golden_refsig.py) and against a scalar
restatement written here; the exact step of its two sums against plain serial sums; the model's parser; the FASTA reader.  No GPU."""
import gzip
import math
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

from rawalign_amd import refsig
from rawalign_amd._lib import RawDTWError
from tests.refsig_cases import ADVERSARIAL, LONG, NEG, cases, inputs_sha256, levels, outputs_sha256, same

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_to_sig_ref.npz")
def serial_sums(v):
    s = s2 = 0.0
    for x in np.asarray(v, np.float32).astype(np.float64).tolist():
        s += x
        s2 += x * x  # (exact in double: the fused form of this line changes nothing)
    return s, s2


def scalar_seq_to_sig(seq, pore, k, strand, contracted):
    v = levels(seq, pore, k, strand)
    j = len(v)
    if j == 0:
        return v
    s, s2 = serial_sums(v)
    mean, q = s / j, s2 / j
    if not (math.isfinite(mean) and math.isfinite(q)):
        var = q - mean * mean
    elif contracted:  # fma(-mean, mean, q): the exact value, rounded once
        var = float(Fraction(q) - Fraction(mean) ** 2)
    else:
        var = q - mean * mean
    std = math.sqrt(var) if var >= 0 else math.nan
    with np.errstate(all="ignore"):
        return ((v.astype(np.float64) - mean) / np.float64(std)).astype(np.float32)


def bits(x: float) -> bytes:
    return b"nan" if x != x else struct.pack("<d", x)


def test_inputs_are_the_fixtures():
    assert str(np.load(GOLDEN)["inputs_sha256"]) == inputs_sha256(cases())


@pytest.mark.parametrize("form", ["plain", "contracted"])
def test_host_equals_the_reference_function(form):
    g = np.load(GOLDEN)
    assert list(g["names"]) == [c[0] for c in cases()]
    for i, (name, seqs, pore, k) in enumerate(cases()):
        got = [refsig.seq_to_sig(s, pore, k, strand, form == "contracted") for s in seqs for strand in (1, 0)]
        assert outputs_sha256(got) == g[f"sha256_{form}"][i].tobytes(), name


@pytest.mark.parametrize("contracted", [False, True])
def test_host_equals_a_scalar_restatement(contracted):
    for name, seqs, pore, k in cases():
        for n, s in enumerate(seqs):
            for strand in (1, 0):
                got = refsig.seq_to_sig(s, pore, k, strand, contracted)
                assert len(got) == max(len(s) - k + 1, 0)
                assert same(got, scalar_seq_to_sig(s, pore, k, strand, contracted)), (name, n, strand)
    one = refsig.seq_to_sig(b"A" * 50, cases()[0][2], 3, 0)
    assert len(one) == 48 and np.all(np.isnan(one))  # std_dev 0


def test_bad_arguments():
    pore = np.zeros(64, np.float32)
    for k in (0, 13):
        with pytest.raises(RawDTWError):
            refsig.seq_to_sig(b"ACGTACGT", np.zeros(64, np.float32), k, 0)
    assert len(refsig.seq_to_sig(b"", pore, 3, 1)) == 0 and len(refsig.seq_to_sig(b"AC", pore, 3, 0)) == 0


def test_pore_model_parser(tmp_path):
    rng = np.random.default_rng(3)
    k, want = 4, rng.normal(90, 10, 256).astype(np.float32)
    rows = []
    for slot in rng.permutation(256):
        if slot in (7, 200):
            continue  # never named: 0
        kmer = "".join("ACGT"[(slot >> 2 * (k - 1 - j)) & 3] for j in range(k))
        if slot % 5 == 0:
            kmer = kmer.lower()
        rows.append(f"{kmer}\t{float(want[slot])!r}\t1.5\t0.9\t0.1\n")
    rows.append("NNAC\t12.5\t1\t1\t1\n")  # N -> A: slot of AAAC, and the later row wins
    want[7] = want[200] = 0.0
    want[1] = 12.5
    p = tmp_path / "model.txt"
    p.write_text("#a comment\n# another\nkmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\n" + "".join(rows[:100]) + "#inside\n\n" + "".join(rows[100:]))
    got, gk = refsig.read_pore_model(str(p))
    assert gk == k and got.tobytes() == want.tobytes()
    bad = tmp_path / "bad.txt"
    bad.write_text("ACGT 1.0\nACG 2.0\n")
    with pytest.raises(RawDTWError) as e:
        refsig.read_pore_model(str(bad))
    assert e.value.status == 1
    with pytest.raises(RawDTWError):
        refsig.read_pore_model(str(tmp_path / "absent.txt"))


def test_sums_step_equals_serial_sums_on_the_cases():
    for name, seqs, pore, k in cases():
        for s in seqs:
            for strand in (1, 0):
                v = levels(s, pore, k, strand)
                got_s, got_s2, fast, slow = refsig.seq_sums(v)
                want_s, want_s2 = serial_sums(v)
                assert bits(got_s) == bits(want_s) and bits(got_s2) == bits(want_s2), (name, len(s), strand)
                assert int(fast[0] + slow[0]) == int(fast[1] + slow[1]) == (len(v) + 63) // 64
                if name == NEG:
                    assert fast[0] == 0  # levels at or below 0: the running sum never qualifies


def test_sums_step_equals_serial_sums_on_random_lists():
    rng = np.random.default_rng(77)
    pools = [
        ADVERSARIAL,
        np.array([1.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** 24, 0.5], np.float32),                 # ties against a sum near 1 and 2^24
        np.array([2.0 ** 20, 2.0 ** 20, 1.0, 2.0 ** 21 - 1], np.float32),                                    # binade crossings
        np.array([-1.0, 1.0, 0.0, -0.0, 3.5, -2.0 ** -30], np.float32),                                      # negatives and zeros
        np.array([1e-45, 1e-40, 0.0, 1e-38, 2.0 ** -126], np.float32),                                       # subnormals
        np.array([np.inf, 1.0, -np.inf, 2.0, 3.0e38, 3.4e38], np.float32),                                   # infinities, and squares that overflow nothing
        np.array([90.0, 91.25, 77.125, 101.5], np.float32),
    ]
    total_fast = 0
    for t in range(2000):
        pool = pools[t % len(pools)]
        n = int(rng.integers(0, 400))
        v = pool[rng.integers(0, len(pool), n)]
        if t % 3 == 0 and n:
            v = np.concatenate([rng.uniform(50, 130, 200).astype(np.float32), v])  # a sum well under way when the pool's values come
        got_s, got_s2, fast, slow = refsig.seq_sums(v)
        want_s, want_s2 = serial_sums(v)
        assert bits(got_s) == bits(want_s) and bits(got_s2) == bits(want_s2), (t, n)
        total_fast += int(fast.sum())
    assert total_fast > 0


def test_long_case_walks_fast():
    """behind element 131 072 the algorithm alone gives 1076 of 1077 fast steps for the sum and 1077 of 1077 for the squares' (one binade
    crossing): at least 9 in 10 are asked for, so a build that always walks slowly fails here"""
    name, seqs, pore, k = [c for c in cases() if c[0] == LONG][0]
    for strand in (1, 0):
        v = levels(seqs[0], pore, k, strand)
        _, _, fast_all, slow_all = refsig.seq_sums(v)
        _, _, fast_head, slow_head = refsig.seq_sums(v[:131072])  # (131 072 = 2048 steps: the head's steps are the whole's first ones)
        fast, slow = fast_all - fast_head, slow_all - slow_head
        steps = (len(v) - 131072 + 63) // 64
        for i in range(2):
            assert int(fast[i] + slow[i]) == steps
            print(f"strand {strand} sum{'2' if i else ''}: {int(fast[i])} of {steps} steps fast")
            assert 10 * int(fast[i]) >= 9 * steps


def test_read_fasta(tmp_path):
    text = b">chr1 first sequence\nACGTN\nacgt\n\n>chr2\tx\nGG\n>empty\n>last\nTTTT"
    want = [("chr1", b"ACGTNacgt"), ("chr2", b"GG"), ("empty", b""), ("last", b"TTTT")]
    plain, gz = tmp_path / "ref.fa", tmp_path / "ref.fa.gz"
    plain.write_bytes(text)
    with gzip.open(gz, "wb") as f:
        f.write(text)
    assert refsig.read_fasta(str(plain)) == want and refsig.read_fasta(str(gz)) == want
