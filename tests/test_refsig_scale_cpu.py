"""What tests/test_refsig_scale_gpu.py relies on, held on the host: the numpy restatement of ri_seq_to_sig (tests/refsig_scale_cases.py)
equals the host restatement bit for bit -- on every earlier case, at k = 1, 2, 7, 12 and on a strand of 8 388 608 elements -- and the
inputs of the table tests cross the thresholds they are there for by the host's own counts.  No GPU; nothing reads the reference."""
import numpy as np
import pytest

from rawalign_amd import refsig, seeding
from rawalign_amd.seeding import SeedIndex, SeedParams
from tests import refsig_cases as rc
from tests import refsig_scale_cases as sc


@pytest.fixture(scope="module", autouse=True)
def release_cases():
    yield
    sc.release()


@pytest.mark.parametrize("contracted", [False, True])
def test_numpy_equals_host_on_the_earlier_cases(contracted):
    for name, seqs, pore, k in rc.cases():
        for n, s in enumerate(seqs):
            for strand in (1, 0):
                want = sc.np_seq_to_sig(s, pore, k, strand, contracted)
                got = refsig.seq_to_sig(s, pore, k, strand, contracted)
                assert rc.same(got, want), (name, n, strand)
                if name == "one_letter_k6":  # std_dev 0: both say NaN throughout
                    assert len(want) and np.all(np.isnan(want)) and np.all(np.isnan(got))


@pytest.mark.parametrize("contracted", [False, True])
@pytest.mark.parametrize("k", sc.SMALL_KS)
def test_numpy_equals_host_at_small_and_large_k(k, contracted):
    name, seqs, pore, kk = [c for c in sc.small_k_cases() if c[3] == k][0]
    assert kk == k and len(pore) == 4 ** k
    assert [max(len(s) - k + 1, 0) for s in seqs] == [0, 0] + list(sc.SMALL_S_LENS)
    for n, s in enumerate(seqs):
        for strand in (1, 0):
            got = refsig.seq_to_sig(s, pore, k, strand, contracted)
            assert len(got) == max(len(s) - k + 1, 0)
            assert rc.same(got, sc.np_seq_to_sig(s, pore, k, strand, contracted)), (name, n, strand)
            if len(got) > 1:
                assert np.all(np.isfinite(got))


def test_long_cases_are_what_the_staging_loop_needs():
    """the lengths in pieces of STAGE_BYTES, and lower case and N on both sides of every multiple"""
    cases = {name: seqs for name, seqs, _, _ in sc.long_cases()}
    pieces = lambda seqs: [[min(sc.STAGE_BYTES, len(s) - at) for at in range(0, len(s), sc.STAGE_BYTES)] for s in seqs]
    assert pieces(cases["split_tail"]) == [[1000], [sc.STAGE_BYTES, 5], [70]]  # pieces 3 and 4 wait for a buffer; base_off 1000
    assert pieces(cases["split_exact"]) == [[sc.STAGE_BYTES], [3]]             # no empty piece; then a sequence below k
    assert pieces(cases["split_three"]) == [[sc.STAGE_BYTES, sc.STAGE_BYTES, 1000]]   # the third piece starts where two have been
    three = cases["split_three"][0][2 * sc.STAGE_BYTES - 3:2 * sc.STAGE_BYTES + 4]
    assert len(three) == 7 and not any(c in b"ACGT" for c in three)
    for s in (cases["split_tail"][1], cases["split_exact"][0], cases["split_three"][0]):
        near = s[sc.STAGE_BYTES - 3:sc.STAGE_BYTES + 4]
        assert len(near) >= 3 and not any(c in b"ACGT" for c in near) and b"N" in near[:3]
    assert b"N" in cases["split_tail"][1][sc.STAGE_BYTES:sc.STAGE_BYTES + 4]


@pytest.mark.parametrize("contracted", [False, True])
def test_numpy_equals_host_on_a_strand_past_the_staging_buffer(contracted):
    """the one place the host restatement runs at this length: a strand of split_tail's long sequence (the other strand and split_exact
    are held to numpy on the device alone)"""
    name, seqs, pore, k = sc.long_case("split_tail")
    s = seqs[1]
    assert len(s) > sc.STAGE_BYTES and len(s) - k + 1 > 3 * sc.GRID_STRIDE_ELEMS
    got = refsig.seq_to_sig(s, pore, k, 0, contracted)
    assert rc.same(got, sc.np_seq_to_sig(s, pore, k, 0, contracted))
    assert np.all(np.isfinite(got))
    if not contracted:  # the exact step's two doubles against the strictly sequential sums
        v = rc.levels(s, pore, k, 0)
        x = v.astype(np.float64)
        s1, s2, fast, slow = refsig.seq_sums(v)
        assert s1 == float(np.cumsum(x)[-1]) and s2 == float(np.cumsum(x * x)[-1])
        assert int(fast[0] + slow[0]) == int(fast[1] + slow[1]) == (len(v) + 63) // 64


# ---- the table's thresholds, by the host's own counts ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genome():
    return sc.table_genome()


def test_default_table_crosses_the_sort_and_the_grid_thresholds(genome):
    fwd, rev = genome
    assert len(fwd) == 9  # seq_bits = 4, id 8 in the top bit
    six = SeedIndex.from_signals(fwd, rev, SeedParams(), threads=16)
    assert six.n_positions > sc.MERGE_SORT_LIMIT
    # entries of the long sequence's forward strand alone: the sketch of the whole strand, the filter rule the table is built by
    n_fwd = len(seeding.sketch(fwd[0], SeedParams())[0])
    print(f"entries: {six.n_positions} in all, {n_fwd} of the long sequence's forward strand")
    assert n_fwd > sc.GRID_STRIDE_ELEMS
    cut = SeedIndex.from_signals(fwd[:2], rev[:2], SeedParams(), threads=16)
    assert cut.n_positions > sc.MERGE_SORT_LIMIT // 2 and cut.n_seq == 2


def test_low_entropy_and_widest_parameters(genome):
    fwd, rev = genome
    full = SeedIndex.from_signals(fwd, rev, SeedParams(), threads=16).n_positions
    low = SeedIndex.from_signals(fwd, rev, SeedParams(e=2, lq=1), threads=16)
    assert low.n_keys < 100 and low.n_positions > sc.MERGE_SORT_LIMIT
    # every kept event but the first e - 1 of a strand ends an entry: e = 2 has 4 more entries a strand than e = 6
    assert low.n_positions == full + 4 * 2 * len(fwd)
    assert sum(len(low.get(h)) for h in low.keys().tolist()) == low.n_positions
    assert max(len(low.get(h)) for h in low.keys().tolist()) > 40_000
    mid = SeedIndex.from_signals(fwd, rev, SeedParams(e=3, lq=2), threads=16)
    assert mid.n_keys < 5000 and mid.n_positions > sc.MERGE_SORT_LIMIT
    wide = SeedIndex.from_signals(fwd, rev, SeedParams(e=9, lq=5, q=32), threads=16)  # 63 of 64 bits: accepted
    assert wide.pars == SeedParams(e=9, lq=5, q=32) and wide.n_positions > sc.MERGE_SORT_LIMIT and wide.n_keys > sc.MERGE_SORT_LIMIT // 2
