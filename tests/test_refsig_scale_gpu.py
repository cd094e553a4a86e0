"""The index build past its own thresholds on the device (inputs and references: tests/refsig_scale_cases.py, held on the host by
tests/test_refsig_scale_cpu.py): a sequence that crosses the 8 MiB staging buffers in pieces, strands of more than 1024 x 256 elements
and entries (the grid-stride loops of k_refsig_write and k_sb_emit), a seed table of more than 2^20 entries (rocPRIM's onesweep radix sort,
where below it a merge sort runs), seq_bits at 1 and 4, 63 of 64 code bits, k = 1, 2, 7, 12, position lists of tens of thousands through
k_seed_write's all-lanes path, and a .ind strand read from the file in pieces.  Exact equality everywhere; a NaN equals a NaN."""
import importlib.util
import os

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import refsig, seeding, synth
from rawalign_amd.index import Index, write_index
from rawalign_amd.seeding import SeedIndex, SeedParams
from tests import refsig_cases as rc
from tests import refsig_scale_cases as sc

pytestmark = pytest.mark.gpu

DEFAULT, WIDE, LOW, MID = SeedParams(), SeedParams(e=9, lq=5, q=32), SeedParams(e=2, lq=1), SeedParams(e=3, lq=2)
PARS = {"default": DEFAULT, "e9_lq5_q32": WIDE, "e2_lq1": LOW, "e3_lq2": MID}


@pytest.fixture(scope="module")
def eng():
    e = ra.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def other():
    """a second engine: what rawdtw_upload_reference lays out for the same arrays"""
    e = ra.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def refs():
    """what the arena tests are held to, each computed once and shared: want(name, contracted) is numpy's answer for a case in one form as
    [strand 1, strand 0 of sequence 0, ...]; walk(name) the fast and slow steps of both sums as the host's walk of the same step takes
    them, every strand's summed (the form changes nothing).  Everything cached goes with the module."""
    cache = {}

    def case(name):
        return sc.long_case(name) if name in sc.LONG_NAMES else [c for c in sc.small_k_cases() + rc.cases() if c[0] == name][0]

    class Refs:
        @staticmethod
        def want(name, contracted):
            if (name, contracted) not in cache:
                _, seqs, pore, k = case(name)
                cache[(name, contracted)] = [sc.np_seq_to_sig(s, pore, k, strand, contracted) for s in seqs for strand in (1, 0)]
            return cache[(name, contracted)]

        @staticmethod
        def walk(name):
            if name not in cache:
                _, seqs, pore, k = case(name)
                fast, slow = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
                for s in seqs:
                    for strand in (1, 0):
                        v = refsig.seq_sums(rc.levels(s, pore, k, strand))
                        fast, slow = fast + v[2], slow + v[3]
                cache[name] = (fast, slow)
            return cache[name]
    yield Refs
    cache.clear()
    sc.release()


def arena_equals(eng, seqs, want, what):
    for s in range(len(seqs)):
        for slot, strand in enumerate((1, 0)):
            got = eng.reference_fetch(s, strand)
            assert rc.same(got, want[2 * s + slot]), (what, s, strand)


def offsets_equal(eng, other, forward, reverse):
    other.upload_reference(forward, reverse)
    for s in range(len(forward)):
        for strand in (0, 1):
            assert eng.reference_offset(s, strand) == other.reference_offset(s, strand), (s, strand)


# ---- A. the arena ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contracted", [False, True])
@pytest.mark.parametrize("name", sc.LONG_NAMES)
def test_long_arena_equals_numpy(eng, other, refs, name, contracted):
    """a sequence in several pieces through the two staging buffers (the third piece of a call waits for buffer 0; split_three's third
    piece is the first whose place in its sequence is a sum), and strands of 32 and 65 trips of k_refsig_write's grid-stride loop"""
    _, seqs, pore, k = sc.long_case(name)
    eng.reference_from_bases(seqs, pore, k, contracted)
    want = refs.want(name, contracted)
    arena_equals(eng, seqs, want, name)
    st = eng.reference_build_stats()
    steps = 2 * sum((max(len(s) - k + 1, 0) + 63) // 64 for s in seqs)
    assert int(st["fast_steps"][0] + st["slow_steps"][0]) == int(st["fast_steps"][1] + st["slow_steps"][1]) == steps
    fast, slow = refs.walk(name)
    assert st["fast_steps"].tolist() == fast.tolist() and st["slow_steps"].tolist() == slow.tolist()
    assert fast[0] > 0 and fast[1] > 0
    print(f"{name} contracted={contracted}: sums {st['sums_ms']:.1f} ms, write {st['write_ms']:.1f} ms")
    offsets_equal(eng, other, want[0::2], want[1::2])


@pytest.mark.parametrize("contracted", [False, True])
@pytest.mark.parametrize("k", sc.SMALL_KS)
def test_small_and_large_k_arena_equals_numpy(eng, refs, k, contracted):
    """k = 7: the first model that stays in global memory; k = 12: the largest, a 24-bit k-mer; k = 1, 2: the smallest"""
    name, seqs, pore, kk = [c for c in sc.small_k_cases() if c[3] == k][0]
    eng.reference_from_bases(seqs, pore, k, contracted)
    arena_equals(eng, seqs, refs.want(name, contracted), name)
    st = eng.reference_build_stats()
    steps = 2 * sum((max(len(s) - k + 1, 0) + 63) // 64 for s in seqs)
    assert int(st["fast_steps"][0] + st["slow_steps"][0]) == int(st["fast_steps"][1] + st["slow_steps"][1]) == steps


def test_a_small_build_behind_a_long_one(eng, refs):
    """the staging buffers and the old arena of a long build are gone cleanly: the next build on the engine is its own"""
    name, seqs, pore, k = sc.long_case("split_exact")
    eng.reference_from_bases(seqs, pore, k, True)
    assert rc.same(eng.reference_fetch(1, 1), np.zeros(0, np.float32))
    name, seqs, pore, k = [c for c in rc.cases() if c[0] == "mixed37_k6"][0]
    eng.reference_from_bases(seqs, pore, k, True)
    arena_equals(eng, seqs, refs.want(name, True), name)
    st = eng.reference_build_stats()
    assert int(st["fast_steps"][0] + st["slow_steps"][0]) == 2 * sum((max(len(s) - k + 1, 0) + 63) // 64 for s in seqs)


# ---- B. the table above 2^20 entries ------------------------------------------------------------------------------------------------------
def same_header(got: SeedIndex, want: SeedIndex, what):
    assert (got.n_seq, got.n_keys, got.n_positions, got.table_bytes) == (want.n_seq, want.n_keys, want.n_positions, want.table_bytes), what
    assert got.pars == want.pars, what
    assert np.array_equal(got.keys(), want.keys()), what


def same_lists(got: SeedIndex, want: SeedIndex, hashes, what):
    for h in hashes:
        assert np.array_equal(got.get(h), want.get(h)), (what, h)


def sampled(want: SeedIndex, n, seed):
    keys = want.keys()
    pick = keys if len(keys) <= n else np.random.default_rng(seed).choice(keys, n, replace=False)
    return pick.tolist() + [0, 1, 0xFFFFFFFF]


@pytest.fixture(scope="module")
def tables(eng):
    """(device table, host table) of table_genome() by parameter set, each built once and shared"""
    built = {}

    def get(name):
        if name not in built:
            fwd, rev = sc.table_genome()
            eng.upload_reference(fwd, rev)
            got = SeedIndex.from_device(eng, PARS[name])
            print(f"{name}: {eng.seed_build_stats()}")
            built[name] = (got, SeedIndex.from_signals(fwd, rev, PARS[name], threads=16))
        return built[name]
    return get


@pytest.mark.parametrize("name", ["e2_lq1", "e3_lq2"])
def test_low_entropy_table_equals_host_list_for_list(tables, name):
    """few keys, each with tens of thousands of positions of every sequence and both strands: equal hashes come out in y order only if the
    second sort is stable above 2^20 entries, and in the order of the sequence ids only if the first one looks at all seq_bits"""
    got, want = tables(name)
    assert want.n_positions > sc.MERGE_SORT_LIMIT and want.n_keys < 5000
    same_header(got, want, name)
    keys = want.keys().tolist()
    same_lists(got, want, keys + [0, 1, 0xFFFFFFFF], name)
    longest = max((want.get(h) for h in keys), key=len)
    assert len(longest) > (40_000 if name == "e2_lq1" else 4_000)
    ids = longest >> np.uint64(32)
    assert np.all(np.diff(longest.astype(np.int64)) > 0) and ids[0] == 0 and ids[-1] == 8  # ascending: sequence 0 first, sequence 8 last


@pytest.mark.parametrize("name", ["default", "e9_lq5_q32"])
def test_big_table_equals_host(tables, name):
    """more than 2^20 entries through the radix sort, more than 1024 x 256 of one strand through k_sb_emit's grid-stride loop; with
    e = 9, lq = 5 the mask of the packed codes is 63 of 64 bits"""
    got, want = tables(name)
    assert want.n_positions > sc.MERGE_SORT_LIMIT
    same_header(got, want, name)
    pick = sampled(want, 20_000, 5)
    same_lists(got, want, pick, name)
    if name == "default":  # seq_bits = 4: id 8 needs the top bit, and it sorts behind id 0
        both = [y for y in (want.get(h) for h in pick) if len(y) > 1 and y[0] >> np.uint64(32) == 0 and y[-1] >> np.uint64(32) == 8]
        assert both


def test_two_sequence_table_equals_host(eng):
    """n_seq = 2: seq_bits = 1, the first sort's end bit at 33"""
    fwd, rev = sc.table_genome_cut()
    eng.upload_reference(fwd, rev)
    want = SeedIndex.from_signals(fwd, rev, DEFAULT, threads=16)
    got = SeedIndex.from_device(eng, DEFAULT)
    assert want.n_seq == 2 and want.n_positions > sc.GRID_STRIDE_ELEMS
    same_header(got, want, "cut")
    pick = sampled(want, 20_000, 6)
    same_lists(got, want, pick, "cut")
    assert any(len(y) > 1 and y[0] >> np.uint64(32) == 0 and y[-1] >> np.uint64(32) == 1 for y in (want.get(h) for h in pick))


@pytest.mark.parametrize("name", ["one_letter_k6", "mixed37_k6"])
def test_table_from_an_arena_built_from_bases(eng, name):
    """NaN throughout (std_dev 0; an unordered compare keeps every event), and 37 sequences with empty ones among them"""
    _, seqs, pore, k = [c for c in rc.cases() if c[0] == name][0]
    eng.reference_from_bases(seqs, pore, k, True)
    fwd = [eng.reference_fetch(s, 1) for s in range(len(seqs))]
    rev = [eng.reference_fetch(s, 0) for s in range(len(seqs))]
    if name == "one_letter_k6":
        assert all(np.all(np.isnan(x)) for x in fwd + rev)
    want = SeedIndex.from_signals(fwd, rev, DEFAULT, threads=4)
    got = SeedIndex.from_device(eng, DEFAULT)
    assert want.n_positions > 100
    same_header(got, want, name)
    same_lists(got, want, want.keys().tolist() + [0, 1, 0xFFFFFFFF], name)


# ---- C. seeding through the big table -----------------------------------------------------------------------------------------------------
def test_seeding_through_the_big_table(eng, tables):
    """a table of 2^21 slots and more, built on the device: the hits of 64 noisy chunks equal the host's through the host's table"""
    got, want = tables("default")
    assert want.table_bytes >= (1 << 21) * 16
    fwd, rev = sc.table_genome()
    rng = np.random.default_rng(41)
    chunks = [(x[lo:lo + 250] + rng.normal(0, 0.03, 250)).astype(np.float32)
              for x in (fwd[0], rev[0]) for lo in rng.integers(0, len(x) - 250, 32).tolist()]
    ev, off = np.concatenate(chunks), np.arange(len(chunks) + 1, dtype=np.uint64) * 250
    want_off, want_hits = seeding.seed_hits_host(want, ev, off)
    eng.upload_seed_index(got)
    got_off, got_hits = eng.seed_hits(ev, off)
    assert len(want_hits) > len(chunks) and np.array_equal(got_off, want_off) and got_hits.tobytes() == want_hits.tobytes()


def test_seeding_through_the_low_entropy_table(eng, tables):
    """every probe returns a list of tens of thousands: k_seed_write's all-lanes path writes nearly every hit"""
    got, want = tables("e2_lq1")
    fwd, rev = sc.table_genome()
    rng = np.random.default_rng(42)
    chunks = [(fwd[0][lo:lo + n] + rng.normal(0, 0.03, n)).astype(np.float32) for lo, n in ((1000, 6), (200_000, 8), (399_000, 10))]
    ev = np.concatenate(chunks)
    off = np.array([0, 6, 14, 24], np.uint64)
    want_off, want_hits = seeding.seed_hits_host(want, ev, off)
    cap = int(want_off[-1])
    assert cap > 3 * 10_000 and np.all(np.diff(want_off.astype(np.int64)) > 10_000)
    eng.upload_seed_index(got)
    got_off, got_hits = eng.seed_hits(ev, off, hits_cap=cap)
    assert np.array_equal(got_off, want_off) and got_hits.tobytes() == want_hits.tobytes()


# ---- D. the .ind upload in pieces ---------------------------------------------------------------------------------------------------------
def test_ind_strand_read_from_the_file_in_pieces(tmp_path, eng, other):
    """a strand of 16 777 216 + 1 floats: two pieces a strand, the second of one float; the pieces of four strands take turns in the two
    staging buffers"""
    rng = np.random.default_rng(43)
    n = sc.INDEX_STAGE_FLOATS + 1
    fwd = [rng.standard_normal(n, np.float32), rng.standard_normal(7, np.float32)]
    rev = [rng.standard_normal(n, np.float32), rng.standard_normal(7, np.float32)]
    path = str(tmp_path / "big.ind")
    write_index(path, ["long", "short"], fwd, rev)
    ix = Index(path)
    try:
        assert ix.lens == [n, 7]
        ix.upload(eng)
        for s in range(2):
            for strand, want in ((1, fwd[s]), (0, rev[s])):
                assert eng.reference_fetch(s, strand, len(want)).tobytes() == want.tobytes(), (s, strand)
        offsets_equal(eng, other, fwd, rev)
    finally:
        ix.close()
        other.upload_reference([fwd[1]], [rev[1]])  # (the large arenas go)
        eng.upload_reference([fwd[1]], [rev[1]])


# ---- E. the tool's other branch -----------------------------------------------------------------------------------------------------------
def test_build_index_with_minimizer_windows(tmp_path):
    """scripts/build_index.py -w 5: the table is built on the host from the fetched signals and written as every other"""
    spec = importlib.util.spec_from_file_location("build_index", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "build_index.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(61)
    k, pore = 6, synth.make_pore_model(6)
    records = [("chrA", rc._bases(rng, 3000)), ("short", b"ACG"), ("chrB", rc._bases(rng, 1201).lower()), ("none", b"")]
    fa, model, out = tmp_path / "ref.fa", tmp_path / "model.txt", tmp_path / "ref.ind"
    fa.write_bytes(b"".join(b">" + n.encode() + b" x\n" + b"\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + b"\n" for n, s in records))
    model.write_text("kmer\tlevel_mean\n" + "".join("%s\t%r\n" % ("".join("ACGT"[(j >> 2 * (k - 1 - t)) & 3] for t in range(k)), float(pore[j]))
                                                      for j in range(4 ** k)))
    info = tool.build_index(str(fa), str(model), str(out), w=5)
    fwd = [refsig.seq_to_sig(s, pore, k, 1) for _, s in records]
    rev = [refsig.seq_to_sig(s, pore, k, 0) for _, s in records]
    want = SeedIndex.from_signals(fwd, rev, SeedParams(w=5))
    ix = Index(str(out))
    try:
        assert (ix.w, ix.e, ix.q, ix.lq, ix.k) == (5, 6, 9, 3, 6) and ix.lens == [len(s) for _, s in records]
        got = SeedIndex.from_index(ix)
        assert (got.n_keys, got.n_positions) == (want.n_keys, want.n_positions) == (info["keys"], info["positions"]) and want.n_keys > 500
        assert got.pars == SeedParams(w=5)
        assert np.array_equal(np.sort(got.keys()), np.sort(want.keys()))
        same_lists(got, want, want.keys().tolist(), "w5")
        plain = SeedIndex.from_signals(fwd, rev, SeedParams())
        assert want.n_positions < plain.n_positions  # (windows of 5 choose: the table is not the w = 0 one)
    finally:
        ix.close()
