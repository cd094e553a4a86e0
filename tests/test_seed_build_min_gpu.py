"""The seed table of a minimizer index (w > 0) built on the device (include/rawdtw.h: rawdtw_seed_index_build_device_min --
rawdtw_seed_build.hip: k_sb_filter without the mask test, k_sb_hash, k_sb_min_count, rocPRIM's scan, k_sb_min_write) against
rawdtw_seed_index_build from the same arrays: the header's numbers, the keys as whole arrays in their order, every key's list.  Then the
reference's own recorded hits through a table the device built, the tool and a mapping run.  Exact equality of integers everywhere;
inputs: tests/seed_build_min_cases.py.  Nothing here reads the reference itself."""
import importlib.util
import os

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapper, refsig, synth
from rawalign_amd._lib import RawDTWError
from rawalign_amd.index import Index
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex, SeedParams
from tests import refsig_cases as rc
from tests import refsig_scale_cases as scale
from tests import seed_build_min_cases as bc
from tests import seed_cases as sc
from tests import seed_min_cases as smc
from tests.test_refsig_scale_gpu import same_header, same_lists, sampled

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    e = ra.Engine(0)
    yield e
    e.close()


def same_table(eng, fwd, rev, p, what, threads=4):
    """the device's table of the uploaded arrays against the host's: header, keys, key order, every list; returns the host's"""
    eng.upload_reference(fwd, rev)
    want = SeedIndex.from_signals(fwd, rev, p, threads=threads)
    got = SeedIndex.from_device(eng, p, minimizer=True)
    same_header(got, want, what)
    same_lists(got, want, want.keys().tolist() + [0, 1, 0xFFFFFFFF, 12345], what)
    st = eng.seed_build_min_stats()
    assert st["entries"] == want.n_positions, what
    got.close()
    return want


# ---- the tie alphabets as whole strands ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [2, 6, 9])
@pytest.mark.parametrize("w", bc.DEVICE_W)
def test_alphabet_strands_equal_the_host_table(eng, w, e):
    positions = 0
    for a in bc.ALPHABETS:
        fwd, rev = bc.alphabet_reference(a)
        want = same_table(eng, fwd, rev, SeedParams(w=w, e=e), ("alphabet", a, w, e))
        positions += want.n_positions
        emers = eng.seed_build_min_stats()["emers"]
        assert emers >= want.n_positions > 0   # (no strand emits an e-mer twice: tests/test_seed_build_min_cpu.py)
    assert positions > (150 if w > 5 else 1500)


# ---- the window's and the tile's edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [2, 5, 64, 255])
def test_window_and_tile_edges_equal_the_host_table(eng, w):
    e = 6
    fwd, rev, Ms = bc.edge_reference(w, e)
    assert set(Ms) >= {0, 1, w - 1, w, w + 1, bc.TILE - 1, bc.TILE, bc.TILE + 1, 2 * bc.TILE + 1}
    assert len(fwd[1]) == 0 and len(fwd[0]) > 2 * bc.TILE and len(fwd[2]) > bc.TILE   # an empty sequence between two long ones
    assert sum(0 < len(x) < e for x in fwd) >= 2                                      # strands with fewer kept events than e
    for x in fwd + rev:
        assert len(bc.kept_events(x)) == len(x)
    same_table(eng, fwd, rev, SeedParams(w=w, e=e), ("edges", w))
    assert eng.seed_build_min_stats()["emers"] == 2 * sum(Ms)


@pytest.mark.parametrize("w", bc.BOUNDARY_W)
def test_minimum_leaves_the_window_at_a_tiles_first_emer(eng, w):
    """rule 3 at e-mer TILE with the new minimum's equal hashes on both sides of the tile boundary: the thread that emits them reads
    staged hashes of the tile before its own (the input's property is asserted here and in tests/test_seed_build_min_cpu.py)"""
    x = bc.boundary_strand(w)
    p = SeedParams(w=w, e=2)
    h, first = bc.emer_hashes(x, p)
    assert np.array_equal(first, np.arange(len(h))) and bc.leaves_at(h, bc.TILE, w)
    ties = [i for i, r in bc.step_rules(h, bc.TILE, len(h), w) if r == 30]
    assert ties and min(ties) < bc.TILE
    other = bc.all_kept(len(x), np.random.default_rng(5))
    same_table(eng, [x, other], [other, x], p, ("boundary", w))   # (the strand as a forward and as a reverse array)


# ---- values -------------------------------------------------------------------------------------------------------------------------------
def value_sets():
    rng = np.random.default_rng(31)
    pore = synth.make_pore_model(6)

    def strands(n):
        s = rc._bases(rng, n + 5)
        return refsig.seq_to_sig(s, pore, 6, 1).copy(), refsig.seq_to_sig(s, pore, 6, 0).copy()
    f, r = strands(3000)
    f[200:420] = f[199]          # homopolymer stretches: runs of skipped events far longer than a step of 64
    r[1000:1070] = r[999] + np.float32(0.2)
    f[2000:2065] = f[1999]
    out = [("homopolymer", [f], [r])]
    f, r = strands(1200)
    M = bc.MASK_SIGNAL
    f[0], f[1], f[300:303], f[1199], r[64], r[127:129] = M, M, M, M, M, M
    out.append(("masked", [f], [r]))
    out.append(("one_short", [f[:3]], [r[:3]]))
    return out


@pytest.mark.parametrize("w", [1, 5, 10])
def test_values_under_the_minimizer_rule(eng, w):
    """homopolymer runs, and RI_MASK_SIGNAL -- kept and coded when w > 0 (rsketch.c:172): the table is not the one of the w = 0 filter"""
    for name, fwd, rev in value_sets():
        p = SeedParams(w=w)
        want = same_table(eng, fwd, rev, p, (name, w))
        if name == "masked" and w == 1:   # w = 1 keeps every e-mer: the masks' e-mers are in the table, those across them are not
            plain = SeedIndex.from_signals(fwd, rev, SeedParams())
            assert want.n_positions > plain.n_positions


def test_nan_strands_from_bases(eng):
    """a one-letter sequence: NaN throughout (std_dev 0); an unordered compare keeps every event, every e-mer has one hash"""
    _, seqs, pore, k = [c for c in rc.cases() if c[0] == "one_letter_k6"][0]
    eng.reference_from_bases(seqs, pore, k, True)
    fwd = [eng.reference_fetch(s, 1) for s in range(len(seqs))]
    rev = [eng.reference_fetch(s, 0) for s in range(len(seqs))]
    assert all(np.all(np.isnan(x)) for x in fwd + rev)
    for w in (5, 255):
        p = SeedParams(w=w)
        want = SeedIndex.from_signals(fwd, rev, p)
        got = SeedIndex.from_device(eng, p, minimizer=True)
        assert want.n_positions > 10
        same_header(got, want, ("nan", w))
        same_lists(got, want, want.keys().tolist() + [0, 1, 0xFFFFFFFF], ("nan", w))


# ---- past the grid-stride threshold ------------------------------------------------------------------------------------------------------
def test_more_than_1024_tiles_in_a_strand(eng):
    fwd, rev = scale.table_genome_cut()
    p = SeedParams(w=5)
    eng.upload_reference(fwd, rev)
    want = SeedIndex.from_signals(fwd, rev, p, threads=16)
    got = SeedIndex.from_device(eng, p, minimizer=True)
    st = eng.seed_build_min_stats()
    print("w = 5, two sequences:", st, eng.seed_build_stats())
    long_strands = [len(bc.kept_events(x)) - p.e + 1 for x in (fwd[0], rev[0])]
    assert min(long_strands) > bc.GRID_Y * bc.TILE   # more than 1024 tiles in a strand: a workgroup takes a second tile
    assert st["emers"] == sum(max(len(bc.kept_events(x)) - p.e + 1, 0) for x in (fwd[1], rev[1])) + sum(long_strands)
    assert st["entries"] == want.n_positions < st["emers"]
    assert abs(eng.seed_build_stats()["emit_ms"] - (st["hash_ms"] + st["count_scan_ms"] + st["write_ms"])) < 1e-3
    same_header(got, want, "cut w5")
    pick = sampled(want, 20_000, 6)
    same_lists(got, want, pick, "cut w5")
    scale.release()


# ---- the reference's recorded hits through a table the device built ---------------------------------------------------------------------
@pytest.mark.parametrize("name", smc.CASES)
def test_fixture_hits_through_a_device_built_table(name):
    fx = smc.Fixture()
    fwd, rev, p, chunks = smc.build_case(name)
    assert p.w > 0 and sc.case_sha256(fwd, rev, chunks) == fx.sha(name)
    e = ra.Engine(0)
    try:
        e.upload_reference(fwd, rev)
        si = SeedIndex.from_device(e, p, minimizer=True)
        e.set_option("seed_minimizer", 1)
        e.upload_seed_index(si)
        ev, off = sc.flat(chunks)
        hoff, hits = e.seed_hits(ev, off)
        assert np.array_equal(hoff, fx.hit_off(name)) and fx.check_rows(name, sc.hit_rows(hits)), name
        assert len(hits) > 0
    finally:
        e.close()


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------
def test_build_index_w5_builds_the_table_on_the_device(tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("build_index", os.path.join(ROOT, "scripts", "build_index.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(61)
    k, pore = 6, synth.make_pore_model(6)
    records = [("chrA", rc._bases(rng, 3000)), ("short", b"ACG"), ("chrB", rc._bases(rng, 1201).lower()), ("none", b"")]
    fa, model, out = tmp_path / "ref.fa", tmp_path / "model.txt", tmp_path / "ref.ind"
    fa.write_bytes(b"".join(b">" + n.encode() + b" x\n" + b"\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + b"\n" for n, s in records))
    model.write_text("kmer\tlevel_mean\n" + "".join("%s\t%r\n" % ("".join("ACGT"[(j >> 2 * (k - 1 - t)) & 3] for t in range(k)), float(pore[j]))
                                                      for j in range(4 ** k)))

    def no_host_build(*a, **kw):
        raise AssertionError("the tool built the table on the host")
    monkeypatch.setattr(tool.SeedIndex, "from_signals", no_host_build)
    info = tool.build_index(str(fa), str(model), str(out), w=5)
    monkeypatch.undo()
    fwd = [refsig.seq_to_sig(s, pore, k, 1) for _, s in records]
    rev = [refsig.seq_to_sig(s, pore, k, 0) for _, s in records]
    want = SeedIndex.from_signals(fwd, rev, SeedParams(w=5))
    ix = Index(str(out))
    try:
        assert ix.w == 5 and (ix.e, ix.q, ix.lq, ix.k) == (6, 9, 3, 6)
        got = SeedIndex.from_index(ix)
        assert (got.n_keys, got.n_positions) == (want.n_keys, want.n_positions) == (info["keys"], info["positions"]) and want.n_keys > 500
        assert got.pars == SeedParams(w=5) and np.array_equal(np.sort(got.keys()), np.sort(want.keys()))
        same_lists(got, want, want.keys().tolist(), "tool w5")
    finally:
        ix.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_paf_lines_through_a_device_built_minimizer_table():
    bp, n = 20_000, 64
    g = synth.make_genome(bp, 515)
    bases = np.frombuffer(b"ACGT", np.uint8)[g].tobytes()
    pore = synth.make_pore_model(6)
    rng = np.random.default_rng(516)
    pa = synth.make_genome_raw_reads(g, rng.integers(0, bp - 1500, n), [1300] * n, rng.integers(0, 2, n), seed=517)
    fwd, rev = refsig.seq_to_sig(bases, pore, 6, 1), refsig.seq_to_sig(bases, pore, 6, 0)
    names, lens = ["genome"], [len(fwd)]
    reads = mapper.SignalReads(pa, lens)
    p = SeedParams(w=5)
    a, b = ra.Engine(0), ra.Engine(0)
    try:
        for e in (a, b):
            e.set_option("seed_minimizer", 1)
        a.reference_from_bases([bases], pore, 6)
        six_a = SeedIndex.from_device(a, p, minimizer=True)
        b.upload_reference([fwd], [rev])
        six_b = SeedIndex.from_signals([fwd], [rev], p)
        assert six_a.n_positions == six_b.n_positions > 1000
        lines = []
        for e, six in ((a, six_a), (b, six_b)):
            cm = mapper.CMapper(e, ra.MapOpt(), StopOpt(), names, lens, slot_events=4096, max_reads=n, threads=3, carry=False, device_chain=True)
            got, rounds = mapper.map_reads_c(reads, list(range(n)), cm, seed_index=six, signal=True)
            cm.close()
            lines.append(got)
        assert lines[0] == lines[1]
        assert sum("\t*\t" not in ln for ln in lines[0]) > n // 2
    finally:
        a.close()
        b.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(eng):
    fwd, rev = bc.alphabet_reference(4)
    eng.upload_reference(fwd, rev)
    before = eng.reference_fetch(4, 1, len(fwd[4]))
    for bad in (SeedParams(w=256), SeedParams(w=5, e=1)):
        with pytest.raises(RawDTWError) as err:
            SeedIndex.from_device(eng, bad, minimizer=True)
        assert err.value.status == INVALID
    fresh = ra.Engine(0)
    try:
        with pytest.raises(RawDTWError) as err:
            SeedIndex.from_device(fresh, SeedParams(w=5), minimizer=True)   # no reference on the context
        assert err.value.status == INVALID
    finally:
        fresh.close()
    assert eng.reference_fetch(4, 1, len(fwd[4])).tobytes() == before.tobytes() == fwd[4].tobytes()
    same_table(eng, fwd, rev, SeedParams(w=5), "after the refusals")
    with pytest.raises(RawDTWError) as err:
        SeedIndex.from_device(eng, SeedParams(w=5))   # without the keyword: rawdtw_seed_index_build_device, as before
    assert err.value.status == UNSUPPORTED
    # w = 0 through the new entry is the existing path
    want = SeedIndex.from_signals(fwd, rev, SeedParams())
    got = SeedIndex.from_device(eng, SeedParams(), minimizer=True)
    same_header(got, want, "w0")
    same_lists(got, want, want.keys().tolist(), "w0")
