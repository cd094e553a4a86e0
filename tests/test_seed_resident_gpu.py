"""The seed index built and kept on the device (include/rawdtw.h: rawdtw_seed_index_build_resident, rawdtw_seed_table_from_entries,
rawdtw_seed_index_fetch -- rawdtw_seed_build.hip: k_sb_next, k_sb_chain, k_sb_mark, k_tb_insert, k_tb_slots) against
rawdtw_seed_index_build / rawdtw_seed_index_from_entries from the same arrays: the header's numbers, the keys as whole arrays in table
order (the slots' layout), every key's list -- the resident index fetched first.  Then the table used without a fetch, what a device-only
index refuses, and the tool.  Exact equality of integers everywhere; inputs: tests/seed_resident_cases.py.  Nothing here reads the
reference itself."""
import importlib.util
import os

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapper, seeding, synth
from rawalign_amd._lib import RawDTWError
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex, SeedParams
from tests import map_ref_cases as mc
from tests import refsig_cases as rfc
from tests import refsig_scale_cases as scale
from tests import seed_build_min_cases as bc
from tests import seed_cases as sc
from tests import seed_min_cases as smc
from tests import seed_resident_cases as rc
from tests.test_refsig_scale_gpu import same_header, same_lists, sampled

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABSENT = [0, 1, 0xFFFFFFFF, 12345]


@pytest.fixture(scope="module")
def eng():
    e = ra.Engine(0)
    e.set_option("seed_minimizer", 1)
    yield e
    e.close()


def same_table(eng, fwd, rev, p, what, threads=4, pick=None, count=True):
    """the resident table of the uploaded arrays, fetched, against the host's: header, keys in table order, lists; the build's kept events
    and entries against the cases module's restatement.  Returns (host table, statistics)."""
    eng.upload_reference(fwd, rev)
    want = SeedIndex.from_signals(fwd, rev, p, threads=threads)
    got = SeedIndex.from_device(eng, p, resident=True)
    st = eng.seed_build_resident_stats()
    assert got.resident and (got.n_seq, got.n_keys, got.n_positions, got.table_bytes) == (want.n_seq, want.n_keys, want.n_positions, want.table_bytes), what
    got.fetch(eng)
    assert not got.resident
    same_header(got, want, what)
    same_lists(got, want, (want.keys().tolist() if pick is None else pick) + ABSENT, what)
    assert st["tile"] == rc.TILE and st["tiles"] == 2 * sum((len(x) + rc.TILE - 1) // rc.TILE for x in fwd), what
    assert st["entries"] == want.n_positions and st["keys"] == want.n_keys and st["log2_slots"] == rc.log2_slots(want.n_keys), what
    if want.n_keys < 100_000:   # the keys not in their home slot, and the table order once more, from insertion written again in Python
        order, displaced = rc.sequential_layout(want.keys())
        assert want.keys().tolist() == order and st["displaced"] == displaced, what
    if count:
        kept, entries = rc.kept_and_entries(fwd, rev, p)
        assert st["kept"] == kept and entries in (None, st["entries"]), what
    got.close()
    return want, st


# ---- the filter ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0, 5])
def test_strands_at_the_tiles_edges_equal_the_host_table(eng, w):
    """the CPU program's strand shapes at the real tile size, each as a forward and as a reverse array, an empty sequence between two
    long ones among them"""
    fwd, rev, names = rc.shape_reference()
    at = names.index("all_kept_0")
    assert len(fwd[at]) == 0 and len(fwd[at - 1]) > rc.TILE and len(fwd[at + 2]) > 2 * rc.TILE
    want, st = same_table(eng, fwd, rev, SeedParams(w=w, e=3), ("shapes", w))
    assert want.n_positions > 50_000


@pytest.mark.parametrize("w", [0, 5])
def test_short_strands_and_an_empty_sequence_equal_the_host_table(eng, w):
    """tests/seed_build_min_cases.py's edge reference: strands with fewer kept events than e, one-event strands, an empty sequence"""
    fwd, rev, Ms = bc.edge_reference(max(w, 2), 6)
    assert len(fwd[1]) == 0 and sum(0 < len(x) < 6 for x in fwd) >= 2
    same_table(eng, fwd, rev, SeedParams(w=w, e=6), ("edges", w))


@pytest.mark.parametrize("w", [0, 5])
def test_a_strand_of_more_tiles_than_the_grid(eng, w):
    """more than 1 024 tiles in a strand, all kept and flat by turns: a workgroup of k_sb_next and k_sb_mark takes a second tile, and the
    chain steps over tiles that keep one event and tiles that keep every one"""
    fwd, rev = rc.long_strand_reference()
    tiles = (len(fwd[0]) + rc.TILE - 1) // rc.TILE
    assert tiles > rc.GRID_Y and tiles > 1024
    p = SeedParams(w=w)
    eng.upload_reference(fwd, rev)
    want = SeedIndex.from_signals(fwd, rev, p, threads=16)
    got = SeedIndex.from_device(eng, p, resident=True).fetch(eng)
    st = eng.seed_build_resident_stats()
    print("w = %d:" % w, st)
    kept = sum(len(rc.kept_events(x, w == 0)) for x in (fwd[0], rev[0]))
    assert st["kept"] == kept and st["tiles"] == 2 * tiles and st["entries"] == want.n_positions
    assert kept > len(fwd[0]) and (w or st["entries"] == kept - 2 * (p.e - 1))
    same_header(got, want, ("long", w))
    same_lists(got, want, sampled(want, 5_000, 7), ("long", w))


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
def same_table_from_entries(eng, hs, ys, what, pick=None):
    want = SeedIndex.from_entries(SeedParams(), 3, hs, ys)
    got = SeedIndex.from_entries(SeedParams(), 3, hs, ys, engine=eng)
    st = eng.seed_build_resident_stats()
    assert got.resident
    got.fetch(eng)
    same_header(got, want, what)
    same_lists(got, want, (np.unique(hs).tolist() if pick is None else pick) + ABSENT, what)
    keys = want.keys()
    assert st["keys"] == want.n_keys == len(np.unique(hs)) and st["entries"] == len(hs) and st["tiles"] == 0
    return want, st, keys


@pytest.mark.parametrize("case", rc.table_cases(), ids=lambda c: c[0])
def test_crafted_tables_equal_fill_table(eng, case):
    name, hs, ys = case
    want, st, keys = same_table_from_entries(eng, hs, ys, name)
    lg = rc.log2_slots(want.n_keys)
    assert want.table_bytes >= 16 * 16 and st["log2_slots"] == lg
    order, displaced = rc.sequential_layout(hs)   # (insertion in ascending hash order, written again in Python)
    assert keys.tolist() == order and st["displaced"] == displaced
    if name in ("one_home", "wraps"):
        assert displaced > 20


def test_a_big_table_with_many_collisions_between_waves(eng):
    hs, ys = rc.big_table()
    assert len(np.unique(hs)) == 1_200_000
    want, st, keys = same_table_from_entries(eng, hs, ys, "big", pick=np.random.default_rng(3).choice(hs, 20_000).tolist())
    print("1.2 M keys:", st)
    order, displaced = rc.sequential_layout(hs)
    assert st["log2_slots"] == 22 and st["displaced"] == displaced > 100_000   # (load 0.29: about one key in seven meets a taken slot)
    assert np.array_equal(keys, np.array(order, np.uint32))


# ---- existing inputs through the resident build ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [2, 6, 9])
@pytest.mark.parametrize("w", [0, 5])
def test_alphabet_strands_equal_the_host_table(eng, w, e):
    for a in bc.ALPHABETS:
        fwd, rev = bc.alphabet_reference(a)
        want, st = same_table(eng, fwd, rev, SeedParams(w=w, e=e), ("alphabet", a, w, e))
        assert want.n_positions > 0


@pytest.mark.parametrize("name", ["default", "e2_lq1"])
def test_the_scale_genome_equals_the_host_table(eng, name):
    """more than 2^20 entries; with e = 2, lq = 1 a table of 36 keys whose longest list has 94 377 positions"""
    p = {"default": SeedParams(), "e2_lq1": SeedParams(e=2, lq=1)}[name]
    fwd, rev = scale.table_genome()
    eng.upload_reference(fwd, rev)
    want = SeedIndex.from_signals(fwd, rev, p, threads=16)
    got = SeedIndex.from_device(eng, p, resident=True).fetch(eng)
    st = eng.seed_build_resident_stats()
    print(name, st)
    assert want.n_positions > scale.MERGE_SORT_LIMIT and st["entries"] == want.n_positions and st["keys"] == want.n_keys
    same_header(got, want, name)
    if name == "e2_lq1":
        keys = want.keys().tolist()
        same_lists(got, want, keys + ABSENT, name)
        assert max(len(want.get(h)) for h in keys) == 94_377
    else:
        same_lists(got, want, sampled(want, 20_000, 5), name)
        assert (st["kept"], st["entries"]) == rc.kept_and_entries(fwd, rev, p)
    scale.release()


def test_nan_strands_from_bases(eng):
    _, seqs, pore, k = [c for c in rfc.cases() if c[0] == "one_letter_k6"][0]
    eng.reference_from_bases(seqs, pore, k, True)
    fwd = [eng.reference_fetch(s, 1) for s in range(len(seqs))]
    rev = [eng.reference_fetch(s, 0) for s in range(len(seqs))]
    assert all(np.all(np.isnan(x)) for x in fwd + rev)
    for w in (0, 5):
        p = SeedParams(w=w)
        want = SeedIndex.from_signals(fwd, rev, p)
        got = SeedIndex.from_device(eng, p, resident=True).fetch(eng)
        assert want.n_positions > 10 and eng.seed_build_resident_stats()["kept"] == 2 * sum(len(x) for x in fwd)
        same_header(got, want, ("nan", w))
        same_lists(got, want, want.keys().tolist() + ABSENT, ("nan", w))


# ---- use without a fetch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.DEVICE_CASES + smc.CASES)
def test_fixture_hits_through_a_table_that_never_left_the_device(eng, name):
    """the reference's own recorded hits (tests/golden/seed_ref.npz, seed_min_ref.npz) seeded from a resident table"""
    cases, fx = (smc, smc.Fixture()) if name in smc.CASES else (sc, sc.Fixture())
    fwd, rev, p, chunks = cases.build_case(name)
    assert sc.case_sha256(fwd, rev, chunks) == fx.sha(name)
    eng.upload_reference(fwd, rev)
    si = SeedIndex.from_device(eng, p, resident=True)
    eng.upload_seed_index(si)   # (the same serial: nothing is sent)
    ev, off = sc.flat(chunks)
    hoff, hits = eng.seed_hits(ev, off)
    assert si.resident and np.array_equal(hoff, fx.hit_off(name)) and len(hits) == int(hoff[-1])
    if cases is smc:
        assert fx.check_rows(name, sc.hit_rows(hits)), name
    else:
        assert np.array_equal(sc.hit_rows(hits), fx.hits(name)), name


@pytest.mark.parametrize("resident", [False, True], ids=["plain", "resident_rounds"])
def test_paf_lines_through_a_resident_table(resident):
    """map_reads_c with the library seeding every round: a resident index on its own context against the host-built index on another"""
    ref = mc.make_reference()
    form, name = mc.FORMS[0], list(mc.WHOLE_SETS)[0]
    wr = mc.WholeReads(form, ref=ref)
    opt, copt = mc.whole_project_opts(name, form)
    lines = []
    for built_resident in (True, False):
        e = ra.Engine(0)
        try:
            e.upload_reference(ref.forward, ref.reverse)
            six = SeedIndex.from_device(e, SeedParams(), resident=True) if built_resident else SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)
            cm = mapper.CMapper(e, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096,
                                max_reads=wr.n_reads, chain_opt=copt, output_chains=True, threads=3, carry=False, groups=1, device_chain=True)
            got, rounds = mapper.map_reads_c(wr, list(range(wr.n_reads)), cm, seed_index=six, resident=resident)
            cm.close()
            assert six.resident == built_resident
            lines.append(got)
        finally:
            e.close()
    assert lines[0] == lines[1] and sum("\t*\t" not in ln for ln in lines[0]) > 0


# ---- refusals and state -------------------------------------------------------------------------------------------------------------------
def refused(status, fn, *a, **kw):
    with pytest.raises(RawDTWError) as err:
        fn(*a, **kw)
    assert err.value.status == status, err.value
    return str(err.value)


def test_a_device_only_index_refuses_what_needs_the_host_copy(eng):
    fwd, rev, p, chunks = sc.build_case("e6")
    ev, off = sc.flat(chunks)
    eng.upload_reference(fwd, rev)
    want = SeedIndex.from_signals(fwd, rev, p)
    si = SeedIndex.from_device(eng, p, resident=True)
    key = int(want.keys()[0])
    refused(UNSUPPORTED, si.get, key)
    refused(UNSUPPORTED, si.keys)
    refused(UNSUPPORTED, seeding.seed_hits_host, si, ev, off)
    other = ra.Engine(0)
    try:
        assert "rawdtw_seed_index_fetch" in refused(UNSUPPORTED, other.upload_seed_index, si)
        refused(INVALID, si.fetch, other)   # (the table is not on that context)
        want_off, want_hits = seeding.seed_hits_host(want, ev, off)
        got_off, got_hits = eng.seed_hits(ev, off)
        assert np.array_equal(got_off, want_off) and got_hits.tobytes() == want_hits.tobytes() and len(want_hits) > 0
        si.fetch(eng)
        si.fetch(eng)   # (an index with its host copy: nothing to do)
        assert not si.resident and np.array_equal(si.get(key), want.get(key)) and np.array_equal(si.keys(), want.keys())
        host_off, host_hits = seeding.seed_hits_host(si, ev, off)
        assert np.array_equal(host_off, want_off) and host_hits.tobytes() == want_hits.tobytes()
        other.upload_seed_index(si)
        got_off, got_hits = other.seed_hits(ev, off)
        assert np.array_equal(got_off, want_off) and got_hits.tobytes() == want_hits.tobytes()
        eng.upload_seed_index(si)   # (still the context's table, under the same serial)
        got_off, got_hits = eng.seed_hits(ev, off)
        assert got_hits.tobytes() == want_hits.tobytes()
    finally:
        other.close()


def test_a_failed_build_leaves_the_table_and_a_replaced_table_cannot_be_fetched(eng):
    fwd, rev, p, chunks = sc.build_case("e6")
    ev, off = sc.flat(chunks)
    eng.upload_reference(fwd, rev)
    si = SeedIndex.from_device(eng, p, resident=True)
    want_off, want_hits = eng.seed_hits(ev, off)
    assert len(want_hits) > 0
    for bad in (SeedParams(w=256), SeedParams(e=1)):
        refused(INVALID, SeedIndex.from_device, eng, bad, resident=True)
    refused(INVALID, SeedIndex.from_entries, SeedParams(), 1, [7, 5], [1, 2], engine=eng)   # (unsorted: refused on the host)
    fresh = ra.Engine(0)
    try:
        refused(INVALID, SeedIndex.from_device, fresh, p, resident=True)   # no reference on the context
    finally:
        fresh.close()
    got_off, got_hits = eng.seed_hits(ev, off)
    assert np.array_equal(got_off, want_off) and got_hits.tobytes() == want_hits.tobytes()
    # another index takes the context's table: the resident one is gone for good
    small = SeedIndex.from_entries(SeedParams(), 1, [5, 5, 7], [8, 9, 1])
    eng.upload_seed_index(small)
    refused(INVALID, si.fetch, eng)
    refused(INVALID, eng.upload_seed_index, si)
    assert si.resident
    si.close()   # (the handle alone)
    again = SeedIndex.from_device(eng, p, resident=True)   # and the context builds the next one as before
    got_off, got_hits = eng.seed_hits(ev, off)
    assert np.array_equal(got_off, want_off) and got_hits.tobytes() == want_hits.tobytes()
    again.close()


def test_the_mappers_host_seeding_refuses_a_device_only_index():
    """a minimizer index on a context whose "seed_minimizer" is off is seeded on the host: that needs the host copy"""
    ref = mc.make_reference()
    form, name = mc.FORMS[0], list(mc.WHOLE_SETS)[0]
    wr = mc.WholeReads(form, ref=ref)
    opt, copt = mc.whole_project_opts(name, form)
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        six = SeedIndex.from_device(e, SeedParams(w=5), resident=True)
        want = SeedIndex.from_signals(ref.forward, ref.reverse, SeedParams(w=5), threads=4)
        lines = []
        for index in (six, six, want):
            cm = mapper.CMapper(e, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096,
                                max_reads=wr.n_reads, chain_opt=copt, output_chains=True, threads=3, carry=False)
            try:
                if index.resident:
                    with pytest.raises(RuntimeError, match="status %d.*rawdtw_seed_index_fetch" % UNSUPPORTED):
                        mapper.map_reads_c(wr, list(range(wr.n_reads)), cm, seed_index=index)
                    index.fetch(e)
                else:
                    lines.append(mapper.map_reads_c(wr, list(range(wr.n_reads)), cm, seed_index=index)[0])
            finally:
                cm.close()
        assert len(lines) == 2 and lines[0] == lines[1]
    finally:
        e.close()


def test_a_begun_seeding_refuses_the_builds(eng):
    """as rawdtw_seed_index_upload: between rawdtw_seed_begin and _end the context's table is in use"""
    import ctypes as C

    fwd, rev, p, chunks = sc.build_case("e6")
    ev, off = sc.flat(chunks)
    eng.upload_reference(fwd, rev)
    si = SeedIndex.from_device(eng, p, resident=True)
    want_off, want_hits = eng.seed_hits(ev, off)
    hoff, hits = np.zeros(len(off), np.uint64), np.zeros(len(want_hits), seeding.HIT_DTYPE)
    eng._check(eng.lib.rawdtw_seed_begin(eng._ctx, len(off) - 1, off.ctypes.data, ev.ctypes.data, hoff.ctypes.data, hits.ctypes.data, len(hits)))
    try:
        refused(INVALID, SeedIndex.from_device, eng, p, resident=True)
        refused(INVALID, SeedIndex.from_entries, SeedParams(), 1, [5, 7], [1, 2], engine=eng)
    finally:
        eng._check(eng.lib.rawdtw_seed_end(eng._ctx, C.byref(C.c_float())))
    assert np.array_equal(hoff, want_off) and hits.tobytes() == want_hits.tobytes() and si.resident   # (the seeding ran on the table that stayed)
    si.close()


# ---- the tool -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0, 5])
def test_build_index_resident_writes_the_same_file(tmp_path, w):
    spec = importlib.util.spec_from_file_location("build_index", os.path.join(ROOT, "scripts", "build_index.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(61)
    k, pore = 6, synth.make_pore_model(6)
    records = [("chrA", rfc._bases(rng, 3000)), ("short", b"ACG"), ("chrB", rfc._bases(rng, 1201).lower()), ("none", b"")]
    fa, model = tmp_path / "ref.fa", tmp_path / "model.txt"
    fa.write_bytes(b"".join(b">" + n.encode() + b" x\n" + b"\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + b"\n" for n, s in records))
    model.write_text("kmer\tlevel_mean\n" + "".join("%s\t%r\n" % ("".join("ACGT"[(j >> 2 * (k - 1 - t)) & 3] for t in range(k)), float(pore[j]))
                                                      for j in range(4 ** k)))
    a = tool.build_index(str(fa), str(model), str(tmp_path / "a.ind"), w=w)
    b = tool.build_index(str(fa), str(model), str(tmp_path / "b.ind"), w=w, resident=True)
    assert a == b and a["keys"] > 500
    assert (tmp_path / "a.ind").read_bytes() == (tmp_path / "b.ind").read_bytes()
