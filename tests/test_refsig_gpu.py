"""The reference from bases on the device (include/rawdtw.h: rawdtw_reference_from_bases, rawdtw_reference_fetch,
rawdtw_reference_build_stats -- rawdtw_refsig.hip) against the host restatement bit for bit, and the seed table built from the arena
(rawdtw_seed_index_build_device, rawdtw_seed_build.hip) against rawdtw_seed_index_build key for key and position for position.
Exact equality everywhere; a NaN equals a NaN.  Nothing here reads the reference itself."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapper, refsig, seeding, synth
from rawalign_amd._lib import RawDTWError
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex, SeedParams
from tests import refsig_cases as rc
from tests.seed_cases import MASK_SIGNAL

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def eng():
    e = ra.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def host():
    """the host restatement of every case, computed once: {(name, contracted): [strand 1, strand 0 of sequence 0, ...]}"""
    return {(name, c): [refsig.seq_to_sig(s, pore, k, strand, c) for s in seqs for strand in (1, 0)]
            for name, seqs, pore, k in rc.cases() for c in (False, True)}


# ---- A. the arena from bases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contracted", [False, True])
@pytest.mark.parametrize("case", rc.cases(), ids=[c[0] for c in rc.cases()])
def test_device_equals_host(eng, host, case, contracted):
    """Every strand of every case, both forms.  The steps: a strand's first step is slow by definition (the sum is still 0) and early
    binades tie or are left, so "slow steps only on the negative model's sum" is held as: with every level at or below 0 all of the sum's
    steps are slow and none fast, while the squares' sum still walks fast; the long case walks fast on both sums, in exactly the steps
    the host's walk of the same code takes."""
    name, seqs, pore, k = case
    eng.reference_from_bases(seqs, pore, k, contracted)
    want = host[(name, contracted)]
    for s in range(len(seqs)):
        for slot, strand in enumerate((1, 0)):
            got = eng.reference_fetch(s, strand)
            assert rc.same(got, want[2 * s + slot]), (name, s, strand)
    st = eng.reference_build_stats()
    steps = sum((max(len(s) - k + 1, 0) + 63) // 64 for s in seqs) * 2
    assert int(st["fast_steps"][0] + st["slow_steps"][0]) == int(st["fast_steps"][1] + st["slow_steps"][1]) == steps
    if name == rc.LONG:
        # what the host's own walk of the same step gives (tests/test_refsig_host.py holds that to 9 in 10 behind element 131 072)
        v = [refsig.seq_sums(rc.levels(seqs[0], pore, k, strand)) for strand in (1, 0)]
        assert st["fast_steps"].tolist() == (v[0][2] + v[1][2]).tolist() and st["slow_steps"].tolist() == (v[0][3] + v[1][3]).tolist()
        assert st["fast_steps"][0] > 0 and st["fast_steps"][1] > 0
    if name == rc.NEG:
        assert st["fast_steps"][0] == 0 and st["slow_steps"][0] == steps  # every level <= 0: the sum never leaves the slow path
        assert st["fast_steps"][1] > 0                                      # (the squares' sum does)


def _case(name):
    return [c for c in rc.cases() if c[0] == name][0]


def test_offsets_costs_and_sharing_equal_an_uploaded_reference(host):
    """the arena is laid out, answers rawdtw_reference_offset, scores and is shared as one that rawdtw_upload_reference made"""
    name, seqs, pore, k = _case("mixed37_k6")
    arrays = host[(name, True)]
    a, b, c = ra.Engine(0), ra.Engine(0), ra.Engine(0)
    try:
        a.reference_from_bases(seqs, pore, k, True)
        b.upload_reference(arrays[0::2], arrays[1::2])
        for s in range(len(seqs)):
            for strand in (0, 1):
                assert a.reference_offset(s, strand) == b.reference_offset(s, strand), (s, strand)
        rng = np.random.default_rng(9)
        events = rng.normal(size=3000).astype(np.float32)
        jobs = np.zeros(48, ra.JOB_DTYPE)
        long_enough = [s for s in range(len(seqs)) if len(arrays[2 * s]) >= 80]
        for j in range(len(jobs)):
            s, strand = long_enough[j % len(long_enough)], j & 1
            L = len(arrays[2 * s])
            n, m = int(rng.integers(2, 60)), int(rng.integers(2, 80))
            jobs[j]["n"], jobs[j]["m"] = n, m
            jobs[j]["read_off"] = rng.integers(0, len(events) - n)
            jobs[j]["ref_off"] = a.reference_offset(s, strand) + int(rng.integers(0, L - m + 1))
            jobs[j]["band_radius"] = -1 if j % 5 == 0 else max(1, n // 10)
            jobs[j]["exclude_last"] = j & 1
        want = b.score_batch(jobs, events)
        got = a.score_batch(jobs, events)
        assert got.tobytes() == want.tobytes() and np.all(np.isfinite(want))
        c._check(c.lib.rawdtw_share_reference(c._ctx, a._ctx))
        a.close()  # the owner goes: the sharer's hold keeps the arena
        assert c.score_batch(jobs, events).tobytes() == want.tobytes()
        assert rc.same(c.reference_fetch(1, 1, len(arrays[2])), arrays[2])
    finally:
        for e in (a, b, c):
            e.close()


def test_a_failed_call_leaves_the_reference(host):
    name, seqs, pore, k = _case("mixed37_k6")
    e = ra.Engine(0)
    try:
        e.reference_from_bases(seqs, pore, k, False)
        for bad_k in (13, 0):
            with pytest.raises(RawDTWError) as err:
                e.reference_from_bases(seqs, np.zeros(4, np.float32), bad_k)
            assert err.value.status == INVALID
        n = C.c_uint64(1 << 31)
        p = (C.c_void_p * 1)(0)
        assert e.lib.rawdtw_reference_from_bases(e._ctx, 1, p, C.byref(n), pore.ctypes.data, k, 0) == INVALID
        assert e.lib.rawdtw_reference_from_bases(e._ctx, 1, None, None, pore.ctypes.data, k, 0) == INVALID
        want = host[(name, False)]
        for s in (1, 7, 36):
            assert rc.same(e.reference_fetch(s, 0, len(want[2 * s + 1])), want[2 * s + 1])
    finally:
        e.close()


# ---- B. the seed table from the arena ---------------------------------------------------------------------------------------------------
def same_index(got: SeedIndex, want: SeedIndex, what):
    assert (got.n_seq, got.n_keys, got.n_positions, got.table_bytes) == (want.n_seq, want.n_keys, want.n_positions, want.table_bytes), what
    assert got.pars == want.pars
    keys = want.keys()
    assert np.array_equal(got.keys(), keys), what
    for h in keys.tolist():
        assert np.array_equal(got.get(h), want.get(h)), (what, h)
    for h in (0, 1, 0xFFFFFFFF, 12345):
        assert np.array_equal(got.get(h), want.get(h))


def signal_sets():
    """(name, forward arrays, reverse arrays): uploaded references the table is built from"""
    rng = np.random.default_rng(31)
    pore = synth.make_pore_model(6)

    def strands(n):
        s = rc._bases(rng, n + 5)
        return refsig.seq_to_sig(s, pore, 6, 1), refsig.seq_to_sig(s, pore, 6, 0)
    out = []
    for e in (2, 6, 9):  # s_len from e - 1 (no entry at all) up
        pairs = [strands(n) for n in (e - 1, e, e + 1, 700, 5000)]
        out.append((f"lengths_e{e}", [p[0] for p in pairs], [p[1] for p in pairs]))
    f, r = strands(3000)
    f, r = f.copy(), r.copy()
    f[200:420] = f[199]          # homopolymer stretches: runs of skipped events far longer than a step of 64
    r[1000:1070] = r[999] + np.float32(0.2)
    f[2000:2065] = f[1999]
    out.append(("homopolymer", [f], [r]))
    seg = strands(400)[0]
    a, b = strands(1500), strands(900)
    fa, rb = a[0].copy(), b[1].copy()
    fa[100:500], fa[900:1300], rb[300:700] = seg, seg, seg   # one segment across sequences and strands: keys with many positions
    out.append(("repeats", [fa, b[0], seg.copy()], [a[1], rb, seg.copy()]))
    f, r = strands(1200)
    f, r = f.copy(), r.copy()
    f[0], f[1], f[300:303], f[1199], r[64], r[127:129] = MASK_SIGNAL, MASK_SIGNAL, MASK_SIGNAL, MASK_SIGNAL, MASK_SIGNAL, MASK_SIGNAL
    out.append(("masked", [f], [r]))
    out.append(("one_short", [f[:3]], [r[:3]]))
    return out


@pytest.fixture(scope="module")
def sets():
    return signal_sets()


@pytest.mark.parametrize("q_lq", [(9, 3), (7, 4)])
@pytest.mark.parametrize("e", [2, 6, 9])
def test_device_table_equals_host_table(eng, sets, e, q_lq):
    p = SeedParams(e=e, q=q_lq[0], lq=q_lq[1])
    n_positions = 0
    for name, fwd, rev in sets:
        eng.upload_reference(fwd, rev)
        want = SeedIndex.from_signals(fwd, rev, p, threads=4)
        got = SeedIndex.from_device(eng, p)
        same_index(got, want, (name, e, q_lq))
        n_positions += want.n_positions
        if name == "repeats" and e == 6:
            assert max(len(want.get(h)) for h in want.keys().tolist()) >= 4
    assert n_positions > 10_000   # (the host's own count: with e = 2 the keys are few, the positions never)


def test_device_table_from_bases_and_its_hits(eng):
    """the table from an arena that came from bases, the multi-sequence case; seeding through it gives the host table's hits"""
    name, seqs, pore, k = _case("mixed37_k6")
    eng.reference_from_bases(seqs, pore, k, True)
    fwd = [refsig.seq_to_sig(s, pore, k, 1) for s in seqs]
    rev = [refsig.seq_to_sig(s, pore, k, 0) for s in seqs]
    want = SeedIndex.from_signals(fwd, rev, threads=4)
    got = SeedIndex.from_device(eng, SeedParams())
    same_index(got, want, name)
    rng = np.random.default_rng(4)
    long_ones = [x for x in fwd + rev if len(x) > 300]
    chunks = [(x[lo:lo + 250] + rng.normal(0, 0.03, 250)).astype(np.float32) for x in long_ones[:24] for lo in (int(rng.integers(0, len(x) - 250)),)]
    ev, off = np.concatenate(chunks), np.arange(len(chunks) + 1, dtype=np.uint64) * 250
    want_off, want_hits = seeding.seed_hits_host(want, ev, off)
    eng.upload_seed_index(got)
    got_off, got_hits = eng.seed_hits(ev, off)
    assert len(want_hits) > len(chunks) and np.array_equal(got_off, want_off) and got_hits.tobytes() == want_hits.tobytes()


def test_minimizer_windows_and_bad_calls_are_refused(eng, sets):
    name, fwd, rev = sets[0]
    eng.upload_reference(fwd, rev)
    before = eng.reference_fetch(4, 1, len(fwd[4]))
    with pytest.raises(RawDTWError) as err:
        SeedIndex.from_device(eng, SeedParams(w=5))
    assert err.value.status == UNSUPPORTED
    for bad in (SeedParams(e=1), SeedParams(e=10), SeedParams(q=0)):
        with pytest.raises(RawDTWError) as err:
            SeedIndex.from_device(eng, bad)
        assert err.value.status == INVALID
    assert eng.reference_fetch(4, 1, len(fwd[4])).tobytes() == before.tobytes() == fwd[4].tobytes()  # nothing changed
    same_index(SeedIndex.from_device(eng, SeedParams()), SeedIndex.from_signals(fwd, rev), "after the refusals")
    fresh = ra.Engine(0)
    try:
        with pytest.raises(RawDTWError) as err:
            SeedIndex.from_device(fresh, SeedParams())   # no reference on the context
        assert err.value.status == INVALID
    finally:
        fresh.close()


# ---- the tool: FASTA + model -> .ind ----------------------------------------------------------------------------------------------------
def test_build_index_writes_an_ind_that_reads_back(tmp_path, eng):
    """scripts/build_index.py: the file's signals are the host's (then k - 1 zeros, as ri_idx_dump writes l_seq floats), its buckets
    load to the table the host builds, and seeding through the loaded table gives the host table's hits"""
    import importlib.util
    import os

    from rawalign_amd.index import Index

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
    info = tool.build_index(str(fa), str(model), str(out))
    assert info["n_seq"] == 4 and info["k"] == 6
    fwd = [refsig.seq_to_sig(s, pore, k, 1) for _, s in records]
    rev = [refsig.seq_to_sig(s, pore, k, 0) for _, s in records]
    ix = Index(str(out))
    assert ix.names == [n for n, _ in records] and ix.lens == [len(s) for _, s in records] and (ix.w, ix.e, ix.q, ix.lq, ix.k) == (0, 6, 9, 3, 6)
    for i in range(4):
        for strand, want in ((1, fwd[i]), (0, rev[i])):
            got = ix.signal(i, strand)
            assert rc.same(got[:len(want)], want) and not np.any(got[len(want):])
    want = SeedIndex.from_signals(fwd, rev)
    got = SeedIndex.from_index(ix)
    assert (got.n_keys, got.n_positions) == (want.n_keys, want.n_positions) and want.n_keys > 3000
    for h in want.keys().tolist():
        assert np.array_equal(got.get(h), want.get(h)), h
    chunks = [(fwd[0][lo:lo + 300] + rng.normal(0, 0.03, 300)).astype(np.float32) for lo in rng.integers(0, 2600, 8)]
    ev, off = np.concatenate(chunks), np.arange(9, dtype=np.uint64) * 300
    want_off, want_hits = seeding.seed_hits_host(want, ev, off)
    eng.upload_seed_index(got)
    got_off, got_hits = eng.seed_hits(ev, off)
    assert len(want_hits) > 8 and np.array_equal(got_off, want_off) and got_hits.tobytes() == want_hits.tobytes()
    ix.close()


# ---- end to end: FASTA-side inputs to PAF lines ------------------------------------------------------------------------------------------
def test_paf_lines_from_bases_equal_those_from_host_arrays():
    bp, n = 20_000, 64
    g = synth.make_genome(bp, 515)
    bases = np.frombuffer(b"ACGT", np.uint8)[g].tobytes()
    pore = synth.make_pore_model(6)
    rng = np.random.default_rng(516)
    pa = synth.make_genome_raw_reads(g, rng.integers(0, bp - 1500, n), [1300] * n, rng.integers(0, 2, n), seed=517)
    fwd, rev = refsig.seq_to_sig(bases, pore, 6, 1), refsig.seq_to_sig(bases, pore, 6, 0)
    names, lens = ["genome"], [len(fwd)]
    reads = mapper.SignalReads(pa, lens)
    a, b = ra.Engine(0), ra.Engine(0)
    try:
        a.reference_from_bases([bases], pore, 6)
        six_a = SeedIndex.from_device(a, SeedParams())
        b.upload_reference([fwd], [rev])
        six_b = SeedIndex.from_signals([fwd], [rev])
        lines = []
        for e, six in ((a, six_a), (b, six_b)):
            cm = mapper.CMapper(e, ra.MapOpt(), StopOpt(), names, lens, slot_events=4096, max_reads=n, threads=3, carry=False, device_chain=True)
            got, rounds = mapper.map_reads_c(reads, list(range(n)), cm, seed_index=six, signal=True)
            cm.close()
            lines.append(got)
        assert lines[0] == lines[1]
        assert sum("\t*\t" not in ln for ln in lines[0]) >= n // 2   # (they map: the test is not one of empty lines)
    finally:
        a.close()
        b.close()
