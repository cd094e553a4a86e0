"""Seeding on the host (rawdtw_seed_host.cpp behind the C ABI): ri_sketch + ri_idx_get as gen_chains calls them
(src/rmap.cpp:364-391), pinned to the reference's recorded answers.  Every comparison is exact equality of integers, in order.
No device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import index as raindex
from rawalign_amd import mapper, seeding
from rawalign_amd._lib import SeedPars, load_library
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import HIT_DTYPE, SeedIndex, SeedParams
from tests import map_ref_cases as mc
from tests import seed_cases as sc
from tests.test_mapper_cpu import _oracle_scorer
from tests.util import OracleScorer

RANGE, INVALID = 4, 1


def _refmap():
    from oracle.loader import RefMap

    return RefMap


needs_ref = pytest.mark.skipif(not __import__("oracle.loader", fromlist=["RefMap"]).RefMap.available(),
                               reason="oracle/_ref/libref_map*.so are built only where the reference's sources are")


@pytest.fixture(scope="module")
def ref():
    return mc.make_reference()


@pytest.fixture(scope="module")
def six(ref):
    return SeedIndex.from_signals(ref.forward, ref.reverse, threads=3)


@pytest.fixture(scope="module")
def sfx():
    return sc.Fixture()


# ---- a plain-Python restatement (rsketch.c:223-274, rawindex.cpp:194-246, rmap.cpp:371-391), the 64-bit hash as the source has it ----
M64, M32 = (1 << 64) - 1, (1 << 32) - 1


def hash64(key, mask=M32):
    key = (~key + (key << 21)) & M64 & mask
    key = key ^ key >> 24
    key = ((key + (key << 3)) + (key << 8)) & M64 & mask
    key = key ^ key >> 14
    key = ((key + (key << 2)) + (key << 4)) & M64 & mask
    key = key ^ key >> 28
    key = (key + (key << 31)) & M64 & mask
    return key


def hash32(key):
    """rawdtw_seed.h's form: 32-bit arithmetic on the key's low half"""
    key &= M32
    key = (~key + (key << 21)) & M32
    key = key ^ key >> 24
    key = ((key + (key << 3)) + (key << 8)) & M32
    key = key ^ key >> 14
    key = ((key + (key << 2)) + (key << 4)) & M32
    key = key ^ key >> 28
    key = (key + (key << 31)) & M32
    return key


def py_sketch(ev, e=6, q=9, lq=3, wrong_start=False):
    """wrong_start: a filter that compares with 0 until an event is kept, instead of with event 0 (what the mask-first case is
    there to tell apart)"""
    ev = np.asarray(ev, np.float32)
    bits = ev.view(np.uint32)
    out, last, kept, quant = [], 0, 0, 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(ev)):
            ref = np.float32(0) if wrong_start and kept == 0 else ev[last]
            if (i > 0 and np.abs(np.float32(ev[i] - ref)) < sc.DIFF) or ev[i] == sc.MASK_SIGNAL:
                continue
            last = i
            b = int(bits[i])
            code = (b >> 30 << lq) | ((b >> (32 - q)) & ((1 << lq) - 1))
            quant = (quant << (lq + 2) | code) & ((1 << (lq + 2) * e) - 1)
            kept += 1
            if kept >= e:
                out.append((hash64(quant), i))
    return out


def py_index(fwd, rev, **p):
    table = {}
    for s in range(len(fwd)):
        for strand, arr in ((1, fwd[s]), (0, rev[s])):
            for h, i in py_sketch(arr, **p):
                table.setdefault(h, []).append(s << 32 | ((i << 1) & M32) | strand)
    for v in table.values():
        v.sort()
    return table


def py_hits(table, ev, **p):
    return [(y >> 32, y & 1, (y >> 1) & 0x7fffffff, i) for h, i in py_sketch(ev, **p) for y in table.get(h, ())]


def test_hash_in_32_bit_arithmetic_equals_the_64_bit_form():
    rng = np.random.default_rng(7)
    keys = rng.integers(0, 1 << 64, 200_000, dtype=np.uint64).tolist() + [0, 1, M32, M32 + 1, M64]
    assert all(hash32(k) == hash64(k) for k in keys)


# ---- 1. the committed mapping fixtures ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 4])
def test_hits_of_the_mapping_fixture(six, threads):
    """fails where the library has no seeding: the 10 860 hits of map_ref_inputs.npz, chunk by chunk"""
    fx = mc.Fixture()
    hoff, hits = seeding.seed_hits_host(six, fx.events, fx.ev_off, threads=threads)
    assert np.array_equal(hoff.astype(np.int64), fx.hit_off) and len(hits) == 10860
    for f in HIT_DTYPE.names:
        assert np.array_equal(hits[f], fx.hits[f]), f
    # the fixture exercises the code: events dropped by the 0.3 rule, a lookup with several positions, chunks without hits
    n_chunks = len(fx.ev_off) - 1
    dropped = 0
    for k in range(n_chunks):
        ev = fx.events[int(fx.ev_off[k]):int(fx.ev_off[k + 1])]
        last = 0
        for i in range(1, len(ev)):
            if abs(np.float32(ev[i] - ev[last])) < sc.DIFF:
                dropped += 1
            else:
                last = i
    assert dropped >= 1
    chunk_of_hit = np.searchsorted(fx.hit_off, np.arange(len(hits)), "right").astype(np.uint64)
    per_lookup = np.unique(chunk_of_hit << np.uint64(32) | hits["query_position"].astype(np.uint64), return_counts=True)[1]
    assert per_lookup.max() > 1                                    # (a hit's query position names its sketch element)
    assert sum(1 for k in range(n_chunks) if fx.hit_off[k + 1] == fx.hit_off[k]) >= 1


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("form", mc.FORMS)
def test_hits_of_the_whole_read_fixture(six, form, threads):
    w = mc.WholeReads(form)
    hoff, hits = seeding.seed_hits_host(six, w.events, w.ev_off, threads=threads)
    assert np.array_equal(hoff.astype(np.int64), w.hit_off) and len(hits) == (1756, 1753)[form]
    assert [tuple(int(v) for v in r) for r in sc.hit_rows(hits)] == [tuple(h) for h in w.hits]


# ---- 2. the seeding fixture ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.CASES)
def test_fixture_belongs_to_the_inputs_made_today(sfx, name):
    fwd, rev, _, chunks = sc.build_case(name)
    assert sc.case_sha256(fwd, rev, chunks) == sfx.sha(name)


@pytest.mark.parametrize("name", sc.CASES)
def test_sketch_and_hits_against_the_reference(sfx, name):
    fwd, rev, p, chunks = sc.build_case(name)
    si = SeedIndex.from_signals(fwd, rev, p, threads=2)
    for c, ev in enumerate(chunks):
        h, pos = seeding.sketch(ev, p)
        wh, wp = sfx.sketch(name, c)
        assert np.array_equal(h, wh) and np.array_equal(pos, wp), (name, c)
    ev, off = sc.flat(chunks)
    for threads in (1, 3):
        hoff, hits = seeding.seed_hits_host(si, ev, off, threads=threads)
        assert np.array_equal(hoff, sfx.hit_off(name)) and np.array_equal(sc.hit_rows(hits), sfx.hits(name)), name


def test_fixture_coverage(sfx):
    """what the cases are there for is really in them"""
    fwd, rev, p, chunks = sc.build_case("edges")
    assert [len(c) for c in chunks[:5]] == [0, 1, p.e - 1, p.e, p.e + 1]
    assert [len(sfx.sketch("edges", c)[0]) for c in range(5)] == [0, 0, 0, 1, 2]
    th = chunks[5]
    _, pos = sfx.sketch("edges", 5)
    base = 60   # threshold_chunk: groups of (-2, 0.25, y, 2) from event 60 on; y is event 62 + 4 g
    kept = [int(62 + 4 * g) in pos.tolist() for g in range(6)]
    assert kept == [False, True, True, True, False, True], (kept, th[base:base + 24])   # (the last: kept only in fp32)
    sp = chunks[6]
    _, pos = sfx.sketch("edges", 6)
    nan_at = int(np.nonzero(np.isnan(sp))[0][0])
    # a NaN is kept (the compare is ordered), and so is the event behind it whatever its value; `last` then sits on that event,
    # and its double is dropped again
    assert {nan_at, nan_at + 1} <= set(pos.tolist()) and nan_at + 2 not in pos.tolist() and sp[nan_at + 1] == sp[nan_at + 2]
    assert not set(np.nonzero(sp == sc.MASK_SIGNAL)[0].tolist()) & set(pos.tolist())
    assert any(np.isinf(sp[i]) for i in pos.tolist())
    assert len(sfx.sketch("edges", 7)[0]) == 0 and len(sfx.sketch("edges", 8)[0]) == 0
    rows = sfx.hits("motif")
    assert np.unique(rows[:int(sfx.hit_off("motif")[1]), 3], return_counts=True)[1].max() > 1024
    assert len(sfx.hits("w255")) <= 2 < len(sfx.hits("w10")) < len(sfx.hits("w5")) < len(sfx.hits("w1"))


def test_mask_first_case_tells_a_filter_that_starts_from_nothing(sfx, six):
    """every chunk of the case begins with RI_MASK_SIGNAL, and the HITS of each differ when the events behind a masked event 0
    are compared with 0 instead of with the mask value: a device test on hits alone pins the rule"""
    _, _, p, chunks = sc.build_case("maskfirst")
    hoff, rows = sfx.hit_off("maskfirst"), sfx.hits("maskfirst")
    for c, ev in enumerate(chunks):
        assert ev[0] == sc.MASK_SIGNAL
        want = [tuple(int(v) for v in r) for r in rows[int(hoff[c]):int(hoff[c + 1])]]
        right = [(int(y) >> 32, int(y) & 1, (int(y) >> 1) & 0x7fffffff, i) for h, i in py_sketch(ev) for y in six.get(h)]
        wrong = [(int(y) >> 32, int(y) & 1, (int(y) >> 1) & 0x7fffffff, i) for h, i in py_sketch(ev, wrong_start=True) for y in six.get(h)]
        assert right == want and wrong != want and len(want) > 0, c


# ---- 3. the plain-Python restatement on random inputs ------------------------------------------------------------------------------
@pytest.mark.parametrize("e,q,lq", [(6, 9, 3), (3, 12, 5), (9, 6, 1), (2, 9, 3)])
def test_against_a_plain_python_restatement(e, q, lq):
    rng = np.random.default_rng(100 * e + q)
    n = 400 if e == 2 else 3000
    fwd = [rng.normal(0, 1, n).astype(np.float32), np.round(rng.normal(0, 1, n // 2), 1).astype(np.float32)]
    rev = [x[::-1].copy() for x in fwd]
    rev[1][:100] = fwd[0][50:150]
    table = py_index(fwd, rev, e=e, q=q, lq=lq)
    p = SeedParams(e=e, q=q, lq=lq)
    si = SeedIndex.from_signals(fwd, rev, p, threads=2)
    assert si.n_keys == len(table) and si.n_positions == sum(len(v) for v in table.values())
    assert sorted(si.keys().tolist()) == sorted(table)
    for h, v in table.items():
        assert si.get(h).tolist() == v
    chunks = []
    for k in range(12):
        s = int(rng.integers(0, 2))
        arr = (fwd, rev)[k % 2][s]
        lo = int(rng.integers(0, len(arr) - 100))
        ch = (arr[lo:lo + int(rng.integers(0, 100))] + rng.normal(0, 0.03, 1)[0]).astype(np.float32)
        if k % 4 == 0 and len(ch) > 10:
            ch[rng.integers(0, len(ch), 3)] = (np.nan, sc.MASK_SIGNAL, np.inf)
        chunks.append(ch)
    ev, off = sc.flat(chunks)
    hoff, hits = seeding.seed_hits_host(si, ev, off, threads=2)
    for c, ch in enumerate(chunks):
        sk = py_sketch(ch, e=e, q=q, lq=lq)
        h, pos = seeding.sketch(ch, p)
        assert list(zip(h.tolist(), pos.tolist())) == sk
        want = py_hits(table, ch, e=e, q=q, lq=lq)
        got = [tuple(int(v) for v in r) for r in sc.hit_rows(hits[int(hoff[c]):int(hoff[c + 1])])]
        assert got == want, (c, len(got), len(want))


# ---- 4. the index file -----------------------------------------------------------------------------------------------------------
def _same_table(a, b, rng):
    assert (a.n_keys, a.n_positions, a.n_seq, a.pars) == (b.n_keys, b.n_positions, b.n_seq, b.pars)
    keys = np.sort(a.keys())
    assert np.array_equal(keys, np.sort(b.keys()))
    for h in keys.tolist():
        assert np.array_equal(a.get(h), b.get(h)), h
    absent = [int(h) for h in rng.integers(0, 1 << 32, 4000) if int(h) not in set(keys.tolist())][:1000]
    assert len(absent) == 1000 and all(len(b.get(h)) == 0 for h in absent) and len(b.get(1 << 40)) == 0
    return keys, absent


def test_index_file_round_trip(tmp_path, ref, six):
    path = str(tmp_path / "with_buckets.ind")
    raindex.write_index(path, ref.names, ref.forward, ref.reverse, buckets=True)
    ix = raindex.Index(path)
    loaded = SeedIndex.from_index(ix)
    _same_table(six, loaded, np.random.default_rng(3))
    assert np.array_equal(ix.signal(1, 0), ref.reverse[1])   # (the sequences' part is what it was)
    # the default stays what it was: empty buckets, which load as an empty index
    path0 = str(tmp_path / "empty.ind")
    raindex.write_index(path0, ref.names, ref.forward, ref.reverse)
    assert os.path.getsize(path0) < os.path.getsize(path)
    empty = SeedIndex.from_index(raindex.Index(path0))
    assert empty.n_keys == 0 and len(empty.get(int(six.keys()[0]))) == 0
    # a given SeedIndex is written as it is
    path2 = str(tmp_path / "given.ind")
    raindex.write_index(path2, ref.names, ref.forward, ref.reverse, buckets=six)
    assert open(path2, "rb").read() == open(path, "rb").read()
    # a file cut short inside the buckets is refused
    cut = str(tmp_path / "cut.ind")
    open(cut, "wb").write(open(path, "rb").read()[:-7])
    with pytest.raises(ra.RawDTWError):
        SeedIndex.from_index(raindex.Index(cut))


class _RefIndex:
    """the reference's ri_idx_load / ri_idx_get / ri_idx_dump (exported by oracle/_ref/libref_map0.so) on a FILE* of libc's"""

    def __init__(self):
        self.lib = C.CDLL(_refmap().path(False))
        self.libc = C.CDLL(None)
        self.libc.fopen.restype = C.c_void_p
        self.libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        self.libc.fclose.argtypes = [C.c_void_p]
        self.lib.ri_idx_load.restype = C.c_void_p
        self.lib.ri_idx_load.argtypes = [C.c_void_p]
        self.lib.ri_idx_dump.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.ri_idx_get.restype = C.POINTER(C.c_uint64)
        self.lib.ri_idx_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int)]

    def load(self, path):
        f = self.libc.fopen(path.encode(), b"rb")
        ri = self.lib.ri_idx_load(f)
        self.libc.fclose(f)
        assert ri
        return ri

    def dump(self, ri, path):
        f = self.libc.fopen(path.encode(), b"wb")
        self.lib.ri_idx_dump(f, ri)
        self.libc.fclose(f)

    def get(self, ri, h):
        n = C.c_int()
        p = self.lib.ri_idx_get(ri, int(h), C.byref(n))
        return [int(p[i]) for i in range(n.value)]


@needs_ref
def test_index_file_against_the_reference_reader_and_writer(tmp_path, ref, six):
    path = str(tmp_path / "ours.ind")
    raindex.write_index(path, ref.names, ref.forward, ref.reverse, buckets=six)
    R = _RefIndex()
    ri = R.load(path)
    rng = np.random.default_rng(4)
    keys = np.sort(six.keys())
    have = set(keys.tolist())
    for h in keys.tolist():
        assert R.get(ri, h) == six.get(h).tolist(), h
    absent = [int(h) for h in rng.integers(0, 1 << 32, 4000) if int(h) not in have][:1000]
    assert all(R.get(ri, h) == [] for h in absent)
    theirs = str(tmp_path / "theirs.ind")
    R.dump(ri, theirs)
    _same_table(six, SeedIndex.from_index(raindex.Index(theirs)), rng)


# ---- 5. live ------------------------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_live_reference_on_random_chunks(ref, seed):
    rng = np.random.default_rng(9000 + seed)
    e = int(rng.integers(3, 10))
    lq = int(rng.integers(1, 5))
    q = int(rng.integers(lq + 2, 13))
    w = (0, 0, 0, 7)[seed - 1]
    p = SeedParams(w=w, e=e, q=q, lq=lq)
    rm = _refmap()(ref.forward, ref.reverse, e=e, q=q, lq=lq, w=w)
    si = SeedIndex.from_signals(ref.forward, ref.reverse, p, threads=2)
    chunks = []
    for k in range(50):
        s = int(rng.integers(0, ref.n_seq))
        arr = (ref.forward, ref.reverse)[k % 2][s]
        lo = int(rng.integers(0, len(arr) - 400))
        chunks.append((arr[lo:lo + int(rng.integers(1, 400))] + rng.normal(0, rng.choice([0.02, 0.1]), 1)[0]).astype(np.float32))
    ev, off = sc.flat(chunks)
    hoff, hits = seeding.seed_hits_host(si, ev, off, threads=3)
    total = 0
    for c, ch in enumerate(chunks):
        want = rm.hits(ch)
        assert np.array_equal(sc.hit_rows(hits[int(hoff[c]):int(hoff[c + 1])]), want), (p, c)
        total += len(want)
    assert total > 100, (p, total)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ref, six):
    lib = load_library()
    fx = mc.Fixture()
    ev, off = np.ascontiguousarray(fx.events[:int(fx.ev_off[4])]), np.ascontiguousarray(fx.ev_off[:5], np.uint64)
    want_off, want = seeding.seed_hits_host(six, ev, off)
    total = int(want_off[-1])
    assert total > 10
    hoff = np.zeros(5, np.uint64)
    hits = np.full(total, 0xAB, np.uint8).repeat(16).view(HIT_DTYPE)
    canary = hits.copy()
    st = lib.rawdtw_seed_hits_host(six._h, 4, off.ctypes.data, ev.ctypes.data, hoff.ctypes.data, hits.ctypes.data, total - 1, 2)
    assert st == RANGE and np.array_equal(hoff, want_off) and np.array_equal(hits, canary)
    st = lib.rawdtw_seed_hits_host(six._h, 4, off.ctypes.data, ev.ctypes.data, hoff.ctypes.data, hits.ctypes.data, total, 2)
    assert st == 0 and np.array_equal(hits, want)
    with pytest.raises(ra.RawDTWError) as ei:
        seeding.seed_hits_host(six, ev, off, hits_cap=3)
    assert ei.value.status == RANGE and np.array_equal(ei.value.hit_off, want_off)
    # null arguments, offsets that descend
    assert lib.rawdtw_seed_hits_host(None, 4, off.ctypes.data, ev.ctypes.data, hoff.ctypes.data, hits.ctypes.data, total, 1) == INVALID
    assert lib.rawdtw_seed_hits_host(six._h, 4, None, ev.ctypes.data, hoff.ctypes.data, hits.ctypes.data, total, 1) == INVALID
    assert lib.rawdtw_seed_hits_host(six._h, 4, off.ctypes.data, None, hoff.ctypes.data, hits.ctypes.data, total, 1) == INVALID
    assert lib.rawdtw_seed_hits_host(six._h, 4, off.ctypes.data, ev.ctypes.data, None, hits.ctypes.data, total, 1) == INVALID
    assert lib.rawdtw_seed_hits_host(six._h, 4, off.ctypes.data, ev.ctypes.data, hoff.ctypes.data, None, total, 1) == INVALID
    bad = off.copy()
    bad[2] = bad[1] - 1
    assert lib.rawdtw_seed_hits_host(six._h, 4, bad.ctypes.data, ev.ctypes.data, hoff.ctypes.data, hits.ctypes.data, total, 1) == INVALID
    # parameters the reference asserts on, or shifts out of range with
    h = C.c_void_p()
    n = C.c_uint32()
    buf = np.zeros(16, np.uint32)
    for kw in (dict(e=1), dict(e=10), dict(w=256), dict(q=0), dict(q=33), dict(lq=31), dict(e=8, lq=6), dict(e=9, lq=6)):
        p = SeedParams(**kw)
        with pytest.raises(ra.RawDTWError) as ei:
            SeedIndex.from_signals(ref.forward, ref.reverse, p)
        assert ei.value.status == INVALID, kw
        assert lib.rawdtw_seed_sketch(C.byref(p.c()), ev.ctypes.data, 16, buf.ctypes.data, buf.ctypes.data, C.byref(n)) == INVALID
    assert SeedIndex.from_signals(ref.forward[:1], ref.reverse[:1], SeedParams(e=9, lq=5, q=32)).n_keys > 0   # (63 bits: allowed)
    assert lib.rawdtw_seed_index_build(1, None, None, None, C.byref(SeedPars(0, 6, 0, 9, 3, 6)), 1, C.byref(h)) == INVALID
    assert lib.rawdtw_seed_index_get(six._h, 5, None, None) == INVALID
    # no sequences: an empty index, no hits
    e0 = SeedIndex.from_signals([], [])
    assert e0.n_keys == 0 and seeding.seed_hits_host(e0, ev, off)[0].tolist() == [0] * 5


# ---- 7. the mapper ------------------------------------------------------------------------------------------------------------------
def _c_mapper(fx, opt, copt, scorer, **kw):
    cm = mapper.CMapper(None, opt, StopOpt(), ["seq%d" % s for s in range(len(fx.lens))], [int(x) for x in fx.lens], slot_events=2048,
                        max_reads=fx.n_reads + 1, chain_opt=copt, output_chains=True, **kw)
    cm.set_scorer(scorer)
    return cm


@pytest.mark.parametrize("name,threads", [("default", 1), ("nbest5", 4)])
def test_mapper_round_seeded_equals_the_round_on_the_fixture_hits(oracle, ref, six, name, threads):
    fx = mc.Fixture(ref=ref)
    opt, copt = mc.project_opts(name, 0)
    opt.flag = (opt.flag & ~mc.CIGAR) | 0x8   # (--dtw-log-scores: the log is compared too)
    score = _oracle_scorer(oracle, ref, opt)
    reads = list(range(fx.n_reads))
    cm = _c_mapper(fx, opt, copt, score, threads=threads)
    want, rounds = mapper.map_reads_c(fx, reads, cm)
    want_log = cm.log()
    cm.close()
    cm = _c_mapper(fx, opt, copt, score, threads=threads)
    got, rounds_s = mapper.map_reads_c(fx, reads, cm, seed_index=six)
    assert got == want and rounds_s == rounds and cm.log() == want_log and want_log
    assert sum("\t*\t" not in ln for ln in got) >= fx.n_reads // 2
    # a seed index with another number of sequences is refused, and nothing changes
    other = SeedIndex.from_signals(ref.forward[:2], ref.reverse[:2])
    rid = cm.add_read("late", 4000, 1)
    ev = fx.chunk(0, 0)[0]
    with pytest.raises(RuntimeError, match="status 1"):
        cm.round([rid], [(ev, [])], seed_index=other)
    assert cm.state(rid) == (False, 0)
    cm.round([rid], [(ev, [])], seed_index=six)
    assert cm.state(rid)[1] == 1
    cm.close()


def test_python_mirror_on_index_seeds_equals_the_fixture_hits(oracle, ref, six):
    fx = mc.Fixture(ref=ref)
    reads = list(range(0, fx.n_reads, 3))
    opt, _ = mc.project_opts("default", 0)
    seeds = mapper.IndexSeeds(six, [[fx.chunk(r, c)[0] for c in range(fx.n_chunks(r))] for r in range(fx.n_reads)], fx.lens)
    for r in reads[:4]:
        for c in range(fx.n_chunks(r)):
            assert seeds.chunk(r, c)[1] == fx.chunk(r, c)[1]
    want = mapper.map_reads(fx, reads, OracleScorer(oracle, ref), opt, StopOpt())
    got = mapper.map_reads(seeds, reads, OracleScorer(oracle, ref), opt, StopOpt())
    assert got == want
