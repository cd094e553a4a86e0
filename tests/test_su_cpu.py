"""--sequence-until and --output-chains through the library (rawdtw_su_*, rawdtw_mapper_su_* / set_sequence_until / batch_records,
flag 0x20 of rawdtw_mapper_paf) without a device.

The state machine (rawalign_amd/csrc/rawdtw_su.cpp) against the plain-Python restatement mapping.SequenceUntil on random record
streams; the mapper driven through the harness hook rawdtw_mapper_set_scorer with the oracle as the scorer (as
tests/test_mapper_cpu.py does) against an independent restatement of rmap.cpp:918-965: the Python mirror per mini-batch, then
SequenceUntil over its lines in order, then the gate of rmap.cpp:960 -- whole lines compared."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapper, synth
from rawalign_amd.mapping import SequenceUntil, StopOpt
from tests.test_mapper_cpu import _oracle_scorer
from tests.util import OracleScorer

RAWDTW_ERR_INVALID = 1


# ------------------------------------------------------------------------------------------------
# the state on its own
# ------------------------------------------------------------------------------------------------
def _stream(rng, n, n_seq, wrap=False, mapped_frac=0.75):
    mapped = (rng.random(n) < mapped_frac).astype(np.uint8)
    ref_id = rng.integers(0, n_seq + 1, n).astype(np.uint32)   # (n_seq: a record on no sequence, never counted)
    frag = (rng.integers(2 ** 32 - 5000, 2 ** 32, n) if wrap else rng.integers(50, 9000, n)).astype(np.uint32)
    return mapped, ref_id, frag


def _python_walk(su, mapped, ref_id, frag, n_seq):
    """the reference's loop (rmap.cpp:918-944) with the restatement: the records that count, in order"""
    for k in range(len(mapped)):
        if mapped[k] and ref_id[k] < n_seq and su.add_mapped_read(int(ref_id[k]), int(frag[k]), k):
            break
    return su.stop


def _assert_same_state(c, p):
    assert c.nreads == p.nreads and c.nestimations == p.nestimations and c.ab_count == p.ab_count
    assert np.array_equal(c.c_estimations, p.c_estimations)


PARAMS = [dict(t_threshold=1.5, tn_samples=5, ttest_freq=500, tmin_reads=500),      # roptions.c:43-46
          dict(t_threshold=1.5, tn_samples=3, ttest_freq=7, tmin_reads=20),         # stops inside the first test
          dict(t_threshold=0.02, tn_samples=4, ttest_freq=5, tmin_reads=10),
          dict(t_threshold=0.0005, tn_samples=2, ttest_freq=3, tmin_reads=0),
          dict(t_threshold=-1.0, tn_samples=2, ttest_freq=4, tmin_reads=3),         # never stops
          dict(t_threshold=1e-6, tn_samples=1, ttest_freq=1, tmin_reads=1)]


@pytest.mark.parametrize("contracted", [0, 1])
@pytest.mark.parametrize("pi", range(len(PARAMS)))
@pytest.mark.parametrize("wrap", [False, True])
def test_state_equals_the_restatement(pi, contracted, wrap):
    n_seq = 5
    prm = dict(PARAMS[pi], contracted=bool(contracted))
    for seed in range(4):
        rng = np.random.default_rng(1000 * pi + 10 * seed + contracted)
        mapped, ref_id, frag = _stream(rng, 3000, n_seq, wrap=wrap)
        want = SequenceUntil(n_seq, **prm)
        stop = _python_walk(want, mapped, ref_id, frag, n_seq)
        one = mapper.CSequenceUntil(n_seq, **prm)           # the whole stream in one call
        assert one.feed(mapped, ref_id, frag) == stop
        _assert_same_state(one, want)
        # in pieces: the stop counts from the first record of the call that fired, and every later call repeats it
        parts = mapper.CSequenceUntil(n_seq, **prm)
        cuts = np.sort(rng.choice(np.arange(1, len(mapped)), 9, replace=False))
        lo, got, local = 0, 0, 0
        for hi in list(cuts) + [len(mapped)]:
            s = parts.feed(mapped[lo:hi], ref_id[lo:hi], frag[lo:hi])
            if got:
                assert s == local
            elif s:
                got, local = lo + s, s
            lo = hi
        assert got == stop
        _assert_same_state(parts, want)
        # record by record through the interface shard.sequence_until_round walks
        rec = mapper.CSequenceUntil(n_seq, **prm)
        assert _python_walk(rec, mapped, ref_id, frag, n_seq) == stop
        _assert_same_state(rec, want)
        if pi == 4:
            assert stop == 0 and want.nestimations > prm["tn_samples"]
        if pi == 1:   # the first test passes: the (tn_samples + 1)-th estimation
            assert stop > 0 and want.nestimations == prm["tn_samples"] + 1
        if wrap:   # two fragments near 2**32 already wrap the uint32 counters
            assert want.nreads >= 2


def test_state_refuses_what_the_reference_divides_by_zero_on():
    from rawalign_amd._lib import SuOpt, load_library

    lib = load_library()
    h = C.c_void_p()
    for n_seq, o in ((0, SuOpt(1.5, 5, 500, 500, 0)), (3, SuOpt(1.5, 0, 500, 500, 0)), (3, SuOpt(1.5, 5, 0, 500, 0))):
        assert lib.rawdtw_su_create(n_seq, C.byref(o), C.byref(h)) == RAWDTW_ERR_INVALID and not h.value
    assert lib.rawdtw_su_create(3, None, C.byref(h)) == 0 and h.value   # NULL: roptions.c:43-46
    s = C.c_uint32(7)
    assert lib.rawdtw_su_feed(h, 1, None, None, None, C.byref(s)) == RAWDTW_ERR_INVALID
    assert lib.rawdtw_su_feed(h, 0, None, None, None, C.byref(s)) == 0 and s.value == 0
    lib.rawdtw_su_destroy(h)
    with pytest.raises(RuntimeError):
        mapper.CSequenceUntil(2, ttest_freq=0)


# ------------------------------------------------------------------------------------------------
# the mapper
# ------------------------------------------------------------------------------------------------
REF = None


def _ref():
    global REF
    if REF is None:
        REF = synth.make_reference([24000, 15000, 9000], seed=20231005 + 31)
    return REF


def _seeds(n, seed=17):
    return mapper.SyntheticSeeds(_ref(), n, seed=seed, max_chunks=4)


def _cmapper(oracle, seeds, opt, stop, n, threads=3, **kw):
    ref = _ref()
    cm = mapper.CMapper(None, opt, stop, [f"seq{s}" for s in range(ref.n_seq)], [len(x) for x in ref.forward],
                        slot_events=max(rd["n_ev"] for rd in seeds.reads) + 8, max_reads=n, carry=True, threads=threads, **kw)
    cm.set_scorer(_oracle_scorer(oracle, ref, opt))
    return cm


def gate(line):
    """rmap.cpp:960/965 for a mapped read at or after the stop point: name, read_length (= read_end), nine '*', mapq, its tags"""
    f = line.split("\t")
    return "\t".join([f[0], f[1]] + ["*"] * 9 + [f[11]] + f[12:])


def restatement(oracle, seeds, batches, opt, stop, su_kw, output_chains=False):
    """the Python mirror per mini-batch (ungated), SequenceUntil over its lines in output order, the gate; returns
    ({read: line}, index of the stop batch or None, the SequenceUntil)"""
    ref = _ref()
    names = [f"seq{s}" for s in range(ref.n_seq)]
    su = SequenceUntil(ref.n_seq, **su_kw)
    lines = {}
    for bi, b in enumerate(batches):
        got, _ = mapper.map_reads(seeds, b, OracleScorer(oracle, ref), opt, stop, output_chains=output_chains)
        for k, line in enumerate(got):
            f = line.split("\t")
            if f[2] != "*" and su.add_mapped_read(names.index(f[5]), int(f[10]), k):
                break
        for k, (r, line) in enumerate(zip(b, got)):
            lines[r] = gate(line) if su.stop and k >= su.stop and line.split("\t")[2] != "*" else line
        if su.stop:
            return lines, bi, su
    return lines, None, su


SU_KW = [dict(t_threshold=1.5, tn_samples=2, ttest_freq=2, tmin_reads=3),
         dict(t_threshold=1.5, tn_samples=1, ttest_freq=3, tmin_reads=8),
         dict(t_threshold=1.5, tn_samples=3, ttest_freq=1, tmin_reads=14, contracted=True)]


@pytest.mark.parametrize("case", [(0x2, 7, 0), (0x2, 11, 1), (0x2 | 0x8, 13, 2), (0x2, 9, 1)])
def test_mapper_sequence_until_equals_the_restatement(oracle, case):
    flag, bsz, ki = case
    su_kw = SU_KW[ki]
    n = 6 * bsz
    seeds = _seeds(n)
    opt, stop = ra.MapOpt(flag=flag), StopOpt()
    ids = list(range(n))
    batches = [ids[i:i + bsz] for i in range(0, n, bsz)]
    want, stop_batch, su = restatement(oracle, seeds, batches, opt, stop, su_kw)
    assert stop_batch in (1, 2), "the parameters are meant to stop in the second or third batch"
    cm = _cmapper(oracle, seeds, opt, stop, n, sequence_until=su_kw)
    got, rounds = mapper.map_reads_c(seeds, ids, cm, batch_size=bsz)
    stopped, n_mapped = cm.su_state()
    assert stopped and n_mapped == su.nreads
    for r in ids:
        assert got[r] == want.get(r, ""), r
    # the same run without sequence-until: every line ungated, more rounds
    cm_off = _cmapper(oracle, seeds, opt, stop, n)
    off, rounds_off = mapper.map_reads_c(seeds, ids, cm_off, batch_size=bsz)
    want_off, _ = mapper.map_reads(seeds, ids, OracleScorer(oracle, _ref()), opt, stop)
    assert off == want_off
    assert rounds < rounds_off and cm.stats()[0] < cm_off.stats()[0]
    assert cm_off.su_state() == (False, 0)
    cm.close()
    cm_off.close()


def test_split_form_in_one_process_equals_su_batch(oracle):
    """batch_records + the walk of shard.sequence_until_round over a CSequenceUntil + su_apply writes what su_batch writes"""
    bsz, n = 10, 60
    seeds = _seeds(n, seed=23)
    opt, stop = ra.MapOpt(), StopOpt()
    su_kw = SU_KW[0]
    a = _cmapper(oracle, seeds, opt, stop, n, sequence_until=su_kw)
    la, ra_ = mapper.map_reads_c(seeds, list(range(n)), a, batch_size=bsz)
    b = _cmapper(oracle, seeds, opt, stop, n, sequence_until=su_kw)
    csu = mapper.CSequenceUntil(_ref().n_seq, **su_kw)
    lb, rb = mapper.map_reads_c(seeds, list(range(n)), b, batch_size=bsz, su=csu)
    assert la == lb and ra_ == rb and a.su_state() == b.su_state() and a.su_state()[0]
    assert csu.nreads == a.su_state()[1]
    a.close()
    b.close()


def _run_batch(cm, seeds, rids, reads):
    while True:
        act = [(rid, r) for rid, r in zip(rids, reads) if not cm.state(rid)[0]]
        if not act:
            return
        cm.round([rid for rid, _ in act], [seeds.chunk(r, cm.state(rid)[1]) for rid, r in act])


def test_reads_in_flight_are_dropped_and_frozen(oracle):
    """the stop fires in batch 0 while batch 1 is in flight (one round done): batch 1's reads are finished at once with their
    chunks_done as they were, run no further round and have no line; a read added afterwards is born finished; the gated
    lines of batch 0 follow rmap.cpp:960/965"""
    n = 20
    seeds = _seeds(n, seed=29)
    opt, stop = ra.MapOpt(), StopOpt()
    su_kw = dict(t_threshold=1.5, tn_samples=1, ttest_freq=1, tmin_reads=0)   # the test passes at the second mapped read
    cm = _cmapper(oracle, seeds, opt, stop, n + 1, sequence_until=su_kw)
    b0, b1 = list(range(10)), list(range(10, 20))
    id0 = [cm.add_read(seeds.read_job(r).name, seeds.read_job(r).qlen, seeds.read_job(r).n_chunks_available) for r in b0]
    id1 = [cm.add_read(seeds.read_job(r).name, seeds.read_job(r).qlen, seeds.read_job(r).n_chunks_available) for r in b1]
    cm.round(id0 + id1, [seeds.chunk(r, 0) for r in b0 + b1])
    _run_batch(cm, seeds, id0, b0)
    before = [cm.state(i) for i in id1]
    assert any(not f for f, _ in before)
    rounds_before = cm.stats()[0]
    s = cm.su_batch(id0)
    want, stop_batch, su = restatement(oracle, seeds, [b0], opt, stop, su_kw)
    assert s == su.stop > 0 and stop_batch == 0
    assert [cm.state(i) for i in id1] == [(True, d) for _, d in before]
    with pytest.raises(RuntimeError):
        cm.round([id1[0]], [seeds.chunk(b1[0], before[0][1])])
    late = cm.add_read("late", 8000, 2)
    assert cm.state(late) == (True, 0)
    cm.finish()
    assert [cm.paf(i) for i in id0] == [want[r] for r in b0]
    assert all(cm.paf(i) == "" for i in id1 + [late])
    assert any(cm.paf(i) == gate(cm.paf(i)) and cm.paf(i).split("\t")[3] == "*" and k >= s for k, i in enumerate(id0)), "no gated line"
    assert cm.stats()[0] == rounds_before
    assert cm.su_state() == (True, su.nreads)
    assert cm.su_batch(id1) == s                                # a batch after the stop: the stop again, still no lines
    assert all(cm.paf(i) == "" for i in id1)
    cm.release_read(late)
    cm.close()


def test_refused_calls_leave_the_state_unchanged(oracle):
    from rawalign_amd._lib import SuOpt

    n = 12
    seeds = _seeds(n, seed=31)
    opt, stop = ra.MapOpt(), StopOpt()
    cm = _cmapper(oracle, seeds, opt, stop, n)
    lib, h = cm.lib, cm._h
    ids = [cm.add_read(seeds.read_job(r).name, seeds.read_job(r).qlen, seeds.read_job(r).n_chunks_available) for r in range(n)]
    arr = np.array(ids[:4], np.uint32)
    s = C.c_uint32()
    assert lib.rawdtw_mapper_su_batch(h, 4, mapper._vp(arr), C.byref(s)) == RAWDTW_ERR_INVALID       # sequence-until is off
    for bad in (SuOpt(1.5, 0, 5, 5, 0), SuOpt(1.5, 3, 0, 5, 0)):
        assert lib.rawdtw_mapper_set_sequence_until(h, C.byref(bad)) == RAWDTW_ERR_INVALID
    assert cm.su_state() == (False, 0)
    cm.set_sequence_until(t_threshold=-1.0, tn_samples=1, ttest_freq=1, tmin_reads=0)   # (never stops)
    _run_batch(cm, seeds, ids[:4], list(range(4)))
    cm.round(ids[4:6], [seeds.chunk(r, 0) for r in (4, 5)])
    unfinished = [i for i in ids[4:] if not cm.state(i)[0]]
    assert unfinished
    for batch in ([ids[0], unfinished[0]], [ids[0], ids[0]], [ids[0], 999]):
        a = np.array(batch, np.uint32)
        assert lib.rawdtw_mapper_su_batch(h, len(a), mapper._vp(a), C.byref(s)) == RAWDTW_ERR_INVALID
        assert lib.rawdtw_mapper_su_apply(h, len(a), mapper._vp(a), 0) == RAWDTW_ERR_INVALID
    assert lib.rawdtw_mapper_su_apply(h, 4, mapper._vp(arr), 5) == RAWDTW_ERR_INVALID                # first_gated past the batch
    assert cm.su_state() == (False, 0) and all(cm.paf(i) for i in ids[:4])
    rec = cm.batch_records(ids[:4])
    assert cm.su_batch(ids[:2]) == 0                                                                 # the first batch closes...
    assert lib.rawdtw_mapper_set_sequence_until(h, None) == RAWDTW_ERR_INVALID                        # ... and the parameters are fixed
    a = np.array(ids[:2], np.uint32)
    assert lib.rawdtw_mapper_su_batch(h, 2, mapper._vp(a), C.byref(s)) == RAWDTW_ERR_INVALID          # closed before
    m, r_, f = cm.batch_records(ids[:4])
    assert all(np.array_equal(x, y) for x, y in zip(rec, (m, r_, f)))                                 # (records change nothing)
    for k in range(4):
        line = cm.paf(ids[k]).split("\t")
        assert bool(m[k]) == (line[2] != "*")
        if m[k]:
            assert r_[k] == int(line[5][3:]) and f[k] == int(line[10])
    cm.close()


def test_output_chains_lines_equal_the_mirror(oracle):
    """flag 0x20: anchors:s: after aln:s:, mapped lines only, "(query,target)" per anchor of chains[0] in stored order"""
    n = 24
    seeds = _seeds(n, seed=37)
    for flag in (0x2, 0x2 | 0x8):
        opt, stop = ra.MapOpt(flag=flag), StopOpt()
        want, _ = mapper.map_reads(seeds, list(range(n)), OracleScorer(oracle, _ref()), opt, stop, output_chains=True)
        cm = _cmapper(oracle, seeds, opt, stop, n, output_chains=True)
        got, _ = mapper.map_reads_c(seeds, list(range(n)), cm)
        assert got == want
        mapped = [line for line in got if line.split("\t")[2] != "*"]
        assert mapped and all(line.split("\t")[-1].startswith("anchors:s:(") for line in mapped)
        assert not any("anchors:s:" in line for line in got if line.split("\t")[2] == "*")
        plain, _ = mapper.map_reads(seeds, list(range(n)), OracleScorer(oracle, _ref()), opt, stop)
        assert [line.split("\tanchors:s:")[0] for line in got] == plain
        cm.close()
