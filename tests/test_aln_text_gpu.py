"""The aln text on the device (include/rawdtw.h, "aln text"; rawalign_amd/csrc/rawdtw_aln_text.hip).
1. rawdtw_aln_text_steps -- the kernels alone -- against rawdtw_aln_text_host, byte for byte: the CPU test's lattice of float bit patterns
   as distances in one call, the path-length and digit-transition cases, 1 / 255 / 256 / 257 jobs with empty jobs between full ones,
   canaries behind text and text_off.
2. rawdtw_traceback_batch_text / _arena_text against rawdtw_traceback_batch_steps + rawdtw_aln_text_host in the same context: every shape
   of [1, 40]^2 and a few jobs of 400 x 3 000 in one call, exclude_last 0 and 1, both modes, uncut and cut into sub-batches; the refusals
   of the steps form with the out arrays untouched.
3. The mapper with rawdtw_mapper_set_device_text: the cigar option sets against the reference's recorded lines and tag by tag against the
   same mapper with the setter off -- sparse and global + full, from host events and from the arena under "signal_cigar"; a banded-cigar
   mapper and a local mapper do not change."""
import ctypes as C

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from rawalign_amd import mapper
from rawalign_amd.dtw import JOB_DTYPE
from rawalign_amd.mapping import StopOpt
from tests import aln_text_cases as A
from tests import map_ref_cases as K
from tests.test_map_ref import check_lines_default_stop, parse
from tests.util import make_arena_jobs

pytestmark = pytest.mark.gpu
INVALID, RANGE = 1, 4
CANARY = 0xA5


def vp(a):
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def eng():
    e = ra.Engine(0)
    yield e
    e.close()


def steps_with_canaries(e, step, d, off, plen, recs, cap):
    """rawdtw_aln_text_steps into buffers with 64 canary bytes (8 canary offsets) behind what the call may write -> (status, text_off, text, bytes)"""
    n = len(plen)
    toff = np.full(n + 1 + 8, 0xA5A5A5A5A5A5A5A5, np.uint64)
    text = np.full(cap + 64, CANARY, np.uint8)
    nb = C.c_uint64(0)
    recs = np.ascontiguousarray(recs, ra.ALN_REC_DTYPE)
    st = e.lib.rawdtw_aln_text_steps(e._ctx, vp(step), vp(d), vp(np.ascontiguousarray(off, np.uint64)), vp(np.ascontiguousarray(plen, np.uint32)), vp(recs), n,
                                     vp(toff), vp(text), cap, C.byref(nb))
    assert np.all(toff[n + 1:] == 0xA5A5A5A5A5A5A5A5) and np.all(text[cap:] == CANARY)
    return st, toff[:n + 1], text, nb.value


def check_steps(e, step, d, off, plen, recs, what):
    want_off, want = ra.aln_text_host(step, d, off, plen, recs)
    total = len(want)
    st, toff, text, nb = steps_with_canaries(e, step, d, off, plen, recs, total + 32)
    assert st == 0 and nb == total and np.array_equal(toff, want_off), what
    assert np.array_equal(text[:total], want), what
    assert np.all(text[total:] == CANARY), what                                   # nothing behind the text, inside the cap either
    st, toff, text, nb = steps_with_canaries(e, step, d, off, plen, recs, total)   # the exact cap
    assert st == 0 and np.array_equal(text[:total], want), what
    toff2, none = e.aln_text(step, d, off, plen, recs, sizes_only=True)
    assert none is None and np.array_equal(toff2, want_off), what
    if total:
        st, toff, text, nb = steps_with_canaries(e, step, d, off, plen, recs, total - 1)
        assert st == RANGE and nb == total and np.array_equal(toff, want_off) and np.all(text == CANARY), what
    return total


def test_the_value_lattice_as_distances_in_one_call(eng):
    v = A.value_lattice()
    rng = np.random.default_rng(A.SEED + 2)
    lens = []
    left = len(v)
    while left:   # jobs of 1 .. 9 000 elements until the lattice is used up: every value is some job's distance
        lens.append(min(left, int(rng.integers(1, 9000))))
        left -= lens[-1]
    step, d, off, plen = A.random_paths(lens, rng, values=v)
    assert len(d) == len(v) and np.array_equal(d.view(np.uint32), v)
    recs = np.zeros(len(lens), ra.ALN_REC_DTYPE)
    recs["off_i"], recs["off_j"], recs["mode"] = rng.integers(0, 5000, len(lens)), rng.integers(0, 1 << 33, len(lens)), rng.integers(0, 2, len(lens))
    want_off, want = ra.aln_text_host(step, d, off, plen, recs)
    toff, text = eng.aln_text(step, d, off, plen, recs, cap=len(want))
    assert np.array_equal(toff, want_off) and len(text) == len(want)
    bad = np.nonzero(text != want)[0]
    assert len(bad) == 0, (len(bad), int(bad[0]), bytes(want[max(0, int(bad[0]) - 40):int(bad[0]) + 40]), bytes(text[max(0, int(bad[0]) - 40):int(bad[0]) + 40]))
    tm = eng.aln_text_timing()
    print("lattice: %d values, %d bytes, count %.2f ms, write %.2f ms" % (len(v), len(want), tm["count_ms"], tm["write_ms"]))
    assert tm["text_bytes"] == len(want) and tm["count_ms"] > 0 and tm["write_ms"] > 0


def test_the_edge_paths(eng):
    step, d, off, plen, recs = A.edge_paths()
    assert check_steps(eng, step, d, off, plen, recs, "edge paths") > 100_000
    # ... and with the paths at other, gapped places of the arrays (path_off is the caller's): the same text
    gap = np.concatenate([[3], np.cumsum(plen.astype(np.uint64) + 5)[:-1] + 3]).astype(np.uint64)
    step2, d2 = np.full(int(gap[-1]) + int(plen[-1]) + 9, 3, np.uint8), np.full(int(gap[-1]) + int(plen[-1]) + 9, 7.5, np.float32)
    for k in range(len(plen)):
        step2[int(gap[k]):int(gap[k]) + int(plen[k])] = step[int(off[k]):int(off[k]) + int(plen[k])]
        d2[int(gap[k]):int(gap[k]) + int(plen[k])] = d[int(off[k]):int(off[k]) + int(plen[k])]
    want_off, want = ra.aln_text_host(step, d, off, plen, recs)
    toff, text = eng.aln_text(step2, d2, gap, plen, recs)
    assert np.array_equal(toff, want_off) and np.array_equal(text, want)


@pytest.mark.parametrize("n_jobs", [1, 255, 256, 257, 1030])
def test_job_counts_around_the_scan_block_with_empty_jobs_between(eng, n_jobs):
    rng = np.random.default_rng(n_jobs)
    lens = rng.integers(1, 200, n_jobs)
    if n_jobs > 1:
        lens[rng.integers(0, n_jobs, n_jobs // 3)] = 0
        lens[[0, n_jobs - 1]] = 0, 70   # an empty first job, a full last one
        lens[n_jobs // 2:n_jobs // 2 + 3] = 0
    step, d, off, plen = A.random_paths(lens, rng)
    recs = np.zeros(n_jobs, ra.ALN_REC_DTYPE)
    recs["off_i"], recs["off_j"], recs["j0"], recs["mode"] = rng.integers(0, 1 << 20, n_jobs), rng.integers(0, 1 << 40, n_jobs), rng.integers(0, 9, n_jobs), rng.integers(0, 2, n_jobs)
    check_steps(eng, step, d, off, plen, recs, n_jobs)


def test_no_job_and_bad_arguments(eng):
    toff, text = eng.aln_text(np.zeros(0, np.uint8), np.zeros(0, np.float32), [0], np.zeros(0, np.uint32), np.zeros(0, ra.ALN_REC_DTYPE))
    assert toff.tolist() == [0] and len(text) == 0
    step, d, off, plen = A.random_paths([5], np.random.default_rng(0))
    st, toff, text, nb = steps_with_canaries(eng, step, d, off, plen, A.rec(mode=3), 200)
    assert st == INVALID and np.all(text == CANARY) and np.all(toff == 0xA5A5A5A5A5A5A5A5)
    nbytes = C.c_uint64(0)
    assert eng.lib.rawdtw_aln_text_steps(eng._ctx, None, vp(d), vp(off), vp(plen), vp(A.rec()), 1, vp(toff), vp(text), 200, C.byref(nbytes)) == INVALID
    assert eng.lib.rawdtw_aln_text_steps(eng._ctx, vp(step), vp(d), vp(off), vp(plen), vp(A.rec()), 1, None, vp(text), 200, C.byref(nbytes)) == INVALID


# ---- 2. the traceback's text form ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tb():
    """every shape of [1, 40]^2 and four jobs of 400 x 3 000 (one the other way round), exclude_last and the mode alternating, offsets that
    push i and j over digit counts.  -> (engine, jobs, events, recs, the steps form's (cost, off, plen, step, dist) in one sub-batch)"""
    rng = np.random.default_rng(A.SEED + 3)
    shapes = [(n, m) for n in range(1, 41) for m in range(1, 41)]
    for at, s in ((100, (400, 3000)), (700, (3000, 400)), (1300, (400, 3000)), (len(shapes), (400, 3000))):
        shapes.insert(at, s)
    cases = [(rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32), -1, (k // 2) % 2 == 1) for k, (n, m) in enumerate(shapes)]
    jobs, ev, rf = make_arena_jobs(cases)
    e = ra.Engine(0)
    e.upload_reference([rf], [rf])
    jobs["ref_off"] += e.reference_offset(0, 1)
    recs = np.zeros(len(jobs), ra.ALN_REC_DTYPE)
    recs["mode"] = np.arange(len(jobs)) % 2
    recs["off_i"], recs["off_j"] = rng.integers(0, 3000, len(jobs)), rng.integers(0, 1 << 27, len(jobs))
    recs["off_j"][::7] = (1 << 32) - 20
    caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
    off = np.concatenate([[0], np.cumsum(caps)]).astype(np.uint64)
    cost, plen = np.zeros(len(jobs), np.float32), np.zeros(len(jobs), np.uint32)
    step, dist = np.zeros(int(off[-1]) + 1, np.uint8), np.zeros(int(off[-1]) + 1, np.float32)
    e._check(e.lib.rawdtw_traceback_batch_steps(e._ctx, vp(jobs), len(jobs), vp(ev), len(ev), vp(cost), vp(off), vp(plen), vp(step), vp(dist)))
    assert e.get_option("tb_sub_batches") == 1
    want_off, want = ra.aln_text_host(step, dist, off, plen, recs)
    for x in (cost, plen, want_off, want):
        x.setflags(write=False)
    yield e, jobs, ev, recs, cost, plen, want_off, want
    e.close()


def check_tb(got, tb, what):
    _, jobs, _, _, cost, plen, want_off, want = tb
    gc, gl, goff, gtext = got
    assert np.array_equal(gc.view(np.uint32), cost.view(np.uint32)) and np.array_equal(gl, plen), what
    assert np.array_equal(goff, want_off), what
    assert len(gtext) == len(want) and np.array_equal(gtext, want), what


def test_traceback_text_equals_steps_plus_host_text(tb):
    e, jobs, ev, recs = tb[:4]
    assert set(jobs["exclude_last"].tolist()) == {0, 1} and set(recs["mode"].tolist()) == {0, 1}
    assert np.any((jobs["exclude_last"] == 1) & (recs["mode"] == 0)) and np.any((jobs["exclude_last"] == 1) & (recs["mode"] == 1))
    check_tb(e.traceback_text(jobs, recs, ev), tb, "batch form")
    assert e.get_option("tb_sub_batches") == 1
    tm = e.aln_text_timing()
    assert tm["text_bytes"] == len(tb[7]) and tm["count_ms"] > 0 and tm["write_ms"] > 0
    # the exact cap, and the arena form over the arena the call before left
    check_tb(e.traceback_text(jobs, recs, ev, cap=len(tb[7])), tb, "batch form, exact cap")
    check_tb(e.traceback_text(jobs, recs), tb, "arena form")
    cost, plen, toff, none = e.traceback_text(jobs, recs, ev, sizes_only=True)
    assert none is None and np.array_equal(toff, tb[6]) and np.array_equal(plen, tb[5])
    assert ra.aln_text_bound(jobs, recs) >= len(tb[7])


def test_the_text_does_not_depend_on_the_cut(tb):
    e, jobs, ev, recs = tb[:4]
    try:
        e.set_option("tb_workspace_mb", 1)
        check_tb(e.traceback_text(jobs, recs, ev), tb, "cut, batch form")
        assert e.get_option("tb_sub_batches") > 2
        check_tb(e.traceback_text(jobs, recs), tb, "cut, arena form")
        assert e.get_option("tb_sub_batches") > 2
        check_tb(e.traceback_text(jobs, recs, ev, cap=len(tb[7])), tb, "cut, exact cap")
        # a cap one byte short: sizes, costs and lengths are filled, the status says so
        n = len(jobs)
        cost, plen, toff, text = np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), np.full(len(tb[7]) + 64, CANARY, np.uint8)
        nb = C.c_uint64(0)
        st = e.lib.rawdtw_traceback_batch_text(e._ctx, vp(jobs), n, vp(ev), len(ev), vp(recs), vp(cost), vp(plen), vp(toff), vp(text), len(tb[7]) - 1, C.byref(nb))
        assert st == RANGE and nb.value == len(tb[7]) and np.array_equal(toff, tb[6]) and np.array_equal(plen, tb[5])
        assert np.all(text[len(tb[7]) - 1:] == CANARY)
    finally:
        e.set_option("tb_workspace_mb", 0)


def test_the_refusals_of_the_steps_form_leave_the_out_arrays_untouched(tb):
    e, jobs, ev, recs = tb[:4]
    lib = e.lib
    few = np.ascontiguousarray(jobs[:6].copy(), JOB_DTYPE)
    r6 = np.ascontiguousarray(recs[:6].copy())
    cost, plen, toff, text = np.full(6, 7.0, np.float32), np.full(6, 77, np.uint32), np.full(7, 777, np.uint64), np.full(4096, CANARY, np.uint8)
    nb = C.c_uint64(12345)

    def untouched():
        return np.all(cost == 7.0) and np.all(plen == 77) and np.all(toff == 777) and np.all(text == CANARY) and nb.value == 12345

    def batch(j, ctx=e._ctx, r=r6, c=cost, pl=plen, to=toff, b=C.byref(nb), events=ev):
        return lib.rawdtw_traceback_batch_text(ctx, vp(j), len(j), vp(events), len(events), None if r is None else vp(r), None if c is None else vp(c),
                                               None if pl is None else vp(pl), None if to is None else vp(to), vp(text), len(text), b)

    assert batch(few, ctx=None) == INVALID and untouched()
    for kw in (dict(r=None), dict(c=None), dict(pl=None), dict(to=None), dict(b=None)):
        assert batch(few, **kw) == INVALID and untouched(), kw
    assert "null" in lib.rawdtw_last_error(e._ctx).decode()
    bad = r6.copy()
    bad["mode"][3] = 2
    assert batch(few, r=bad) == INVALID and untouched()
    zero = few.copy()
    zero["n"][2] = 0
    assert batch(zero) == INVALID and untouched()
    banded = few.copy()
    banded["band_radius"][1] = 5
    st_steps = e.lib.rawdtw_traceback_batch_steps(e._ctx, vp(banded), 6, vp(ev), len(ev), vp(np.zeros(6, np.float32)), vp(np.arange(7, dtype=np.uint64) * 100),
                                                  vp(np.zeros(6, np.uint32)), vp(np.zeros(700, np.uint8)), vp(np.zeros(700, np.float32)))
    assert st_steps != 0 and batch(banded) == st_steps and untouched()
    far = few.copy()
    far["read_off"][4] = len(ev)
    st_steps = e.lib.rawdtw_traceback_batch_steps(e._ctx, vp(far), 6, vp(ev), len(ev), vp(np.zeros(6, np.float32)), vp(np.arange(7, dtype=np.uint64) * 100),
                                                  vp(np.zeros(6, np.uint32)), vp(np.zeros(700, np.uint8)), vp(np.zeros(700, np.float32)))
    assert st_steps != 0 and batch(far) == st_steps and untouched()
    # the arena form: a job beyond the arena, a context without one
    e.upload_events(ev)
    assert lib.rawdtw_traceback_arena_text(e._ctx, vp(far), 6, vp(r6), vp(cost), vp(plen), vp(toff), vp(text), len(text), C.byref(nb)) == INVALID and untouched()
    assert "arena" in lib.rawdtw_last_error(e._ctx).decode()
    bare = ra.Engine(0)
    try:
        assert lib.rawdtw_traceback_arena_text(bare._ctx, vp(few), 6, vp(r6), vp(cost), vp(plen), vp(toff), vp(text), len(text), C.byref(nb)) == INVALID and untouched()
    finally:
        bare.close()
    # ... and the call still goes through afterwards
    c2, p2, t2, x2 = e.traceback_text(few, r6, ev)
    assert np.array_equal(t2, tb[6][:7]) and np.array_equal(x2, tb[7][:int(tb[6][6])])


# ---- 3. the mapper ------------------------------------------------------------------------------------------------------------------------
def aln_tags(line):
    _, mapped, tags = parse(line)
    return (tags.get("alns"), tags.get("aln")) if mapped else (None, None)


def rounds_mapper_lines(fx, engine, opt, copt, device_text, banded_cigar=False, **kw):
    cm = mapper.CMapper(engine, opt, StopOpt(), ["seq%d" % s for s in range(len(fx.lens))], [int(x) for x in fx.lens], slot_events=2048,
                        max_reads=fx.n_reads, chain_opt=copt, output_chains=True, threads=3, carry=False, device_chain=True, **kw)
    lines, _ = mapper.map_reads_c(fx, list(range(fx.n_reads)), cm, device_text=device_text, banded_cigar=banded_cigar)
    cm.close()
    return lines


@pytest.fixture(scope="module")
def fx():
    return K.Fixture()


@pytest.fixture(scope="module")
def meng(fx):
    e = ra.Engine(0)
    e.upload_reference(fx.ref.forward, fx.ref.reverse)
    yield e
    e.close()


def same_tags(on, off, what, at_least):
    assert len(on) == len(off)
    n = 0
    for r, (a, b) in enumerate(zip(on, off)):
        fa, ma, ta = parse(a)
        fb, mb, tb_ = parse(b)
        assert fa[:12] == fb[:12] and ma == mb and list(ta) == list(tb_), (what, r)
        for k in ta:
            assert ta[k] == tb_[k], (what, r, k)
        n += int("aln" in ta and ta["aln"].startswith("("))
    assert on == off and n >= at_least, (what, n)


@pytest.mark.parametrize("form", K.FORMS)
def test_sparse_cigar_mapper_against_the_reference_and_the_setter_off(fx, meng, form):
    opt, copt = K.project_opts("cigar", form)
    lines = {on: rounds_mapper_lines(fx, meng, opt, copt, on, groups=1 + form) for on in (True, False)}
    n = check_lines_default_stop(fx, "cigar", form, lines[True], "device text")   # alns:f: and the element count of aln:s: as the reference recorded them
    assert n >= fx.n_reads // 2
    same_tags(lines[True], lines[False], ("sparse", form), n)


@pytest.mark.parametrize("form", K.FORMS)
def test_global_full_cigar_mapper_equals_the_setter_off(fx, meng, form):
    """mode 0: the global branch's quirk -- only a path's last element moved, by len times the chain's start anchor"""
    opt, copt = K.project_opts("global_full", form)
    opt.flag |= K.CIGAR
    lines = {on: rounds_mapper_lines(fx, meng, opt, copt, on) for on in (True, False)}
    same_tags(lines[True], lines[False], ("global + full", form), fx.n_reads // 2)
    first = next(parse(ln)[2]["aln"] for ln in lines[True] if parse(ln)[1])
    assert first.startswith("(0,0,")


@pytest.mark.parametrize("form", K.FORMS)
def test_whole_reads_with_device_text_are_what_the_reference_printed(meng, form):
    """tests/golden/map_ref_reads.npz holds the reference's own aln:s: text: every line whole"""
    wr = K.WholeReads(form)
    opt, copt = K.whole_project_opts("cigar", form)
    want = [wr.expected_line("cigar", r) for r in range(wr.n_reads)]
    for dev, groups in ((True, 1), (False, 2)):
        cm = mapper.CMapper(meng, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096,
                            max_reads=wr.n_reads, chain_opt=copt, output_chains=True, threads=3, groups=groups, carry=False, device_chain=dev)
        got, _ = mapper.map_reads_c(wr, list(range(wr.n_reads)), cm, device_text=True)
        cm.close()
        for r, (g, w) in enumerate(zip(got, want)):
            assert g == w, (form, dev, groups, r)
    assert sum("\taln:s:(" in ln for ln in want) >= 3


@pytest.mark.parametrize("name,form", [("cigar", 0), ("cigar", 1), ("global_full", 1)])
def test_from_the_arena_under_signal_cigar(name, form):
    """rounds from signal with "signal_cigar" on: the finish takes rawdtw_traceback_arena_text; the lines are the recorded ones (sparse) and
    those of the setter off"""
    from rawalign_amd.seeding import SeedIndex
    from tests.test_signal_round_gpu import _Signal

    ref = K.make_reference()
    six = SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)
    raws = K.make_raw_reads()
    wr = K.WholeReads(form, ref=ref)
    opt, copt = K.whole_project_opts(name, form)
    opt.flag |= K.CIGAR
    lines = {}
    for on in (True, False):
        e = ra.Engine(0)
        try:
            e.upload_reference(ref.forward, ref.reverse)
            e.set_option("signal_cigar", 1)
            cm = mapper.CMapper(e, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096,
                                max_reads=wr.n_reads, chain_opt=copt, output_chains=True, threads=3, carry=False, groups=1, device_chain=True)
            lines[on], _ = mapper.map_reads_c(_Signal(wr, raws), list(range(wr.n_reads)), cm, seed_index=six, signal=True,
                                              event_opt=ra.EventOptions(contracted=bool(form)), device_text=on)
            assert cm.signal_stats()["event_bytes_crossed"] == 0 and cm.timing()["event_bytes"] == 0
            cm.close()
        finally:
            e.close()
    same_tags(lines[True], lines[False], (name, form, "arena"), 3)
    if name == "cigar":
        assert lines[True] == [wr.expected_line("cigar", r) for r in range(wr.n_reads)]


def test_a_banded_cigar_mapper_and_a_local_mapper_do_not_change(fx, meng):
    opt, copt = K.project_opts("global_banded", 1)
    opt.flag |= K.CIGAR
    lines = {on: rounds_mapper_lines(fx, meng, opt, copt, on, banded_cigar=True) for on in (True, False)}
    same_tags(lines[True], lines[False], "banded cigar", 3)
    e = ra.Engine(0)
    try:
        e.upload_reference(fx.ref.forward, fx.ref.reverse)
        e.set_border_local(True)
        wr = K.WholeReads(0)
        opt, copt = K.whole_project_opts("cigar", 0)
        opt.dtw_border_constraint = 2
        lines = {}
        for on in (True, False):
            cm = mapper.CMapper(e, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096,
                                max_reads=wr.n_reads, chain_opt=copt, output_chains=True, threads=3, carry=False, device_chain=True)
            lines[on], _ = mapper.map_reads_c(wr, list(range(wr.n_reads)), cm, device_text=on)
            cm.close()
        same_tags(lines[True], lines[False], "local", 3)
    finally:
        e.close()
