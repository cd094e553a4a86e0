"""The banded global traceback on the device (include/rawdtw.h, "banded traceback": rawdtw_banded_traceback_steps,
rawdtw_dtw_global_banded_tb, rawdtw_mapper_set_banded_cigar; kernels: rawdtw_band_tb.hip), bit for bit throughout: costs, lengths, step
bytes, distances.

The yardstick is the library's host restatement (rawdtw_banded_tb_host, which tests/test_banded_tb_cpu.py holds to the numpy model of the
definition, to the oracle and to the compiled reference); small shapes are also held to the numpy model, costs to the oracle's banded
cost, and a band that holds the whole matrix to the oracle's DTW_global_tb."""
import ctypes as C

import numpy as np
import pytest

try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

import rawalign_amd as ra
from oracle.loader import Oracle, OrcOpt
from rawalign_amd.dtw import JOB_DTYPE
from tests import banded_tb_cases as bc
from tests import value_cases as vc
from tests.util import make_arena_jobs

pytestmark = pytest.mark.gpu
INVALID, RANGE, UNSUPPORTED = 1, 4, 5
STEP_CANARY, D_CANARY = 0xAB, np.float32(-777.25)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def engine_for(cases, **options):
    """cases: [(a, b, R, exclude_last)] -> (engine, jobs, events): every b in the engine's reference arena, every a in `events`"""
    jobs, ev, rf = make_arena_jobs(cases)
    eng = ra.Engine(0)
    for name, value in options.items():
        eng.set_option(name, value)
    eng.upload_reference([rf], [rf])
    jobs["ref_off"] += eng.reference_offset(0, 1)
    return eng, jobs, ev


def host_answers(cases):
    return [ra.banded_tb_host(a, b, R, ex) for a, b, R, ex in cases]


def check(cases, want, tb, what):
    cost, off, plen, step, pd = tb
    for k, ((a, b, R, ex), r) in enumerate(zip(cases, want)):
        key = (what, k, len(a), len(b), R, ex)
        s, ln = int(off[k]), int(plen[k])
        assert bc.bits(cost[k])[0] == bc.bits(r.cost)[0], key + (cost[k], r.cost)
        assert ln == len(r.i), key + (ln, len(r.i))
        if ln == 0:
            continue
        assert step[s] == 0, key
        i, j = ra.expand_steps(step[s:s + ln])
        assert np.array_equal(i, r.i) and np.array_equal(j, r.j), key
        assert np.array_equal(bc.bits(pd[s:s + ln]), bc.bits(r.difference)), key


def test_grid(orc):
    """one call of every (n, m) in [1, 40]^2 x R in {0, 1, 2, 3, 5, n + m}, normal and three-valued signals"""
    grid = bc.grid_cases(bc.PLAIN, 40, radii=bc.RADII + (None,))
    cases = [(a, b, R, q & 1) for q, (a, b, R) in enumerate(grid)]
    assert len(cases) == 2 * 1600 * 6
    want = host_answers(cases)
    eng, jobs, ev = engine_for(cases)
    tb = eng.banded_traceback(jobs, ev)
    check(cases, want, tb, "grid")
    assert eng.get_option("tb_sub_batches") == 1
    cost, off, plen, step, pd = tb
    for k, (a, b, R, ex) in enumerate(cases):
        assert bc.bits(cost[k])[0] == bc.bits(orc.dtw_banded(a, b, R, ex))[0], (k, len(a), len(b), R, ex)
        assert plen[k] >= max(len(a), len(b)) - ex   # (below 1e10 every job has a path)
        if R == len(a) + len(b):
            c, pi, pj, pdd = orc.dtw_global_tb(a, b, ex)
            s = int(off[k])
            i, j = ra.expand_steps(step[s:s + int(plen[k])])
            assert bc.bits(cost[k])[0] == bc.bits(c)[0] and np.array_equal(i, pi) and np.array_equal(j, pj), (k, len(a), len(b), ex)
        if k % 16 == 0:
            w = bc.model(orc, a, b, R, ex)
            r = want[k]
            assert bc.bits(r.cost)[0] == bc.bits(w["cost"])[0] and np.array_equal(r.i, w["i"]) and np.array_equal(r.j, w["j"])
    t = eng.banded_traceback_timing()
    assert t["path_elements"] == int(plen.sum()) and t["fill_ms"] > 0 and t["walk_ms"] > 0
    assert t["direction_bytes"] == sum((bc.dir_bytes(len(a), len(b), R) + 255) & ~255 for a, b, R, ex in cases)
    eng.close()


def test_band_widths_around_the_kernels_bounds():
    """48 x 48: the band's width is set by R alone -- K = R + 1 on both sides of the fill kernel's class and chunk bounds and at the limit"""
    rng = np.random.default_rng(4848)
    cases = []
    for q, R in enumerate(bc.boundary_radii()):
        draw = bc.PLAIN["normal" if q & 1 else "three"]
        cases.append((draw(rng, 48), draw(rng, 48), R, (q >> 1) & 1))
    assert max(R for _, _, R, _ in cases) + 1 == bc.MAX_K
    eng, jobs, ev = engine_for(cases)
    check(cases, host_answers(cases), eng.banded_traceback(jobs, ev), "widths")
    eng.close()


def test_shapes():
    """3 000 x 3 000 at 300; 3 000 x 2 049 at 300 and its transpose (slant and swap); a row and a column; pure diagonals of 64, 65 and 128
    elements (the walk's flush residues 0, 1 and 63 with exclude_last)"""
    rng = np.random.default_rng(3000)
    shapes = [(3000, 3000, 300), (3000, 2049, 300), (2049, 3000, 300), (1, 65, 3), (65, 1, 3)]
    cases = []
    for n, m, R in shapes:
        a = rng.normal(size=n).astype(np.float32)
        b = (np.interp(np.linspace(0, n - 1, m), np.arange(n), a) + rng.normal(0, 0.2, m)).astype(np.float32)
        cases += [(a, b, R, 0), (a, b, R, 1)]
    for n in (64, 65, 128):
        a = np.arange(n, dtype=np.float32) * 3
        cases += [(a, a.copy(), 2, 0), (a, a.copy(), 2, 1)]
    want = host_answers(cases)
    for (a, b, R, ex), r in zip(cases[-6:], want[-6:]):
        assert len(r.i) == len(a) - ex and np.array_equal(r.i, r.j)   # (the construction did what it says)
    eng, jobs, ev = engine_for(cases)
    check(cases, want, eng.banded_traceback(jobs, ev), "shapes")
    for a, b, R, ex in (cases[0], cases[3], cases[5], cases[7], cases[-1]):  # the single-call drop-in
        r, w = eng.DTW_global_banded_tb(a, b, R, ex), ra.banded_tb_host(a, b, R, ex)
        assert bc.bits(r.cost)[0] == bc.bits(w.cost)[0] and np.array_equal(r.i, w.i) and np.array_equal(r.j, w.j)
        assert np.array_equal(bc.bits(r.difference), bc.bits(w.difference))
    eng.close()


def canaried(jobs, off=None):
    caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
    total = int(caps.sum()) if off is None else int((off[:len(jobs)] + caps).max())
    return (np.full(len(jobs), D_CANARY, np.float32), np.full(len(jobs), 0xDEADBEEF, np.uint32), np.full(max(total, 1), STEP_CANARY, np.uint8),
            np.full(max(total, 1), D_CANARY, np.float32))


def untouched(out):
    cost, plen, step, pd = out
    return (bc.bits(cost) == bc.bits(D_CANARY)[0]).all() and (plen == 0xDEADBEEF).all() and (step == STEP_CANARY).all() and \
        (bc.bits(pd) == bc.bits(D_CANARY)[0]).all()


def test_value_domains(orc):
    """every domain of tests/value_cases.py at the mapper's radius and at 2: costs are the oracle's; the jobs without a path have
    path_len 0 and nothing written into their stretches"""
    cases = []
    for name in vc.DOMAIN_NAMES:
        for q, (a, b, ex) in enumerate(vc.fixture_cases(name)):
            cases.append((a, b, vc.fixture_radii(len(a))[0] if q % 3 else 2, ex))
    want = host_answers(cases)
    eng, jobs, ev = engine_for(cases)
    out = canaried(jobs)
    cost, off, plen, step, pd = eng.banded_traceback(jobs, ev, out=out)
    check(cases, want, (cost, off, plen, step, pd), "domains")
    none = 0
    for k, (a, b, R, ex) in enumerate(cases):
        assert bc.bits(cost[k])[0] == bc.bits(orc.dtw_banded(a, b, R, ex))[0], k
        s, e = int(off[k]), int(off[k + 1])
        assert (step[s + int(plen[k]):e] == STEP_CANARY).all() and (bc.bits(pd[s + int(plen[k]):e]) == bc.bits(D_CANARY)[0]).all(), k
        none += plen[k] == 0 and len(a) + len(b) > 2
    print("jobs without a path:", none)
    assert none >= 20
    eng.close()


def mixed_jobs(count, seed):
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(count):
        n = int(rng.integers(1, 420))
        m = max(1, int(n * rng.uniform(0.5, 1.6)))
        R = int(rng.choice([0, 1, 3, 8, 40, 70, 200])) if k % 5 else max(1, n // 10)
        draw = bc.PLAIN["three" if k % 3 == 0 else "normal"]
        cases.append((draw(rng, n), draw(rng, m), R, k & 1))
    return cases


def test_sub_batches_at_1_mib():
    cases = mixed_jobs(120, 120)
    want = host_answers(cases)
    one, jobs, ev = engine_for(cases)
    small, jobs_s, _ = engine_for(cases, tb_workspace_mb=1)
    whole = one.banded_traceback(jobs, ev)
    assert one.get_option("tb_sub_batches") == 1
    check(cases, want, whole, "unsplit")
    # the caller's layout: a gap of 0..6 elements behind every job
    caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
    gaps = (np.arange(len(jobs)) % 7).astype(np.uint64)
    off = np.zeros(len(jobs), np.uint64)
    off[1:] = np.cumsum(caps + gaps)[:-1]
    out = canaried(jobs_s, off)
    cost, off2, plen, step, pd = small.banded_traceback(jobs_s, ev, path_off=off, out=out)
    model = bc.sub_batches(jobs_s, 1)
    assert small.get_option("tb_sub_batches") == len(model) >= 3, (small.get_option("tb_sub_batches"), model)
    assert np.array_equal(bc.bits(cost), bc.bits(whole[0])) and np.array_equal(plen, whole[2])
    for k in range(len(jobs)):
        s, ln, s0 = int(off[k]), int(plen[k]), int(whole[1][k])
        assert np.array_equal(step[s:s + ln], whole[3][s0:s0 + ln]) and np.array_equal(bc.bits(pd[s:s + ln]), bc.bits(whole[4][s0:s0 + ln])), k
        e = int(off[k + 1]) if k + 1 < len(jobs) else len(step)
        assert (step[s + ln:e] == STEP_CANARY).all() and (bc.bits(pd[s + ln:e]) == bc.bits(D_CANARY)[0]).all(), k
    t = small.banded_traceback_timing()
    assert t["direction_bytes"] == one.banded_traceback_timing()["direction_bytes"] and t["path_elements"] == int(plen.sum())
    one.close()
    small.close()


def test_arena_form():
    """events None: the jobs read the event arena as it lies.  The first job lies flush against the start of both arenas, the last
    against their ends: the reference arena is the forward strand at offset 0 and the reverse strand behind it (each a multiple of four
    floats long here, so nothing pads it), and the second half of the jobs reads the reverse strand"""
    cases = mixed_jobs(40, 41)
    pad = -sum(len(b) for _, b, _, _ in cases) % 4
    a, b, R, ex = cases[-1]
    cases[-1] = (a, np.concatenate([b, b[:pad]]), R, ex)   # (the last window a little longer: the strand ends on a multiple of four)
    want = host_answers(cases)
    jobs, ev, rf = make_arena_jobs(cases)
    assert len(rf) % 4 == 0
    eng = ra.Engine(0)
    eng.upload_reference([rf], [rf])
    assert eng.reference_offset(0, 1) == 0 and eng.reference_offset(0, 0) == len(rf)
    jobs["ref_off"][20:] += len(rf)
    assert jobs[0]["read_off"] == 0 and int(jobs[-1]["read_off"]) + int(jobs[-1]["n"]) == len(ev)
    assert jobs[0]["ref_off"] == 0 and int(jobs[-1]["ref_off"]) + int(jobs[-1]["m"]) == 2 * len(rf)
    eng.upload_events(ev)
    check(cases, want, eng.banded_traceback(jobs), "arena form")
    check(cases, want, eng.banded_traceback(jobs), "arena form, again")
    for field in ("n", "m"):   # one element more on either side is outside: the ends are the arenas' ends
        over = jobs.copy()
        over[field][-1] += 1
        with pytest.raises(ra.RawDTWError) as err:
            eng.banded_traceback(over)
        assert err.value.status == RANGE, field
    check(cases, want, eng.banded_traceback(jobs, ev), "h_events form behind it")
    eng.close()


def test_refusals():
    cases = mixed_jobs(12, 7)
    want = host_answers(cases)
    eng, jobs, ev = engine_for(cases)
    changes = [("n", 0, INVALID), ("m", 0, INVALID), ("band_radius", -1, INVALID), ("band_radius", -2, INVALID),
               ("read_off", len(ev), RANGE), ("read_off", len(ev) - int(jobs[5]["n"]) + 1, RANGE), ("m", 1 << 30, RANGE), ("ref_off", 1 << 40, RANGE),
               ("band_radius", bc.MAX_K, UNSUPPORTED)]
    for field, value, status in changes:
        bad = jobs.copy()
        bad[field][5] = value
        out = canaried(jobs)   # (sized for the good jobs: a refusal writes nothing)
        with pytest.raises(ra.RawDTWError) as err:
            eng.banded_traceback(bad, ev, path_off=np.zeros(len(jobs), np.uint64), out=out)
        assert err.value.status == status, (field, value, err.value)
        assert untouched(out), (field, value)
        check(cases, want, eng.banded_traceback(jobs, ev), "after %s = %r" % (field, value))  # a good call on the same context
    assert "too large for the LDS-resident band kernel" in str(err.value)
    # a null argument
    out = canaried(jobs)
    off = np.zeros(len(jobs) + 1, np.uint64)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    for null in range(5):
        args = [vp(out[0]), vp(off), vp(out[1]), vp(out[2]), vp(out[3])]
        args[null] = None
        assert eng.lib.rawdtw_banded_traceback_steps(eng._ctx, vp(jobs), len(jobs), vp(ev), len(ev), *args) == INVALID
    assert eng.lib.rawdtw_banded_traceback_steps(eng._ctx, None, len(jobs), vp(ev), len(ev), vp(out[0]), vp(off), vp(out[1]), vp(out[2]), vp(out[3])) == INVALID
    assert untouched(out)
    # no job: RAWDTW_OK, nothing touched
    assert eng.lib.rawdtw_banded_traceback_steps(eng._ctx, None, 0, None, 0, None, None, None, None, None) == 0
    # the global entries keep refusing a banded job, the planner's refusal stays
    np.cumsum(jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1, out=off[1:])
    plen, cost = np.zeros(len(jobs), np.uint32), np.zeros(len(jobs), np.float32)
    step, pd = np.zeros(int(off[-1]) + 1, np.uint8), np.zeros(int(off[-1]) + 1, np.float32)
    assert eng.lib.rawdtw_traceback_batch_steps(eng._ctx, vp(jobs), len(jobs), vp(ev), len(ev), vp(cost), vp(off), vp(plen), vp(step), vp(pd)) == UNSUPPORTED
    check(cases, want, eng.banded_traceback(jobs, ev), "after the refusals")
    eng.close()
    # a missing arena: no reference; no events for the arena form
    bare = ra.Engine(0)
    out = canaried(jobs)
    with pytest.raises(ra.RawDTWError) as err:
        bare.banded_traceback(jobs, ev, out=out)
    assert err.value.status == INVALID and untouched(out)
    bare.close()
    eng, jobs, ev = engine_for(cases)
    with pytest.raises(ra.RawDTWError) as err:
        eng.banded_traceback(jobs, out=out)
    assert err.value.status == INVALID and untouched(out)
    for a, b, R in ((ev[:0], ev[:3], 1), (ev[:3], ev[:0], 1), (ev[:3], ev[:3], -1)):
        with pytest.raises(ra.RawDTWError) as err:
            eng.DTW_global_banded_tb(a, b, R)
        assert err.value.status == INVALID
    check(cases, want, eng.banded_traceback(jobs, ev), "a context that refused the arena form")
    eng.close()


# ---- the mapper: --dtw-output-cigar at global + banded (rawdtw_mapper_set_banded_cigar) ------------------------------------------------
N_READS = 64
GLOBAL_BANDED = dict(dtw_border_constraint=0, dtw_fill_method=1)


@pytest.fixture(scope="module")
def workload():
    from rawalign_amd import mapper, synth

    ref = synth.make_reference([29903], seed=20231005 + 1)
    # 900 events a chunk: a read that maps in its first chunk has a job of about 890 x 700 at radius 89, 76 KB of directions by
    # banded_tb_cases.dir_bytes -- some fifty mapped reads pass 2 MiB, so the finish at "tb_workspace_mb" = 1 takes three sub-batches or more
    return ref, mapper.SyntheticSeeds(ref, N_READS, seed=3, events_per_chunk=900, max_chunks=4)


def run_mapper(workload, opt, banded_cigar, **options):
    """-> (lines, the reads' events as the mapper holds them, tb_sub_batches)"""
    from rawalign_amd import mapper
    from rawalign_amd.mapping import StopOpt

    ref, seeds = workload
    eng = ra.Engine(0)
    try:
        eng.upload_reference(ref.forward, ref.reverse)
        for k, v in options.items():
            eng.set_option(k, v)
        cm = mapper.CMapper(eng, opt, StopOpt(), ["seq0"], [len(ref.forward[0])], slot_events=max(rd["n_ev"] for rd in seeds.reads) + 8,
                            max_reads=N_READS, carry=True, threads=4, groups=1, output_chains=True)
        try:
            lines, _ = mapper.map_reads_c(seeds, list(range(N_READS)), cm, banded_cigar=banded_cigar)
            return lines, [cm.read_events(r) for r in range(N_READS)], eng.get_option("tb_sub_batches")
        finally:
            cm.close()
    finally:
        eng.close()


def strip_tags(line):
    return "\t".join(f for f in line.split("\t") if not f.startswith(("alns:f:", "aln:s:")))


def rebuilt_tags(orc, ref, opt, line, events):
    """alns:f: and aln:s: of a mapped read's line from its anchors:s: tag: the oracle's score-only align_chain and rawdtw_banded_tb_host on
    the job rawdtw_chain_build_jobs(..., cigar = 0) builds, written with the global mode's quirk (rmap.cpp:230-233: only the last tuple moves)"""
    f = line.split("\t")
    tag = [x for x in f if x.startswith("anchors:s:")][0][len("anchors:s:"):]
    anchors = np.array([tuple(int(v) for v in p.split(","))[::-1] for p in tag.strip("()").split(")(")], ra.ANCHOR_DTYPE)  # "(query,target)", end-first
    seq = int(f[5][3:])   # "seq<index>"
    arr = ref.forward[seq] if f[4] == "-" else ref.reverse[seq]   # (strand 1 is written "-" and selects forward_signals, rmap.cpp:183-188)
    s, e = anchors[-1], anchors[0]
    n, m = int(e["query_position"]) - int(s["query_position"]) + 1, int(e["target_position"]) - int(s["target_position"]) + 1
    R = max(1, int(np.float32(n) * np.float32(opt.dtw_band_radius_frac)))
    q0, t0 = int(s["query_position"]), int(s["target_position"])
    r = ra.banded_tb_host(events[q0:q0 + n], arr[t0:t0 + m], R, 0)
    ln = len(r.i)
    aln = "".join("(%d,%d,%g)" % (int(i) + (ln * q0 if k + 1 == ln else 0), int(j) + (ln * t0 if k + 1 == ln else 0), float(d))
                  for k, (i, j, d) in enumerate(zip(r.i, r.j, r.difference)))
    oopt = OrcOpt(0, 1, opt.dtw_band_radius_frac, opt.dtw_match_bonus, opt.dtw_min_score, int(opt.fused_score))
    score = orc.align_chain(anchors, arr, events, oopt, -1e10)
    return "alns:f:%f" % float(score), "aln:s:" + aln, (n, m, R)


@pytest.fixture(scope="module")
def plain_lines(workload):
    """the non-CIGAR mapper at global + banded"""
    return run_mapper(workload, ra.MapOpt(flag=0x2, **GLOBAL_BANDED), False)[0]


def check_cigar_lines(orc, workload, opt, lines, events, plain):
    """-> the mapped reads' jobs (n, m, band_radius) in read order, as the finish builds them"""
    mapped, shapes = 0, []
    for r, (line, base) in enumerate(zip(lines, plain)):
        assert strip_tags(line) == base, r
        if "\tanchors:s:" not in line:
            assert line == base
            continue
        mapped += 1
        alns, aln, shape = rebuilt_tags(orc, workload[0], opt, line, events[r])
        shapes.append(shape)
        f = line.split("\t")
        assert alns in f and aln in f, (r, alns, [x[:60] for x in f if x.startswith("al")])
    assert mapped >= 12
    jobs = np.zeros(len(shapes), JOB_DTYPE)
    jobs["n"], jobs["m"], jobs["band_radius"] = np.array(shapes).T
    return jobs


def test_mapper_setter_off_fails_as_before(workload):
    with pytest.raises(RuntimeError, match="rawdtw_mapper_finish -> 5"):
        run_mapper(workload, ra.MapOpt(flag=0x2 | 0x4, **GLOBAL_BANDED), False)


def test_mapper_banded_cigar(orc, workload, plain_lines):
    opt = ra.MapOpt(flag=0x2 | 0x4, **GLOBAL_BANDED)
    lines, events, subs = run_mapper(workload, opt, True)
    assert subs == 1
    jobs = check_cigar_lines(orc, workload, opt, lines, events, plain_lines)
    small, _, subs = run_mapper(workload, opt, True, tb_workspace_mb=1)
    print("sub-batches of the finish at 1 MiB:", subs, bc.sub_batches(jobs, 1))
    assert subs == len(bc.sub_batches(jobs, 1)) >= 3 and small == lines


class Spiked:
    """the workload's reads with 3e10 in every 50th event of the first mappable read's chunks: its job's sums pass 1e10 at once, the walk leaves the
    band's cells (rawdtw_banded_tb_host says so below) and the read has no path"""
    def __init__(self, seeds):
        self.seeds, self.reads = seeds, seeds.reads
        self.SPIKED = next(r for r, rd in enumerate(seeds.reads) if rd["mappable"])

    def read_job(self, r):
        return self.seeds.read_job(r)

    def chunk(self, r, c):
        ev, hits = self.seeds.chunk(r, c)
        if r == self.SPIKED:
            ev = np.array(ev, np.float32)
            ev[1::50] = 3e10
        return ev, hits


def test_mapper_banded_cigar_of_a_read_without_a_path(orc, workload):
    """a mapped read whose banded job has no path: an empty aln:s:, alns:f: from the cost as ever.  dtw_min_score is lowered so that the
    chain is kept at a cost beyond 1e10."""
    ref, seeds = workload
    spiked = (ref, Spiked(seeds))
    opt = ra.MapOpt(flag=0x2 | 0x4, dtw_min_score=-1e30, **GLOBAL_BANDED)
    plain = run_mapper(spiked, ra.MapOpt(flag=0x2, dtw_min_score=-1e30, **GLOBAL_BANDED), False)[0]
    lines, events, _ = run_mapper(spiked, opt, True)
    check_cigar_lines(orc, spiked, opt, lines, events, plain)
    f = lines[spiked[1].SPIKED].split("\t")
    assert "aln:s:" in f and any(x.startswith("alns:f:-") for x in f), [x[:40] for x in f if x.startswith("al")]
    assert sum("\taln:s:(" in x for x in lines) >= 12


def test_sparse_cigar_mapper_is_untouched_by_the_setter(workload):
    opt = ra.MapOpt(flag=0x2 | 0x4, dtw_border_constraint=1, dtw_fill_method=1)
    off = run_mapper(workload, opt, False)[0]
    on = run_mapper(workload, opt, True)[0]
    assert on == off and sum("\taln:s:(" in x for x in on) >= 12


def test_mapper_banded_cigar_from_the_arena(orc):
    """rounds from signal under "signal_cigar": the finish reads every mapped read's events in its slot of the arena and no event crosses
    the link; every mapped line's tags are rebuilt from rawdtw_banded_tb_host and the oracle on the read's events (rawdtw_mapper_read_events
    fetches them out of the arena), and the lines are those of the same windows fed as host events, whose finish uploads the host's copy"""
    from rawalign_amd import mapper
    from rawalign_amd.mapping import StopOpt
    from rawalign_amd.seeding import SeedIndex
    from tests import map_ref_cases as mc
    from tests import optins_cases as oc
    from tests.test_signal_round_gpu import _Signal

    form = 1
    ref = mc.make_reference()
    six = SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)
    raws = mc.make_raw_reads()
    wr = mc.WholeReads(form, ref=ref)
    opt = ra.MapOpt(flag=mc.EVAL | mc.CIGAR, fused_score=True, **GLOBAL_BANDED)
    copt = mc.whole_project_opts("cigar", form)[1]
    names, lens = ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens]

    def run(src, **kw):
        e = ra.Engine(0)
        try:
            e.upload_reference(ref.forward, ref.reverse)
            if kw.get("signal"):
                e.set_option("signal_cigar", 1)
            cm = mapper.CMapper(e, opt, StopOpt(), names, lens, slot_events=4096, max_reads=wr.n_reads, chain_opt=copt, output_chains=True, threads=3,
                                carry=False, groups=1, device_chain=True)
            got, _ = mapper.map_reads_c(src, list(range(wr.n_reads)), cm, seed_index=six, banded_cigar=True, **kw)
            crossed = cm.signal_stats()["event_bytes_crossed"]
            events = [cm.read_events(r) for r in range(wr.n_reads)]
            cm.close()
            return got, crossed, events
        finally:
            e.close()

    host, _, _ = run(oc.whole_chunks(six, wr, raws, form), resident=True)
    got, crossed, events = run(_Signal(wr, raws), signal=True, event_opt=ra.EventOptions(contracted=bool(form)))
    assert crossed == 0
    mapped = 0
    for r, line in enumerate(got):
        if "\tanchors:s:" not in line:
            assert "\taln:s:" not in line
            continue
        mapped += 1
        alns, aln, _ = rebuilt_tags(orc, ref, opt, line, events[r])
        f = line.split("\t")
        assert alns in f and aln in f and len(aln) > len("aln:s:"), (r, alns, [x[:60] for x in f if x.startswith("al")])
    assert mapped >= 3
    assert got == host
