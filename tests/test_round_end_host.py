"""The batched host restatement of a round's end (rawdtw_round_end_host: gen_primary_chains, comp_mapq, the stop rule for every read
of a round) against the REFERENCE's answers in tests/golden/map_ref_rounds.npz -- every option set, both builds, every (read, round) --
and against per-read calls of the two host functions it is made of; and, from the host alone, what the inputs of
tests/test_round_end_gpu.py are built to show: which reads the device must decline and that they are few.  No device."""
import ctypes as C

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd._lib import ChainRec
from tests import map_ref_cases as K
from tests import round_end_cases as R


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("name", list(K.OPTION_SETS))
def test_fixture_rounds_against_the_reference(name, form):
    rd, want = R.fixture_round(name, form)
    assert rd.n_reads > 100 and int(rd.chain_off[-1]) > rd.n_reads
    out, primary = rd.host()
    R.check_fixture_round(rd, want, out, primary, ("host", name, form))
    assert not R.must_decline(rd, out, primary).any()   # (the device test asserts that nothing of the fixture declines)


def per_read(rd, r):
    """the two host functions on read r, as rawdtw_mapper.cpp's round end calls them: (n_primary, mapq, high, primaries' indices)"""
    lib = ra.load_library()
    recs, score, keep = rd.read(r)
    part = [c for c in range(len(recs)) if not rd.evaluate or keep[c]]
    if not part:
        return 0, 0, False, []
    arr = (ChainRec * len(part))()
    for k, c in enumerate(part):
        x = recs[c]
        arr[k] = ChainRec(x["chaining_score"], score[c], int(x["key"]) >> 1, int(x["start_position"]), int(x["end_position"]), int(x["n_anchors"]), int(x["key"]) & 1, 0, c)
    kept = (C.c_uint32 * len(part))()
    nk = lib.rawdtw_gen_primary_chains(arr, len(part), C.byref(rd.opt), kept)
    prim = (ChainRec * nk)(*[arr[kept[k]] for k in range(nk)])
    high = bool(lib.rawdtw_is_mapped_with_high_confidence(prim, nk, C.byref(rd.opt)))
    return nk, int(prim[0].mapq), high, [int(p.tag) for p in prim]


def check_against_per_read(rd, out, primary, skip):
    for r in range(rd.n_reads):
        if skip[r]:   # (two equal records, a NaN: the sort's result is its own affair)
            continue
        nk, mapq, high, idx = per_read(rd, r)
        c0 = int(rd.chain_off[r])
        assert (int(out[r]["n_primary"]), int(out[r]["mapq"]), int(out[r]["flags"])) == (nk, mapq, int(high)), (r, out[r], nk, mapq, high)
        assert [int(x) for x in primary[c0:c0 + nk]] == idx, r
        assert (primary[c0 + nk:int(rd.chain_off[r + 1])] == R.NO_PRIMARY).all(), r


@pytest.mark.parametrize("case", [c[0] for c in R.random_rounds()])
def test_random_rounds_against_per_read_calls_and_few_reads_decline(case):
    rd = dict(R.random_rounds())[case]
    out, primary = rd.host()
    decl = R.must_decline(rd, out, primary)
    print("%s: %d reads, %d chains, %d must decline" % (case, rd.n_reads, int(rd.chain_off[-1]), int(decl.sum())))
    assert (~decl).sum() >= 0.95 * rd.n_reads
    assert not (out["flags"] & R.ROUND_DECLINED).any()   # the host never declines
    sizes = np.diff(rd.chain_off).astype(np.int64)
    if rd.n_reads >= 63:   # every count is there, empty reads between full ones, and a keep mask that empties a read
        assert set(R.COUNTS) <= set(sizes.tolist()) and (sizes[1:4:2] == 0).all() and sizes[0] == 64 and sizes[2] == 65
        assert (out["n_primary"] >= 2).sum() > rd.n_reads // 8 and len(set(out["mapq"].tolist())) > 5
        assert {0, 1} <= set((out["flags"] & R.ROUND_HIGH).tolist())
        if rd.evaluate:
            assert ((sizes > 0) & (out["n_primary"] == 0)).any()
    check_against_per_read(rd, out, primary, decl & (sizes <= 64))


@pytest.mark.parametrize("group", R.edge_groups())
def test_constructed_edges_are_what_they_say(group):
    rd, es = R.edges_round(group)
    out, primary = rd.host()
    assert not R.must_decline(rd, out, primary).any()
    for r, (name, _, _, _, (n, mapq, high, first)) in enumerate(es):
        o = out[r]
        assert n is None or int(o["n_primary"]) == n, (name, o)
        assert mapq is None or int(o["mapq"]) == mapq, (name, o)
        assert high is None or bool(int(o["flags"]) & R.ROUND_HIGH) == high, (name, o)
        assert first is None or int(primary[int(rd.chain_off[r])]) == first, (name, primary[int(rd.chain_off[r])])
    check_against_per_read(rd, out, primary, np.zeros(rd.n_reads, bool))


@pytest.mark.parametrize("evaluate", (0, 1))
def test_constructed_declines_are_found_from_the_host_alone(evaluate):
    rd = R.declines_round(evaluate)
    out, primary = rd.host()
    decl = R.must_decline(rd, out, primary)
    assert [bool(x) for x in decl] == [n is not None for n in rd.names], list(zip(rd.names, decl))
    assert decl.sum() >= 4


def test_a_read_at_a_time_is_the_fall_back():
    """n_reads = 1 with chain_off + r and out + r, the other arrays as they are: what a caller does with a declined read"""
    lib = ra.load_library()
    rd = dict(R.random_rounds())["n63-eval1-sel2"]
    out, primary = rd.host()
    one, prim = np.zeros(1, ra.ROUND_OUT_DTYPE), np.full(int(rd.chain_off[-1]), 7, np.uint32)
    for r in (0, 2, 9, 62):
        st = lib.rawdtw_round_end_host(C.byref(rd.opt), 1, C.c_void_p(rd.chain_off.ctypes.data + 8 * r), rd.recs.ctypes.data_as(C.c_void_p),
                                       rd.score.ctypes.data_as(C.c_void_p), rd.keep.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p),
                                       prim.ctypes.data_as(C.c_void_p))
        assert st == 0 and one[0] == out[r]
        c0, c1 = int(rd.chain_off[r]), int(rd.chain_off[r + 1])
        assert (prim[c0:c1] == primary[c0:c1]).all()
