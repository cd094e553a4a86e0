"""The inputs of tests/test_chain_decline_gpu.py have the shape its cases rely on -- decided on the host alone.  The round-level case against
rawdtw_chain_decline_host and a plain-Python count of seeds, chains and ties; the mapper-level cases (tests/optins_cases.py's inputs under
the caps of tests/chain_decline_cases.py) from the Python mirror's seed and candidate counts.  Every case has a round with a declined read,
a read with chains that the device chains, and fewer than half of its (read, round) pairs declined: a test cannot pass by declining
everything.  Also the stand-alone program over the append's offsets, plain and under the sanitizers.  Run with -s to see the figures.  No device."""
import os
import subprocess

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapping as M
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex
from tests import chain_decline_cases as dc
from tests import chain_many_cases as cm
from tests import map_ref_cases as mc
from tests import optins_cases as oc
from tests.test_device_chain import host_chains
from tests.test_signal_round_gpu import FLOW_CHUNKS, FLOW_READS, flow  # noqa: F401  (the fixture itself)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")


def plain_count(lib, copt, seeds, seed_cap, max_chains):
    """the reason a read declines for, counted in plain Python from the host restatement's chains in generation order (lists by key)"""
    if len(seeds) > seed_cap:
        return 1
    order = np.lexsort((seeds["query_position"], seeds["target_position"], seeds["key"]))
    s = seeds[order]
    scores, maxs = [], 0.0
    for key in np.unique(s["key"]):
        g = s[s["key"] == key]
        a = np.zeros(len(g), ra.ANCHOR_DTYPE)
        a["target_position"], a["query_position"] = g["target_position"], g["query_position"]
        cs, maxs = M.chain_anchors(a, copt, maxs, int(key) >> 1, int(key) & 1)
        scores += [float(np.float32(c.chaining_score)) for c in cs]
    assert len(scores) == len(host_chains(lib, copt, seeds))
    if max_chains:
        return 2 if len(scores) > max_chains else 0
    first = scores[:32]
    return (2 if len(scores) > 32 else 0) | (4 if len(scores) > 16 and len(set(first)) < len(first) else 0)


def test_the_round_level_case_declines_what_it_says():
    lib, copt = ra.load_library(), M.default_chain_opt(6)
    reads = dc.round_reads()
    assert [len(s) for s in reads[:4]] == [1, dc.SEED_CAP, dc.SEED_CAP + 1, 300] and len(reads) == 10 and len(reads[9]) == 0
    assert len(reads[5]) <= dc.SEED_CAP and len(reads[7]) <= dc.SEED_CAP
    for many in (0, dc.MANY):
        why, n_chains = ra.chain_decline_host(copt, reads, dc.SEED_CAP, 0, many)
        print(many, why.tolist(), n_chains.tolist())
        assert why.tolist() == [plain_count(lib, copt, s, dc.SEED_CAP, many) for s in reads]
        assert {r: int(w) for r, w in enumerate(why) if w} == dc.DECLINED[many]
        assert (n_chains[5], n_chains[7]) == (33, 17) and len({len(np.unique(reads[5]["key"])), 33}) == 1
        assert 0 < np.count_nonzero(why) < len(reads) / 2
        assert sum(1 for r in range(10) if not why[r] and n_chains[r]) >= 3
    sc = sorted(float(c[0]) for c in host_chains(lib, copt, reads[7]))
    assert len(sc) == 17 and len(set(sc)) == 16   # (two of the 17 chains with exactly equal scores)
    for name, idx in dc.orders().items():
        why, _ = ra.chain_decline_host(copt, [reads[i] for i in idx], dc.SEED_CAP, 0, 0)
        assert sorted(idx) == list(range(10)) and (why[0] != 0) == (name == "rotated") and (why[-1] != 0) == (name == "reversed")
        assert any(why[k] and why[k + 1] for k in range(9))   # (two declined reads adjacent)
    # with the long path on a read between the caps is chained; the default cap is the device's own 2 048
    assert ra.chain_decline_host(copt, reads, dc.SEED_CAP, 200, 0)[0].tolist() == [0, 0, 0, 1, 0, 6, 0, 4, 0, 0]
    assert ra.chain_decline_host(copt, reads, 0, 0, 0)[0].tolist() == [0, 0, 0, 0, 0, 6, 0, 4, 0, 0]
    for per_read, want in ((dc.all_above(), 1), (dc.none_above(), 0)):
        why, _ = ra.chain_decline_host(copt, per_read, dc.SEED_CAP, 0, 0)
        assert why.tolist() == [want] * len(per_read) == [plain_count(lib, copt, s, dc.SEED_CAP, 0) for s in per_read]


def test_the_seeded_round_declines_for_every_reason_under_its_cap():
    """tests/test_chain_decline_gpu.py's append-then-DTW case"""
    lib, copt = ra.load_library(), M.default_chain_opt(6)
    _, per_read = cm.seeded_round()
    why, n_chains = ra.chain_decline_host(copt, per_read, 850, 0, 0)
    assert why.tolist() == [plain_count(lib, copt, s, 850, 0) for s in per_read]
    assert {1, 4, 6} <= set(why.tolist()) and sum(1 for r in range(len(per_read)) if not why[r] and n_chains[r]) >= 20


def check_case(name, got):
    want = dc.MAPPER_CASES[name]
    print(name, got)
    for k, v in got.items():
        if want.get(k) is not None:
            assert v == want[k], (name, k, v, want[k])
    n_declined = got["by_seeds"] + got["by_chains"]
    assert any(got["declined"]) and 0 < n_declined < got["pairs"] / 2
    assert got["chained_device"] > 0


@pytest.fixture(scope="module")
def ref():
    return mc.make_reference()


def test_the_whole_reads_decline_a_few_pairs_under_their_caps(oracle, ref):
    raws = mc.make_raw_reads()
    si = SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)
    wr = mc.WholeReads(0, ref=ref)
    src = oc.whole_chunks(si, wr, raws, 0)
    opt, copt = mc.whole_project_opts("default", 0)
    for name, stop in (("whole_fb", oc.never()), ("whole_default", StopOpt())):
        rounds, declined = oc.seed_counts(src, oracle, ref, opt, copt, stop)
        cands = oc.candidate_counts(src, oracle, ref, opt, copt, stop)
        assert declined == 0   # (the round end takes every read: none is seeded from the host for that)
        got = dc.mapper_figures(rounds, cands, dc.MAPPER_CASES[name]["cap"])
        check_case(name, got)
        assert any(cands[k].get(r, 0) for k, row in enumerate(rounds) for r in row if r not in got["declined"][k])   # (a device-chained read with chains)
    assert dc.MAPPER_CASES["whole_fb"]["cap"] == oc.C_FB and [bool(d) for d in dc.MAPPER_CASES["whole_fb"]["declined"]] == oc.FB_FALLS_BACK


def test_the_constructed_read_declines_alone(oracle):
    dref, reads = oc.decline_case()
    si = SeedIndex.from_signals(dref.forward, dref.reverse, threads=4)
    src = oc.EventReads(si, reads, [len(x) for x in dref.forward])
    opt, copt = mc.whole_project_opts("default", 0)
    rounds, declined = oc.seed_counts(src, oracle, dref, opt, copt, oc.never())
    cands = oc.candidate_counts(src, oracle, dref, opt, copt, oc.never())
    assert declined == 0
    check_case("decline_case", dc.mapper_figures(rounds, cands, None))
    assert dc.MAPPER_CASES["decline_case"]["declined"][oc.DECLINED_ROUND] == [oc.DECLINER]


def test_the_int16_flow_declines_fewer_than_half_of_its_pairs(oracle, flow):  # noqa: F811
    sref = flow[0]
    src = oc.flow_chunks(flow, FLOW_READS, FLOW_CHUNKS)
    rounds, declined = oc.seed_counts(src, oracle, sref, ra.MapOpt(), None, StopOpt())
    cands = oc.candidate_counts(src, oracle, sref, ra.MapOpt(), None, StopOpt())
    assert declined == 0
    got = dc.mapper_figures(rounds, cands, oc.L_MIX_FLOW)
    assert got["by_seeds"] == oc.above(rounds, oc.L_MIX_FLOW) == oc.FLOW["above"][0]
    check_case("flow", got)
    assert sum(1 for d in got["declined"] if d) == dc.MAPPER_CASES["flow"]["rounds_with_declines"] and not got["declined"][-1]


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_the_appends_offsets(tmp_path, flags):
    """rawalign_amd/csrc/rawdtw_chain_append.h by tests/abi/chain_append.cpp, with its own main: nothing is preloaded"""
    exe = os.path.join(str(tmp_path), "chain_append")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "abi", "chain_append.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok 409", run.stdout + run.stderr   # (270 rounds, 138 of them with something to append, the bad offsets)
