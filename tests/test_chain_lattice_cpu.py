"""tests/chain_lattice_cases.py on the host: on every case the tracer (py_chain of tests/test_mapping_host.py, tracing) and
rawdtw_chain_anchors agree -- scores by bits, every anchor of every chain (the predecessors), the running maximum --, the tracer finds each
probe's exit, winner and carried counter where the generator meant them, the coverage table of the predecessor loop's lanes holds, and each
probe's result is observed in the chains its read reports."""
import numpy as np
import pytest

from rawalign_amd import mapping as M
from rawalign_amd.dtw import ANCHOR_DTYPE
from tests import chain_lattice_cases as cl
from tests.test_mapping_host import f32

LANES = [(b, l) for b in range(cl.BLOCKS) for l in range(64)]


@pytest.fixture(scope="module")
def traced():
    """[(round name, options, [(probe, chains, maxs, the probe anchor's trace, DP values of its list)])] -- computed once"""
    out = []
    for name, copt, probes in cl.rounds():
        rows = []
        for p in probes:
            chains, maxs, tr, dp = cl.trace_read(p["seeds"], copt)
            rows.append((p, chains, maxs, tr[-1], dp))
        out.append((name, copt, rows))
    return out


def host_chains_as_generated(seeds, copt):
    chains, maxs = [], 0.0
    for key, g in cl.sorted_lists(seeds):
        a = np.zeros(len(g), ANCHOR_DTYPE)
        a["target_position"], a["query_position"] = g["target_position"], g["query_position"]
        cs, maxs = M.chain_anchors(a, copt, maxs, key >> 1, key & 1)
        chains += [(f32(c.chaining_score), key, [(int(x["target_position"]), int(x["query_position"])) for x in c.anchors]) for c in cs]
    return chains, maxs


def test_counts(traced):
    n_probes = sum(len(rows) for _, _, rows in traced)
    print("rounds", len(traced), "probes", n_probes, "seeds", sum(len(p["seeds"]) for _, _, rows in traced for p, *_ in rows),
          "longest", max(len(p["seeds"]) for _, _, rows in traced for p, *_ in rows))
    assert len(traced) == len(cl.SKIP_ROUNDS) + len(cl.BANDS) + 6
    assert max(len(p["seeds"]) for _, _, rows in traced for p, *_ in rows) <= 270   # (about 260: three blocks, the bait, the gap anchor and up to 63 fillers)


def test_tracer_and_host_function_agree_on_every_case(traced):
    for name, copt, rows in traced:
        for p, chains, maxs, _, _ in rows:
            got, gmax = host_chains_as_generated(p["seeds"], copt)
            assert f32(gmax).view(np.uint32) == f32(maxs).view(np.uint32), (name, p["name"])
            assert len(got) == len(chains), (name, p["name"], got, chains)
            for (gs, gk, ga), (ws, wk, wa) in zip(got, chains):
                assert gs.view(np.uint32) == ws.view(np.uint32) and gk == wk and ga == wa, (name, p["name"])


def test_every_probe_ends_wins_and_carries_where_it_was_meant_to(traced):
    for name, copt, rows in traced:
        for p, _, _, tr, _ in rows:
            w = p["want"]
            if "exit" in w:
                assert (tr["exit"], tr["exit_off"], tr["last"]) == (w["exit"], w["exit_off"], w["last"]), (name, p["name"], tr)
                assert tr["improvers"] == sorted(tr["improvers"])
                assert tr["pred"] == (tr["ai"] if tr["last"] is None else tr["ai"] - 1 - tr["last"])
                assert tr["score"] == f32(cl.E + (0 if tr["last"] is None else cl.A0 + tr["last"]))
            if "carry" in w:
                boundary, c = w["carry"]
                assert tr["carry"][boundary - 1] == c, (name, p["name"], tr)
            if "tie" in w:
                near, far = w["tie"]
                assert near in tr["improvers"] and far not in tr["improvers"] and tr["last"] == near, (name, p["name"], tr)


def test_no_candidate_of_a_lattice_probe_chains_with_another(traced):
    """every anchor but the probe scores e, so that the read reports [probe, winner] and nothing else"""
    for name, copt, rows in traced:
        for p, chains, _, tr, dp in rows:
            if p["family"] in ("value", "end"):
                continue
            assert all(x == f32(cl.E) for x in dp[:-1]), (name, p["name"])
            assert len(chains) == (0 if tr["last"] is None else 1), (name, p["name"], chains)


def cells(traced, family, reason, rounds=None):
    got = set()
    for name, _, rows in traced:
        if rounds is not None and name not in rounds:
            continue
        for p, _, _, tr, _ in rows:
            if p["family"] == family and tr["exit"] == reason:
                got.add((tr["exit_off"] // 64, tr["exit_off"] % 64))
    return got


def test_coverage_of_the_exit(traced):
    assert cells(traced, "exit_gap", "gap") == set(LANES)
    assert cells(traced, "exit_start", "band") == set(LANES)
    for m in cl.SKIP_ROUNDS:
        # (UNREACHABLE["exit_skip"]: no exit by skip below offset m)
        assert cells(traced, "exit_skip", "skip", rounds=("skips %d" % m,)) == {(b, l) for b, l in LANES if 64 * b + l >= m}, m
    assert cells(traced, "exit_skip", "skip") == set(LANES)
    # exits on lanes 0 .. 24 of block 0, which no earlier input reached but under max_num_skips = 3
    assert {(0, l) for l in range(25)} <= cells(traced, "exit_skip", "skip", rounds=("skips 0", "skips 1", "skips 2"))
    # the band's true end: one round a length, in a list that is not the read's first, g0 no multiple of 64
    for b in cl.BANDS:
        rows = [r for name, _, rs in traced if name == "band %d" % b for r in rs]
        assert rows and all(tr["exit"] == "band" and tr["exit_off"] == b for _, _, _, tr, _ in rows), b
        for p, *_ in rows:
            lists = cl.sorted_lists(p["seeds"])
            assert len(lists) == 2 and len(lists[0][1]) % 64 != 0 and len(lists[1][1]) - 1 > b


def test_coverage_of_the_winner(traced):
    win, after_lower = set(), set()
    for _, _, rows in traced:
        for p, _, _, tr, _ in rows:
            if tr["last"] is not None:
                win.add((tr["last"] // 64, tr["last"] % 64))
                if tr["last"] >= 64 and any(i < 64 for i in tr["improvers"]):
                    after_lower.add((tr["last"] // 64, tr["last"] % 64))   # `best` arrives from the step before
    assert win >= set(LANES)
    assert after_lower >= {(b, l) for b, l in LANES if b >= 1}


def test_coverage_of_the_carried_counter(traced):
    seen = {}
    for name, copt, rows in traced:
        for p, _, _, tr, _ in rows:
            for c in tr["carry"]:
                seen.setdefault(copt.max_num_skips, set()).add(c)
    assert min(seen[25]) <= -64 and {-17, -16, -15, -2, -1, 0, 1, 24, 25} <= seen[25]
    for m in cl.SKIP_ROUNDS:
        assert {m - 1, m} <= seen[m], (m, seen[m])
    # the counter at max_num_skips on entry: the exit is lane 0 of that block
    for name, copt, rows in traced:
        for p, _, _, tr, _ in rows:
            if p["family"] == "carry" and p["want"]["carry"][1] == copt.max_num_skips:
                assert tr["exit"] == "skip" and tr["exit_off"] == 64 * p["want"]["carry"][0]
    # a run of improvers across a boundary
    assert any(p["family"] == "carry" and {62, 63, 64, 65} <= set(tr["improvers"]) for _, _, rows in traced for p, _, _, tr, _ in rows)
    assert any(p["family"] == "carry" and {126, 127, 128, 129} <= set(tr["improvers"]) for _, _, rows in traced for p, _, _, tr, _ in rows)


def test_coverage_of_ties_and_residues(traced):
    ties = {p["want"]["tie"] for _, _, rows in traced for p, *_ in rows if p["family"] == "tie"}
    assert {(x, x + 1) for x in cl.TIE_LANES} <= ties
    assert any(p["family"] == "tie" and tr["exit"] == "skip" and tr["exit_off"] == p["want"]["tie"][1] for _, _, rows in traced for p, _, _, tr, _ in rows)
    res = {}
    for _, _, rows in traced:
        for p, _, _, tr, _ in rows:
            if p["family"] == "residue":
                n = len(p["seeds"])
                assert (n - 1) % 64 == p["want"]["residue"], p["name"]   # the probe is the read's last anchor
                res.setdefault((tr["exit"], tr["exit_off"]), set()).add((n - 1) % 64)
    for d in cl.RESIDUE_OFFSETS:
        assert res[("gap", d)] == set(cl.RESIDUES) and res[("band", d)] == set(cl.RESIDUES), d
    for d in [d for d in cl.RESIDUE_OFFSETS if d >= 30]:
        assert res[("skip", d)] == set(cl.RESIDUES), d


def test_each_probe_decides_a_reported_chain(traced):
    """per family: what the read reports shows the probe's result"""
    for name, copt, rows in traced:
        for p, chains, _, tr, _ in rows:
            fam, w = p["family"], p["want"]
            if fam in ("exit_skip", "exit_gap", "exit_start", "exit_band", "carry", "residue", "tie"):
                lst = cl.sorted_lists(p["seeds"])[-1][1]
                probe_at = len(lst) - 1
                baited = fam in ("exit_skip", "carry", "exit_band") or (fam in ("tie", "residue") and tr["exit"] == "skip")
                if baited:
                    # a loop that goes on past the exit finds a better predecessor right there
                    bait = lst[probe_at - 1 - (tr["exit_off"] + (0 if fam == "exit_band" else 1))]
                    assert int(bait["query_position"]) == cl.Q0 - cl.Q_I and cl.T0 - int(bait["target_position"]) > cl.A0 + (-1 if tr["last"] is None else tr["last"]), (name, p["name"])
                if tr["last"] is None:
                    # the loop has to end before any improver: no chain.  The bait would make one; an exit by gap or list start has nothing
                    # in front of it here (offset 0, or skippers and passed-over candidates only)
                    assert chains == [] and (baited or tr["exit_off"] == 0), (name, p["name"])
                    continue
                (score, key, an), = chains
                winner = lst[probe_at - 1 - tr["last"]]
                assert an == [(cl.T0, cl.Q0), (int(winner["target_position"]), int(winner["query_position"]))], (name, p["name"])
                assert score == f32(cl.E + cl.A0 + tr["last"])
                if fam == "tie":
                    far = lst[probe_at - 1 - w["tie"][1]]
                    assert (int(far["target_position"]), int(far["query_position"])) != an[1]   # the two are told apart by their positions
            elif fam == "value":
                if "score" in w:
                    assert len(chains) == 1 and chains[0][0] == f32(w["score"]) and len(chains[0][2]) == 3, (name, p["name"], chains)
                elif w["scores"]:
                    assert len(chains) == 1 and chains[0][0] == f32(copt.e + min(w["td"], w["qd"], copt.e)) and len(chains[0][2]) == 2, (name, p["name"], chains)
                else:
                    assert chains == [], (name, p["name"], chains)
            else:
                assert fam == "end"
                assert [float(c[0]) for c in chains] == w["chain_scores"], (name, p["name"], chains)
