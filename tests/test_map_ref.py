"""Chaining, align_chain and the chunk rounds against the REFERENCE's own compiled rmap.cpp: tests/golden/map_ref_*.npz hold what
its gen_chains, align_chain and is_mapped_with_high_confidence answered (scripts/make_golden_map.py; the reference's units
compiled where they lie into oracle/_ref/libref_map{0,1}.so, oracle/ref_map_wrap.cpp).  Everything is compared on bits and
integers: scores as float32 bits, positions, counts, mapq, anchors by SHA-256.  No tolerance anywhere.

Without a device: the host chaining (rawdtw_chain_anchors, rawdtw_sort_by_chaining_score, gen_primary_chains, comp_mapq, the
stop rule), the Python mirror of the chunk loop scored by the oracle's C restatement of align_chain, and the library's mapper
(rawdtw_mapper_round) scored by the same -- for sixteen option sets and both contraction forms of rmap.cpp:306."""
import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapper
from rawalign_amd import mapping as M
from rawalign_amd.mapping import StopOpt
from tests import map_ref_cases as K
from tests.test_mapping_host import py_chain
from tests.util import OracleScorer

f32 = np.float32


@pytest.fixture(scope="module")
def fx():
    return K.Fixture()


def replay(fx, name, form, lists=None):
    """Per (read, round): the round's candidate chains from the host chaining on the stored hits, re-seeded with the chains the
    fixture holds for the round before (found among that round's candidates by their anchors' digest).  Yields
    (read, round, candidates in evaluation order or None for a chunk below min_events, events so far)."""
    opt, copt = K.project_opts(name, form)
    runs_dtw = bool(opt.flag & (K.EVAL | 0x8))
    for r in range(fx.n_reads):
        prev, offset, events = [], 0, np.zeros(0, np.float32)
        for rnd in range(fx.n_chunks(r)):
            ev, hits = fx.chunk(r, rnd)
            events = np.concatenate([events, ev])
            if len(ev) < 50:
                yield r, rnd, None, events
                continue
            if lists is not None:
                del lists[:]
            cands = K.host_candidates(prev, hits, offset, copt, len(fx.lens), sort=runs_dtw, lists_out=lists)
            offset += len(ev)
            yield r, rnd, cands, events
            by = {}
            for c in cands:
                by.setdefault((c.reference_sequence_index, c.strand, bytes(K.anchors_digest(c.anchors))), c)
            prev = []
            for rec in fx.chains(name, form, r, rnd)[0]:
                key = (int(rec["seq"]), int(rec["strand"]), bytes(rec["digest"]))
                assert key in by, (name, form, r, rnd, "a chain of the reference is not among the host chaining's candidates")
                prev.append(by[key])


def coverage(fx, verbose=False):
    """The coverage conditions of the fixture, counted from what is stored; asserts them and returns the counts as lines."""
    lines, ok = [], []
    n = fx.n_reads
    # (over the option sets: under the default options the running best of rmap.cpp:515-524 cuts nearly every second chain --
    # align_chain's attainable score counts a part's shared end event once, its final score twice -- so several primary chains
    # are the rule under global DTW and without EVALUATE_CHAINS and the exception elsewhere; `default` is counted on its own too)
    def with_two(names):
        return {r for name in names for r in range(n) for c in range(fx.n_chunks(r)) if len(fx.chains(name, 1, r, c)[0]) >= 2}
    multi = with_two(K.OPTION_SETS)
    mid = {r for name in K.OPTION_SETS for r in range(n) for c in range(fx.n_chunks(r)) for ch in fx.chains(name, 1, r, c)[0][:1] if 0 < int(ch["mapq"]) < 60}
    lines.append("reads with 2 or more primary chains in some round: %d of %d (under the default options alone: %d); reads with 0 < mapq < 60: %d"
                 % (len(multi), n, len(with_two(["default"])), len(mid)))
    ok.append((len(multi) * 5 >= n and len(mid) >= 3, lines[-1]))
    # the sets that carry the overlap rule and the mapq-below-60 path (no EVALUATE_CHAINS, or global DTW: one part, so the
    # attainable score is the final one), each on its own so that none of them can erode unnoticed
    per_set = {name: len(with_two([name])) for name in ("noeval", "global_full", "global_banded")}
    lines.append("reads with 2 or more primary chains, per set: %s" % per_set)
    ok.append((per_set["noeval"] * 5 >= n and per_set["global_full"] >= 3 and per_set["global_banded"] >= 3, lines[-1]))
    cut = below = kept = 0
    for name in K.OPTION_SETS:
        mn = f32(K.ref_opt_fields(name).get("dtw_min_score", 20.0))
        if not K.ref_opt_fields(name)["flag"] & K.EVAL:
            continue
        for form in K.FORMS:
            s = fx.z[fx.key(name, form) + "cands"]["score"].view(np.float32)
            cut += int((s == f32(-1e10)).sum())
            below += int(((s != f32(-1e10)) & (s < mn)).sum())
            kept += int((s >= mn).sum())
    lines.append("candidate scores: %d exactly -1e10, %d below dtw_min_score and not cut, %d kept" % (cut, below, kept))
    ok.append((cut and below and kept, lines[-1]))
    stops = [fx.stop_round("default", 1, r) for r in range(n)]
    hist = {k: sum(1 for s in stops if s is not None and (s + 1 == k if k < 3 else s + 1 >= 3)) for k in (1, 2, 3)}
    never = sum(1 for s in stops if s is None)
    lines.append("reads stopping at round 1: %d, 2: %d, 3 or later: %d; never mapped: %d" % (hist[1], hist[2], hist[3], never))
    ok.append((hist[1] and hist[2] and hist[3] and never >= 2, lines[-1]))
    best = {(int(ch["seq"]), int(ch["strand"])) for name in K.OPTION_SETS for form in K.FORMS
            for ch in fx.z[fx.key(name, form) + "chains"][fx.z[fx.key(name, form) + "chain_off"][:-1][np.diff(fx.z[fx.key(name, form) + "chain_off"]) > 0]]}
    lines.append("(sequence, strand) pairs carrying a best chain: %s" % sorted(best))
    ok.append(({s for s, _ in best} == set(range(len(fx.lens))) and {st for _, st in best} == {0, 1}, lines[-1]))
    ties = adjusted = 0
    radii = {}
    for name in ("default", "frac025", "frac004"):
        frac = f32(K.ref_opt_fields(name).get("dtw_band_radius_frac", 0.10))
        for r, rnd, cands, _ in replay(fx, name, 1, lists := []):
            if not cands:
                continue
            if name == "default":
                sc = [int(K.bits(c.chaining_score)) for c in cands]
                ties += int(len(set(sc)) < len(sc))
                maxs = 0.0
                for _, _, a in lists:   # a chain's score against the DP value at its end anchor (the plain-Python restatement's)
                    dp = []
                    chains, maxs = py_chain(a.astype(ra.ANCHOR_DTYPE), maxs=maxs, dp_out=dp)
                    adjusted += sum(1 for adj, idx in chains if f32(adj) != dp[idx[0]])
            for c in cands:
                a = c.anchors
                q = a["query_position"].astype(np.int64)
                if name != "default":
                    for nq in (q[:-1] - q[1:] + 1):
                        rad = max(1, int(f32(nq) * frac))
                        radii[(name, int(nq), rad)] = radii.get((name, int(nq), rad), 0) + 1
    lines.append("(read, round) pairs with two chains of equal chaining score: %d; chains adjusted by stop_at_an_used_anchor: %d" % (ties, adjusted))
    ok.append((ties >= 5 and adjusted >= 1, lines[-1]))
    small = sorted({rad for (_, nq, rad) in radii if nq < 10})
    wide = sum(v for (_, nq, rad), v in radii.items() if nq < 20 and rad >= 4)
    lines.append("band-fraction sets: radii at read-side lengths below 10: %s; parts with radius >= 4 below length 20: %d" % (small, wide))
    # (int(n * 0.25) is at most 2 for n < 10: radius 3 below length 10 is out of reach of the fractions the sets fix)
    ok.append(({1, 2} <= set(small) and wide >= 1, lines[-1]))
    if verbose:
        for line in lines:
            print(line)
    assert all(c for c, _ in ok), [line for c, line in ok if not c]
    return lines


def test_fixture_belongs_to_the_inputs_synth_makes_today(fx):
    ref = K.make_reference()
    reads = K.make_reads(ref)
    assert K.inputs_sha256(ref, reads) == fx.sha, "rawalign_amd/synth.py or tests/map_ref_cases.py drifted: run scripts/make_golden_map.py"
    assert fx.n_reads == len(reads)
    for r, vals in enumerate(reads):
        got = np.concatenate([fx.chunk(r, c)[0] for c in range(fx.n_chunks(r))])
        assert np.array_equal(got.view(np.uint32), vals.view(np.uint32))
    assert any(len(fx.chunk(r, fx.n_chunks(r) - 1)[0]) < 50 for r in range(fx.n_reads))   # a last chunk below min_events


def test_fixture_coverage(fx):
    for line in coverage(fx):
        print(line)
    # where the reference is build-dependent the inputs keep clear of it: at most 16 candidate chains a read (the order
    # std::sort leaves equal elements in at rmap.cpp:512 is an insertion sort's up to there), no best chain with a zero score
    # (comp_mapq divides by it, rmap.cpp:74-77)
    for name in K.OPTION_SETS:
        for form in K.FORMS:
            k = fx.key(name, form)
            assert int(np.diff(fx.z[k + "cand_off"]).max()) <= 16
            off = fx.z[k + "chain_off"]
            first = fx.z[k + "chains"][off[:-1][np.diff(off) > 0]]
            score = first["alignment" if K.ref_opt_fields(name)["flag"] & K.EVAL else "chaining"].view(np.float32)
            assert (score > 0).all()


def check_round(fx, name, form, r, rnd, chains, opt, what):
    want, mapped = fx.chains(name, form, r, rnd)
    got = np.array([K.chain_rec(c) for c in chains], K.CHAIN_REC) if chains else np.zeros(0, K.CHAIN_REC)
    assert len(got) == len(want), (what, name, form, r, rnd, len(got), len(want))
    assert (got == want).all(), (what, name, form, r, rnd, got, want)
    assert M.is_mapped_with_high_confidence(chains, opt, StopOpt()) == mapped, (what, name, form, r, rnd)


@pytest.mark.parametrize("name", ["noeval", "nofilter", "nbest5", "minanch3", "skips3", "band20"])
def test_host_chaining_against_the_reference(fx, name):
    """rawdtw_chain_anchors list by list with the running maximum carried on (rmap.cpp:428-507, 130-173), re-seeded with the
    round before (344-357), then gen_primary_chains / comp_mapq / the stop rule (90-128, 65-88, 594-665).  Under `noeval` the
    chaining scores decide everything and no DTW is involved; for the chaining option sets the survivors' alignment scores are
    the fixture's (the reference's align_chain), so that only the chaining and the selection are under test here.
    What this ties to the reference and what it does not: the stored candidate lists come from the project's own host chaining
    (the reference does not show its chains before selection), so a candidate that selection rejects is held as a regression
    only.  Tied to the reference are the chains that pass selection -- under `noeval` every one of them is the reference's own,
    scores, positions, anchors and mapq -- through the generator's assertion that selection on the scored candidates equals
    what gen_chains returned, and through replay()'s assertion that every chain of the reference is among the candidates."""
    opt, copt = K.project_opts(name, 1)
    for r, rnd, cands, _ in replay(fx, name, 1):
        if cands is None:
            continue
        rec = fx.candidates(name, 1, r, rnd)
        assert len(rec) == len(cands)
        post = []
        for c, k in zip(cands, rec):
            assert int(K.bits(c.chaining_score)) == int(k["chaining"]) and bytes(K.anchors_digest(c.anchors)) == bytes(k["digest"])
            if opt.flag & K.EVAL:
                c.alignment_score = float(np.uint32(k["score"]).view(np.float32))
                if f32(c.alignment_score) >= f32(opt.dtw_min_score):
                    post.append(c)
            else:
                post.append(c)
        check_round(fx, name, 1, r, rnd, M.gen_primary_chains(post, opt) if post else [], opt, "host chaining")


class RecordingScorer(OracleScorer):
    """the oracle's scorer, keeping every round's candidate scores (evaluation order) per read"""

    def __init__(self, oracle, ref):
        super().__init__(oracle, ref)
        self.rounds = []

    def score(self, reads, opt):
        out = super().score(reads, opt)
        self.rounds.append([[(c.alignment_score, c) for c in chains] for _, chains in reads])
        return out


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("name", list(K.OPTION_SETS))
def test_python_mirror_with_the_oracle_scorer_against_the_reference(fx, oracle, name, form):
    """mapper.map_reads (the mirror of map_worker_for / ri_map_frag / gen_chains) with the C restatement of align_chain as the
    scorer: every round's chains of every read, every candidate's score (cut chains and ties included), the stop rule."""
    opt, copt = K.project_opts(name, form)
    reads = list(range(fx.n_reads))
    sc = RecordingScorer(oracle, fx.ref)
    seen = []

    def on_round(rnd, chains):
        for r, cs in chains.items():
            check_round(fx, name, form, r, rnd - 1, cs, opt, "python mirror")
            seen.append((r, rnd - 1))
    mapper.map_reads(fx, reads, sc, opt, StopOpt(**K.NEVER), chain_opt=copt, on_round=on_round)
    assert len(seen) == sum(fx.n_chunks(r) for r in reads)
    if opt.flag & K.EVAL:
        for rnd, per_read in enumerate(sc.rounds):
            active = [r for r in reads if fx.n_chunks(r) > rnd]
            assert len(active) == len(per_read)
            for r, cs in zip(active, per_read):
                want = fx.candidates(name, form, r, rnd)
                assert len(cs) == len(want), (name, form, r, rnd)
                for (s, c), k in zip(cs, want):
                    assert int(K.bits(s)) == int(k["score"]) and int(K.bits(c.chaining_score)) == int(k["chaining"]), (name, form, r, rnd, s, k)
                    assert bytes(K.anchors_digest(c.anchors)) == bytes(k["digest"])
    if opt.flag & K.CIGAR:   # the final alignment of a mapped read (rmap.cpp:715-717) against the reference's align_chain(cigar)
        k = fx.key(name, form)
        for i, r in enumerate(fx.z[k + "cigar_read"]):
            rnd = fx.stop_round(name, form, int(r))
            ev = np.concatenate([fx.chunk(int(r), c)[0] for c in range(rnd + 1)])
            rec = fx.chains(name, form, int(r), rnd)[0][0]
            best = [c for _, c in sc.rounds[rnd][[q for q in reads if fx.n_chunks(q) > rnd].index(int(r))] if bytes(K.anchors_digest(c.anchors)) == bytes(rec["digest"])][0]
            ch = sc.align_cigar(ra.Chain(best.chaining_score, best.reference_sequence_index, best.strand, best.anchors), ev, opt)
            d = ch.dtw_result
            assert int(K.bits(ch.alignment_score)) == int(fx.z[k + "cigar_alns"][i]) and int(K.bits(d.cost)) == int(fx.z[k + "cigar_cost"][i])
            assert len(d.i) == int(fx.z[k + "cigar_len"][i]) and bytes(K.path_digest(d.i, d.j, d.difference)) == bytes(fx.z[k + "cigar_digest"][i])


def oracle_scorer_fn(oracle, ref, opt):
    from tests.test_mapper_cpu import _oracle_scorer

    return _oracle_scorer(oracle, ref, opt)


def parse(line):
    f = line.split("\t")
    mapped = f[4] in "+-"
    tags = {}
    for t in f[12:]:
        k, _, v = t.split(":", 2)
        tags[k] = v
    return f, mapped, tags


def fmt(x):
    return "%f" % float(x)


def check_lines_default_stop(fx, name, form, lines, what):
    """PAF lines of a run under the default stop rule against the fixture's chains at every read's stop round: mapq, strand,
    sequence, start, end (rmap.cpp:749-756), ci, cm, nc, s1, s2, sm, anchors:s: (731-747)"""
    n_mapped = 0
    for r, line in enumerate(lines):
        f, mapped, tags = parse(line)
        rnd = fx.stop_round(name, form, r)
        assert mapped == (rnd is not None), (what, name, form, r, line)
        last = rnd if mapped else fx.n_chunks(r) - 1
        ch = fx.chains(name, form, r, last)[0]
        assert int(tags["nc"]) == len(ch), (what, name, form, r)
        if len(ch) == 0:
            assert tags["cm"] == "0" and tags["s1"] == "0"
            continue
        c0 = ch[0]
        sm = f32(0)
        for c in ch:
            sm = f32(sm + np.uint32(c["chaining"]).view(np.float32))
        sm = f32(sm / f32(len(ch)))
        assert int(tags["cm"]) == int(c0["n_anchors"]) and tags["s1"] == fmt(np.uint32(c0["chaining"]).view(np.float32)), (what, name, form, r, line)
        assert tags["s2"] == (fmt(np.uint32(ch[1]["chaining"]).view(np.float32)) if len(ch) > 1 else fmt(0)), (what, name, form, r)   # (rmap.cpp:737: the conditional is a float either way)
        assert tags["sm"] == fmt(sm), (what, name, form, r)
        assert tags["at"] == fmt(np.uint32(c0["at"]).view(np.float32)) and tags["aq"] == fmt(np.uint32(c0["aq"]).view(np.float32)), (what, name, form, r, line)
        if not mapped:
            continue
        n_mapped += 1
        assert tags["ci"] == str(rnd + 1)
        start, end, L = int(c0["start"]), int(c0["end"]), int(fx.lens[int(c0["seq"])])
        assert f[4] == ("-" if c0["strand"] else "+") and f[5] == "seq%d" % int(c0["seq"]) and int(f[6]) == L
        assert int(f[7]) == ((L + 1 - end) if c0["strand"] else start) and int(f[10]) == end - start + 1 and int(f[11]) == int(c0["mapq"])
        a = np.array([tuple(int(x) for x in p.split(",")) for p in tags["anchors"].strip("()").split(")(")], np.int64)   # (query, target)
        an = np.zeros(len(a), ra.ANCHOR_DTYPE)
        an["query_position"], an["target_position"] = a[:, 0], a[:, 1]
        assert bytes(K.anchors_digest(an)) == bytes(c0["digest"]), (what, name, form, r)
        if K.ref_opt_fields(name)["flag"] & K.CIGAR and what != "C mapper":
            k = fx.key(name, form)
            i = list(fx.z[k + "cigar_read"]).index(r)
            assert tags["alns"] == fmt(np.uint32(fx.z[k + "cigar_alns"][i]).view(np.float32))
            assert tags["aln"].count("(") == int(fx.z[k + "cigar_len"][i])
    return n_mapped


def check_lines_after_c_chunks(fx, name, form, c, lines, what):
    """a run that never stops and has max_num_chunk = c: every read is unmapped, its line shows the chains after round
    min(c, its chunks): cm, nc, s1, s2, sm, at, aq.  (ci and the
    read length depend on the chunk accounting of rmap.cpp:696 and are left to the default-stop comparison.)"""
    for r, line in enumerate(lines):
        f, mapped, tags = parse(line)
        assert not mapped
        ch = fx.chains(name, form, r, min(c, fx.n_chunks(r)) - 1)[0]
        assert int(tags["nc"]) == len(ch), (what, name, form, c, r, line)
        if len(ch):
            sm = f32(0)
            for x in ch:
                sm = f32(sm + np.uint32(x["chaining"]).view(np.float32))
            assert int(tags["cm"]) == int(ch[0]["n_anchors"]) and tags["s1"] == fmt(np.uint32(ch[0]["chaining"]).view(np.float32))
            assert tags["s2"] == (fmt(np.uint32(ch[1]["chaining"]).view(np.float32)) if len(ch) > 1 else fmt(0))
            assert tags["sm"] == fmt(f32(sm / f32(len(ch)))), (what, name, form, c, r)
            assert tags["at"] == fmt(np.uint32(ch[0]["at"]).view(np.float32)) and tags["aq"] == fmt(np.uint32(ch[0]["aq"]).view(np.float32)), (what, name, form, c, r, line)


def run_c_mapper(fx, name, form, stop, engine=None, scorer=None, **kw):
    opt, copt = K.project_opts(name, form)
    if engine is None:
        opt.flag &= ~K.CIGAR   # (the final traceback of rmap.cpp:715-717 is the device's: the cigar set's lines carry alns / aln in the GPU test)
    cm = mapper.CMapper(engine, opt, stop, ["seq%d" % s for s in range(len(fx.lens))], [int(x) for x in fx.lens], slot_events=2048,
                        max_reads=fx.n_reads, chain_opt=copt, output_chains=True, **kw)
    if scorer is not None:
        cm.set_scorer(scorer)
    lines, _ = mapper.map_reads_c(fx, list(range(fx.n_reads)), cm)
    cm.close()
    return lines


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("k,name", list(enumerate(K.OPTION_SETS)))
def test_c_mapper_with_the_oracle_scorer_against_the_reference(fx, oracle, k, name, form):
    """rawdtw_mapper_round through CMapper, the oracle as the scorer (no device): the PAF fields the fixture holds, under the
    default stop rule and, round by round, under max_num_chunk = c with a stop rule that never fires; threads, groups and
    carry vary with the option set"""
    opt, _ = K.project_opts(name, form)
    sc = oracle_scorer_fn(oracle, fx.ref, opt)
    kw = dict(threads=(1, 4, 3)[k % 3], groups=1 + (k + form) % 2, carry=bool((k // 2 + form) % 2))
    n = check_lines_default_stop(fx, name, form, run_c_mapper(fx, name, form, StopOpt(), scorer=sc, **kw), "C mapper")
    assert n >= fx.n_reads // 2
    for c in range(1, max(fx.n_chunks(r) for r in range(fx.n_reads)) + 1):
        lines = run_c_mapper(fx, name, form, StopOpt(max_num_chunk=c, **K.NEVER), scorer=sc, **kw)
        check_lines_after_c_chunks(fx, name, form, c, lines, "C mapper")


@pytest.mark.skipif(not __import__("oracle.loader", fromlist=["RefMap"]).RefMap.available(), reason="oracle/_ref/libref_map*.so are built only where the reference's sources are")
@pytest.mark.parametrize("seed", [1, 2])
def test_live_reference_on_fresh_reads(oracle, seed):
    """Breadth beyond the committed fixture: the reference library itself on reads drawn with other seeds (other stretches, noise,
    strands), recorded in memory the way the fixture is, against the Python mirror and the C mapper."""
    ref = K.make_reference()
    rng = np.random.default_rng(1000 + seed)
    reads = []
    for _ in range(6):
        s, st = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        n = int(rng.integers(300, 1500))
        start = int(rng.integers(0, len(ref.forward[s]) - n))
        arr = ref.forward[s] if st else ref.reverse[s]
        reads.append((arr[start:start + n] + rng.normal(0, rng.uniform(0.03, 0.25), n)).astype(np.float32))
    reads.append(rng.normal(0, 1, 700).astype(np.float32))
    live = K.Fixture(K.record_inputs(ref, reads), {}, ref)
    cov = dict(cut=0, below=0, kept=0, ties=0)
    for name, form in (("default", 1), ("default", 0), ("frac025", 1), ("global_full", 0), ("nofilter", 1), ("noeval", 0)):
        K.run_set(live, ref, name, form, live.z, cov)
        opt, copt = K.project_opts(name, form)
        mapper.map_reads(live, list(range(live.n_reads)), OracleScorer(oracle, ref), opt, StopOpt(**K.NEVER), chain_opt=copt,
                         on_round=lambda rnd, chains: [check_round(live, name, form, r, rnd - 1, cs, opt, "live") for r, cs in chains.items()])
        lines = run_c_mapper(live, name, form, StopOpt(), scorer=oracle_scorer_fn(oracle, ref, opt), threads=2)
        check_lines_default_stop(live, name, form, lines, "live C mapper")
    assert cov["kept"] > 0


# ---- whole raw reads: what the reference's map_worker_for printed (tests/golden/map_ref_reads.npz) -------------------------------------
def test_whole_read_fixture_belongs_to_the_raw_reads_synth_makes_today():
    z = np.load(K.READS)
    assert K.raw_sha256(K.make_raw_reads()) == z["raw_sha256"].tobytes(), "synth.make_genome_raw_reads or tests/map_ref_cases.py drifted: run scripts/make_golden_map.py"
    for form in K.FORMS:   # the records cover mapped reads on both strands, stops after 1, 2 and 3 chunks, and an unmapped read
        rec = z["default/%d/records" % form]
        ci = {str(t).split("\t")[0] for t in z["default/%d/tags" % form]}
        assert set(rec[:, 0]) == {0, 1} and set(rec[rec[:, 0] == 1][:, 8]) == {0, 1} and {"ci:i:1", "ci:i:2", "ci:i:3"} <= ci


@pytest.mark.parametrize("form", K.FORMS)
def test_detect_events_host_against_the_reference_on_the_raw_reads(form):
    """the project's detect_events_host, plain and contracted, on every chunk of the raw reads against the events the reference's
    detect_events gave (revent.c:190, built with contraction off and as an FMA host builds it): bit for bit"""
    from rawalign_amd import events as E

    wr = K.WholeReads(form)
    raws = K.make_raw_reads()
    chunks = [c for sig in raws for c in K.raw_chunks(sig)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint64)
    eoff, ev = E.detect_events_host(np.concatenate(chunks), off, E.EventOptions(contracted=bool(form)), threads=2)
    assert np.array_equal(eoff.astype(np.int64), wr.ev_off) and np.array_equal(ev.view(np.uint32), wr.events.view(np.uint32))
    assert len(ev) > 5000


def whole_read_lines_c(wr, name, form, engine=None, scorer=None, **kw):
    opt, copt = K.whole_project_opts(name, form)
    cm = mapper.CMapper(engine, opt, StopOpt(), ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], slot_events=4096,
                        max_reads=wr.n_reads, chain_opt=copt, output_chains=True, **kw)
    if scorer is not None:
        cm.set_scorer(scorer)
    lines, _ = mapper.map_reads_c(wr, list(range(wr.n_reads)), cm)
    cm.close()
    return lines


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("name", list(K.WHOLE_SETS))
def test_whole_reads_against_what_the_reference_printed(oracle, name, form):
    """Whole raw reads: the reference's own chunk loop (map_worker_for: detect_events, seeding, gen_chains, the stop rule, the
    record and tags of rmap.cpp:696-801) recorded per read; the Python mirror and the C++ mapper, fed the stored events and hits
    chunk by chunk, must print the same line field for field -- read length and positions, strand sign, fragment start and
    length, mapq, ci, sl, cm, nc, s1, s2, sm, at, aq, anchors:s:, and alns / aln under the cigar flag (the mirror; the C++
    mapper's final traceback is the device's, so its cigar lines are compared in tests/test_map_ref_gpu.py)."""
    wr = K.WholeReads(form)
    opt, copt = K.whole_project_opts(name, form)
    want = [wr.expected_line(name, r) for r in range(wr.n_reads)]
    got, _ = mapper.map_reads(wr, list(range(wr.n_reads)), OracleScorer(oracle, wr.ref), opt, StopOpt(), chain_opt=copt, output_chains=True)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.replace("synth_", "seq") == w, ("python mirror", name, form, r)
    if not opt.flag & K.CIGAR:
        got = whole_read_lines_c(wr, name, form, scorer=oracle_scorer_fn(oracle, wr.ref, opt), threads=2)
        for r, (g, w) in enumerate(zip(got, want)):
            assert g == w, ("C mapper", name, form, r)
