"""The inputs, option sets and fixture access of tests/golden/map_ref_*.npz: the answers of the REFERENCE's own mapping code
(src/rmap.cpp compiled where it lies, oracle/_ref/libref_map{0,1}.so) recorded by scripts/make_golden_map.py.

Shared by the generator and by tests/test_map_ref.py / tests/test_map_ref_gpu.py, so that both draw the same inputs.  The
inputs are seeded and regenerated anywhere; the fixture carries their SHA-256 and the events and hits themselves."""
import hashlib
import os

import numpy as np

import rawalign_amd as ra
from rawalign_amd import mapping as M
from rawalign_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "map_ref_inputs.npz")
READS = os.path.join(HERE, "golden", "map_ref_reads.npz")
ROUNDS = os.path.join(HERE, "golden", "map_ref_rounds.npz")

EVENTS_PER_CHUNK = 400
SEQ_LENS = (9000, 7000, 6000)
REF_SEED = 20240611
E = 6   # events a seed (ri_idxopt_init)

# roptions.h flags
EVAL, CIGAR, NOFILTER, OUTCHAINS = 0x2, 0x4, 0x10, 0x20

# Option sets: name -> fields of ri_mapopt_t that differ from ri_mapopt_init (names of oracle.loader.RefMapOpt)
OPTION_SETS = {
    "default": {},
    "global_full": dict(dtw_border_constraint=0, dtw_fill_method=0),
    "sparse_full": dict(dtw_fill_method=0),
    "global_banded": dict(dtw_border_constraint=0, dtw_fill_method=1),
    "frac025": dict(dtw_band_radius_frac=0.25),
    "frac004": dict(dtw_band_radius_frac=0.04),
    "bonus06": dict(dtw_match_bonus=0.6),
    "min5": dict(dtw_min_score=5.0),
    "min60": dict(dtw_min_score=60.0),
    "nbest5": dict(num_best_chains=5),
    "minanch3": dict(min_num_anchors=3),
    "skips3": dict(max_num_skips=3),
    "band20": dict(chaining_band_length=20),
    "nofilter": dict(flag=EVAL | NOFILTER),
    "noeval": dict(flag=0),
    "cigar": dict(flag=EVAL | CIGAR),
}
FORMS = (0, 1)   # 0: contraction off (libref_map0), 1: the FMA build (libref_map1); MapOpt.fused_score


def ref_opt_fields(name):
    """the RefMapOpt fields of an option set (flag defaults to EVALUATE_CHAINS: ri_mapopt_init leaves it 0, main.cpp sets it)"""
    f = dict(flag=EVAL)
    f.update(OPTION_SETS[name])
    return f


def project_opts(name, form):
    """(MapOpt, ChainOpt) of an option set for the project's side"""
    f = ref_opt_fields(name)
    opt = ra.MapOpt(dtw_border_constraint=f.get("dtw_border_constraint", 1), dtw_fill_method=f.get("dtw_fill_method", 1),
                    dtw_band_radius_frac=f.get("dtw_band_radius_frac", 0.10), dtw_match_bonus=f.get("dtw_match_bonus", 0.4),
                    dtw_min_score=f.get("dtw_min_score", 20.0), flag=f["flag"] & (EVAL | CIGAR | 0x8), fused_score=bool(form))
    copt = M.ChainOpt(2000, 5000, f.get("chaining_band_length", 5000), f.get("max_num_skips", 25), f.get("min_num_anchors", 2),
                      f.get("num_best_chains", 3), 10.0, E, 1 if f["flag"] & NOFILTER else 0)
    return opt, copt


NEVER = dict(min_bestmap_ratio=1e9, min_meanmap_ratio=1e9, min_chain_anchor=10 ** 6)


def make_reference():
    """three sequences; one stretch copied exactly to another sequence (equal hits, equal scores: ties) and one copied with
    small noise onto the other strand's array of a third (competing chains, mapq between 0 and 60)"""
    ref = synth.make_reference(SEQ_LENS, seed=REF_SEED)
    rng = np.random.default_rng(REF_SEED + 1)
    fwd = [x.copy() for x in ref.forward]
    rev = [x.copy() for x in ref.reverse]
    fwd[1][1500:2400] = fwd[0][2000:2900]                                                     # exact copy, 900 events
    rev[2][3000:4000] = (fwd[1][4000:5000] + rng.normal(0, 0.03, 1000)).astype(np.float32)    # noisy copy on the other strand
    rev[0][6000:6700] = (rev[1][500:1200] + rng.normal(0, 0.02, 700)).astype(np.float32)
    return synth.Reference(fwd, rev, ref.names)


# (sequence, strand, start, events, noise sd) -- strand 1 reads the forward array (rmap.cpp:183-188); None: from nowhere
READ_SPECS = [
    (0, 1, 300, 1200, 0.05), (0, 0, 1000, 1230, 0.08), (1, 1, 5200, 800, 0.05), (1, 0, 3000, 1630, 0.12),
    (2, 1, 200, 1020, 0.10), (2, 0, 500, 430, 0.05), (0, 1, 6000, 400, 0.15), (2, 1, 4000, 1600, 0.20),
    # on the exact copy (sequence 0 2000..2900 == sequence 1 1500..2400): inside it, leaving it after 1, 2, 3 chunks
    (0, 1, 2000, 800, 0.05), (0, 1, 2450, 1200, 0.05), (0, 1, 2100, 1600, 0.06), (1, 1, 1500, 1600, 0.05),
    (1, 1, 1700, 1230, 0.10), (0, 1, 1700, 1600, 0.08), (1, 1, 1550, 830, 0.07),
    # on the noisy copies
    (1, 1, 4000, 1200, 0.05), (2, 0, 3000, 1600, 0.05), (1, 1, 4300, 1220, 0.10), (2, 0, 3500, 1200, 0.08),
    (1, 0, 500, 1200, 0.05), (0, 0, 6100, 1000, 0.06), (1, 0, 300, 1600, 0.10),
    # sparse anchors (noisy reads) on the noisy copies: either chain may come first in the evaluation order
    (2, 0, 3100, 800, 0.22), (1, 1, 4100, 800, 0.22), (2, 0, 3300, 790, 0.25), (1, 1, 4500, 420, 0.2), (1, 0, 600, 560, 0.22), (0, 0, 6050, 600, 0.22),
    # a stretch of the read repeated (events 100..200 twice): a second chain that runs into the first one's anchors
    (0, 1, 4000, 800, 0.05, "repeat"), (1, 0, 5000, 1200, 0.06, "repeat"), (2, 1, 2500, 780, 0.08, "repeat"),
    # one and two chunks from nowhere in front (a stalled pore, an adapter): the read maps a round or two later
    (0, 1, 5000, 1200, 0.05, "junk1"), (1, 0, 2000, 1600, 0.08, "junk2"), (2, 1, 1000, 1230, 0.06, "junk1"), (0, 0, 3000, 1600, 0.05, "junk2"),
    # short segments of one neighbourhood in scrambled order: anchors of many diagonals interleave in target order, so that the
    # chaining DP's skip counter (rmap.cpp:476-484: down on an improvement, up otherwise) decides where the inner loop ends
    ("scramble", 15), ("scramble", 18), ("scramble", 23), ("scramble", 24),
    None, None, None,
]


def make_reads(ref):
    """event-level reads: noisy copies of reference stretches on both strands with a few events dropped or doubled, reads from
    nowhere, and reads whose last chunk is shorter than min_events; chunks of EVENTS_PER_CHUNK events"""
    rng = np.random.default_rng(REF_SEED + 2)
    reads = []
    for k, spec in enumerate(READ_SPECS):
        if spec is None:
            vals = rng.normal(0, 1, 800 + 30 * (k % 2)).astype(np.float32)
        elif spec[0] == "scramble":
            g = np.random.default_rng(5000 + spec[1])
            s, st = int(g.integers(0, 3)), int(g.integers(0, 2))
            arr = ref.forward[s] if st else ref.reverse[s]
            start = int(g.integers(0, len(arr) - 700))
            seg = int(g.integers(12, 40))
            idx = np.concatenate([np.arange(a, a + seg) for a in start + g.integers(0, 200, 2 * (EVENTS_PER_CHUNK // seg))])
            vals = (arr[idx] + g.normal(0, 0.04, len(idx))).astype(np.float32)
        else:
            s, st, start, n, sd = spec[:5]
            kind = spec[5] if len(spec) > 5 else ""
            arr = ref.forward[s] if st == 1 else ref.reverse[s]
            idx = np.arange(start, start + n)
            if kind == "repeat":
                idx = np.concatenate([idx[:200], idx[100:200], idx[200:]])[:n]
            mult = rng.choice(3, size=n, p=(0.02, 0.95, 0.03))   # dropped / kept / doubled
            idx = np.repeat(idx, mult)[:n]
            vals = (arr[idx] + rng.normal(0, sd, len(idx))).astype(np.float32)
            if kind.startswith("junk"):
                j = int(kind[4:]) * EVENTS_PER_CHUNK
                vals[:j] = rng.normal(0, 1, j).astype(np.float32)
        reads.append(vals)
    return reads


def chunks_of(vals):
    return [vals[i:i + EVENTS_PER_CHUNK] for i in range(0, len(vals), EVENTS_PER_CHUNK)]


def inputs_sha256(ref, reads) -> bytes:
    h = hashlib.sha256()
    for x in list(ref.forward) + list(ref.reverse) + list(reads):
        h.update(np.ascontiguousarray(x, "<f4").tobytes())
        h.update(np.array([len(x)], "<i8").tobytes())
    return h.digest()


def anchors_digest(anchors) -> np.ndarray:
    """8 bytes of the SHA-256 of a chain's anchors (target, query as little-endian uint32, end-first)"""
    a = np.ascontiguousarray(anchors, ra.ANCHOR_DTYPE)
    h = hashlib.sha256()
    h.update(a["target_position"].astype("<u4").tobytes())
    h.update(a["query_position"].astype("<u4").tobytes())
    return np.frombuffer(h.digest()[:8], np.uint8)


def path_digest(pi, pj, pd) -> np.ndarray:
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(pi, "<u8").tobytes())
    h.update(np.ascontiguousarray(pj, "<u8").tobytes())
    h.update(np.ascontiguousarray(pd, "<f4").view("<u4").tobytes())
    return np.frombuffer(h.digest()[:8], np.uint8)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
CHAIN_REC = np.dtype([("chaining", "<u4"), ("alignment", "<u4"), ("seq", "u1"), ("strand", "u1"), ("mapq", "u1"), ("pad", "u1"),
                      ("start", "<u4"), ("end", "<u4"), ("n_anchors", "<u4"), ("digest", "u1", (8,)), ("at", "<u4"), ("aq", "<u4")])
CAND_REC = np.dtype([("chaining", "<u4"), ("score", "<u4"), ("seq", "u1"), ("strand", "u1"), ("n_anchors", "<u2"), ("digest", "u1", (8,))])


class Fixture:
    """Events and hits per (read, chunk); per (option set, form): per (read, round) the chains gen_chains left (CHAIN_REC), the
    stop rule's answer under the default stop options, the candidate chains of the round in evaluation order with the reference's
    align_chain score (CAND_REC), and for the cigar set the final alignment of the reads that map."""

    def __init__(self, zi=None, z=None, ref=None):
        """the committed fixture, or one recorded just now (record_inputs / run_set)"""
        zi = np.load(INPUTS) if zi is None else zi
        self.sha = zi["inputs_sha256"].tobytes()
        self.n_reads = int(zi["n_reads"])
        self.chunk_first = zi["chunk_first"]      # chunk (r, c) has index chunk_first[r] + c
        self.ev_off, self.events = zi["ev_off"], zi["events"]
        self.hit_off = zi["hit_off"]
        self.hits = np.zeros(len(zi["hit_target"]), [("ref_seq", "<u4"), ("strand", "<i4"), ("target_position", "<u4"), ("query_position", "<u4")])
        self.hits["ref_seq"], self.hits["strand"] = zi["hit_seq"], zi["hit_strand"]
        self.hits["target_position"], self.hits["query_position"] = zi["hit_target"], zi["hit_query"]
        self.z = np.load(ROUNDS) if z is None else z
        self.ref = ref if ref is not None else make_reference()
        self.lens = np.array([len(x) for x in self.ref.forward])

    def n_chunks(self, r):
        return int(self.chunk_first[r + 1] - self.chunk_first[r])

    def chunk(self, r, c):
        """(events, hits as (seq, strand, target, query) tuples): the interface of mapper.SyntheticSeeds"""
        ci = int(self.chunk_first[r]) + c
        ev = self.events[int(self.ev_off[ci]):int(self.ev_off[ci + 1])]
        h = self.hits[int(self.hit_off[ci]):int(self.hit_off[ci + 1])]
        return ev, [(int(x["ref_seq"]), int(x["strand"]), int(x["target_position"]), int(x["query_position"])) for x in h]

    def read_job(self, r):
        from rawalign_amd.mapper import ReadJob

        return ReadJob(f"read_{r}", qlen=self.n_chunks(r) * 4000, n_chunks_available=self.n_chunks(r))

    def key(self, name, form):
        return f"{name}/{form}/"

    def chains(self, name, form, r, rnd):
        """the chains after round rnd (0-based) of read r, and the stop rule's answer"""
        k = self.key(name, form)
        i = int(self.chunk_first[r]) + rnd
        off = self.z[k + "chain_off"]
        return self.z[k + "chains"][int(off[i]):int(off[i + 1])], bool(self.z[k + "mapped"][i])

    def candidates(self, name, form, r, rnd):
        k = self.key(name, form)
        i = int(self.chunk_first[r]) + rnd
        off = self.z[k + "cand_off"]
        return self.z[k + "cands"][int(off[i]):int(off[i + 1])]

    def stop_round(self, name, form, r):
        """0-based round at which the read stops under the default stop rule (None: never maps)"""
        for rnd in range(self.n_chunks(r)):
            if self.chains(name, form, r, rnd)[1]:
                return rnd
        return None


def anchor_gaps(anchors):
    """at / aq of a chain's anchors as float32 bits (rmap.cpp:719-729: uint32 differences of consecutive anchors accumulated in
    float, divided by the number of anchors) -- on the reference's own anchors when the generator records them"""
    a = np.ascontiguousarray(anchors, ra.ANCHOR_DTYPE)
    at = aq = np.float32(0)
    for i in range(len(a) - 1):
        at = np.float32(at + np.float32(np.uint32(a[i]["target_position"]) - np.uint32(a[i + 1]["target_position"])))
        aq = np.float32(aq + np.float32(np.uint32(a[i]["query_position"]) - np.uint32(a[i + 1]["query_position"])))
    n = np.float32(len(a))
    return bits(np.float32(at / n)), bits(np.float32(aq / n))


def chain_rec(d):
    """CHAIN_REC of a chain given as oracle.loader.RefMap.chains gives it, or as a rawalign_amd Chain"""
    rec = np.zeros((), CHAIN_REC)
    rec["at"], rec["aq"] = anchor_gaps(d["anchors"] if isinstance(d, dict) else d.anchors)
    if isinstance(d, dict):
        rec["chaining"], rec["alignment"] = bits(d["chaining_score"]), bits(d["alignment_score"])
        rec["seq"], rec["strand"], rec["mapq"] = d["reference_sequence_index"], d["strand"], d["mapq"]
        rec["start"], rec["end"], rec["n_anchors"] = d["start_position"], d["end_position"], d["n_anchors"]
        rec["digest"] = anchors_digest(d["anchors"])
    else:
        rec["chaining"], rec["alignment"] = bits(d.chaining_score), bits(d.alignment_score)
        rec["seq"], rec["strand"], rec["mapq"] = d.reference_sequence_index, d.strand, getattr(d, "mapq", 0)
        rec["start"], rec["end"], rec["n_anchors"] = d.start_position, d.end_position, d.n_anchors
        rec["digest"] = anchors_digest(d.anchors)
    return rec


def host_candidates(prev_chains, hits, chunk_start, copt, n_seq, sort=True, lists_out=None):
    """The candidate chains of one round from the project's host chaining (rawdtw_chain_anchors list by list with the running
    maximum carried on, rawdtw_sort_by_chaining_score): prev_chains as Chain objects, hits as (seq, strand, target, query in the
    chunk).  In evaluation order when `sort` (rmap.cpp:512), else in the order of rmap.cpp:430-431."""
    from rawalign_amd.align import evaluation_order
    from rawalign_amd.mapper import _SortHelper

    per = {}
    for ch in prev_chains:
        per.setdefault((ch.reference_sequence_index, ch.strand), []).extend(
            (int(a["target_position"]), int(a["query_position"])) for a in ch.anchors)
    for s, st, t, q in hits:
        per.setdefault((s, st), []).append((t, q + chunk_start))
    chains, maxs = [], 0.0
    for s in range(n_seq):
        for st in (0, 1):
            lst = per.get((s, st))
            if not lst:
                continue
            a = np.array(sorted(lst), dtype=[("target_position", "<u4"), ("query_position", "<u4")])
            if lists_out is not None:
                lists_out.append((s, st, a))
            cs, maxs = M.chain_anchors(a.astype(ra.ANCHOR_DTYPE), copt, maxs, s, st)
            chains.extend(cs)
    if sort and chains:
        order = evaluation_order(_SortHelper.get(), [c.chaining_score for c in chains])
        chains = [chains[int(k)] for k in order]
    return chains


# ---- recording (where oracle/_ref/libref_map*.so are) ---------------------------------------------------------------------------
def _refmap():
    from oracle.loader import RefMap

    return RefMap


def as_chain(d):
    ch = ra.Chain(float(d["chaining_score"]), d["reference_sequence_index"], d["strand"], d["anchors"].copy())
    ch.alignment_score = float(d["alignment_score"])
    ch.start_position, ch.end_position = d["start_position"], d["end_position"]
    return ch


def record_inputs(ref, reads):
    rms = [_refmap()(ref.forward, ref.reverse, fused=bool(f)) for f in FORMS]
    chunk_first, ev_off, hit_off, evs, hits = [0], [0], [0], [], []
    for vals in reads:
        cs = chunks_of(vals)
        chunk_first.append(chunk_first[-1] + len(cs))
        for ch in cs:
            h0, h1 = rms[0].hits(ch), rms[1].hits(ch)
            assert np.array_equal(h0, h1), "the two builds seed differently"
            evs.append(ch)
            hits.append(h0)
            ev_off.append(ev_off[-1] + len(ch))
            hit_off.append(hit_off[-1] + len(h0))
    hits = np.concatenate(hits)
    return dict(inputs_sha256=np.frombuffer(inputs_sha256(ref, reads), np.uint8), n_reads=np.int64(len(reads)),
                        chunk_first=np.array(chunk_first, np.int64), ev_off=np.array(ev_off, np.int64), events=np.concatenate(evs).astype(np.float32),
                        hit_off=np.array(hit_off, np.int64), hit_seq=hits[:, 0].astype(np.uint8), hit_strand=hits[:, 1].astype(np.uint8),
                        hit_target=hits[:, 2].astype(np.uint16 if hits[:, 2].max() < 65536 else np.uint32), hit_query=hits[:, 3].astype(np.uint16))


def run_set(fx, ref, name, form, out, cov):
    rm = _refmap()(ref.forward, ref.reverse, fused=bool(form))
    fields = ref_opt_fields(name)
    ro = rm.set_opt(**fields)
    opt, copt = project_opts(name, form)
    stop = M.StopOpt()
    runs_dtw = bool(fields["flag"] & (EVAL | 0x8))
    evaluate = bool(fields["flag"] & EVAL)
    chains_all, chain_off, mapped_all, cands_all, cand_off = [], [0], [], [], [0]
    cig = []
    for r in range(fx.n_reads):
        rid = rm.new_read()
        prev, offset, events, done = [], 0, np.zeros(0, np.float32), False
        for rnd in range(fx.n_chunks(r)):
            ev, hits = fx.chunk(r, rnd)
            events = np.concatenate([events, ev])
            cands, kept = [], None
            if len(ev) >= ro.min_events:
                cands = host_candidates(prev, hits, offset, copt, ref.n_seq, sort=runs_dtw)
                if runs_dtw:
                    best, kept = np.float32(0.0), []
                    for c in cands:                      # rmap.cpp:515-524 with the reference's own align_chain
                        s = rm.align_chain(c.anchors, c.reference_sequence_index, c.strand, events, False, float(best))
                        c.alignment_score = float(s)
                        if s >= np.float32(ro.dtw_min_score):
                            if s > best:
                                best = s
                            kept.append(c)
                        cov["cut"] += int(s == np.float32(-1e10))
                        cov["below"] += int(s != np.float32(-1e10) and s < np.float32(ro.dtw_min_score))
                        cov["kept"] += int(s >= np.float32(ro.dtw_min_score))
                offset += len(ev)
            mapped = rm.round(rid, ev)
            got, off = rm.chains(rid)
            assert off == offset, (name, form, r, rnd, off, offset)
            if len(ev) >= ro.min_events:
                post = kept if evaluate else cands
                want = M.gen_primary_chains(list(post), opt, stop) if post else []
                assert len(want) == len(got), (name, form, r, rnd, len(want), len(got))
                for w, g in zip(want, got):
                    a, b = chain_rec(w), chain_rec(g)
                    if not evaluate:
                        a["alignment"] = b["alignment"]  # (0 in the reference; whatever a scorer left here)
                    assert a == b, (name, form, r, rnd, a, b)
                assert M.is_mapped_with_high_confidence(want, opt, stop) == mapped
                # coverage, by inspection of the candidate list
                sc = [bits(c.chaining_score) for c in cands]
                cov["ties"] += int(len(set(int(x) for x in sc)) < len(sc))
            for g in got:
                chains_all.append(chain_rec(g))
            chain_off.append(len(chains_all))
            mapped_all.append(mapped)
            for c in cands:
                rec = np.zeros((), CAND_REC)
                rec["chaining"], rec["score"] = bits(c.chaining_score), bits(c.alignment_score if runs_dtw else 0.0)
                rec["seq"], rec["strand"], rec["n_anchors"], rec["digest"] = c.reference_sequence_index, c.strand, c.n_anchors, anchors_digest(c.anchors)
                cands_all.append(rec)
            cand_off.append(len(cands_all))
            if mapped and not done:
                done = True
                if fields["flag"] & CIGAR:
                    g0 = got[0]
                    s, (cost, pi, pj, pd) = rm.align_chain(g0["anchors"], g0["reference_sequence_index"], g0["strand"], events, True)
                    cig.append((r, int(bits(s)), int(bits(cost)), len(pi), path_digest(pi, pj, pd)))
            prev = [as_chain(g) for g in got]
    k = fx.key(name, form)
    out[k + "chains"] = np.array(chains_all, CHAIN_REC) if chains_all else np.zeros(0, CHAIN_REC)
    out[k + "chain_off"] = np.array(chain_off, np.int64)
    out[k + "mapped"] = np.array(mapped_all, np.uint8)
    out[k + "cands"] = np.array(cands_all, CAND_REC) if cands_all else np.zeros(0, CAND_REC)
    out[k + "cand_off"] = np.array(cand_off, np.int64)
    if fields["flag"] & CIGAR:
        out[k + "cigar_read"] = np.array([c[0] for c in cig], np.int64)
        out[k + "cigar_alns"] = np.array([c[1] for c in cig], np.uint32)
        out[k + "cigar_cost"] = np.array([c[2] for c in cig], np.uint32)
        out[k + "cigar_len"] = np.array([c[3] for c in cig], np.int64)
        out[k + "cigar_digest"] = np.array([c[4] for c in cig], np.uint8).reshape(len(cig), 8)


# ---- whole raw reads through the reference's own chunk loop (map_worker_for, rmap.cpp:667-822) ------------------------------------
CHUNK_SAMPLES = 4000
# (sequence, strand, first k-mer, k-mers, kind): "junk" = the first chunk from nowhere; None = a read from nowhere; the stretch
# 4000..5000 of sequence 1's forward signal has a noisy copy on sequence 2 (make_reference): competing chains
RAW_SPECS = [(0, 1, 500, 1400, ""), (1, 0, 3000, 900, ""), (2, 1, 200, 1100, ""), (0, 0, 4000, 400, ""), (1, 1, 4100, 1300, ""),
             (2, 0, 1500, 1000, "junk"), (0, 1, 6500, 1250, "junk"), (1, 1, 300, 430, ""), None]
# option sets of the whole-read record, all with --output-chains
WHOLE_SETS = {
    "default": dict(flag=EVAL | OUTCHAINS),
    "noeval": dict(flag=OUTCHAINS),
    "cigar": dict(flag=EVAL | CIGAR | OUTCHAINS),
    "global_full": dict(flag=EVAL | OUTCHAINS, dtw_border_constraint=0, dtw_fill_method=0),
    "frac025": dict(flag=EVAL | OUTCHAINS, dtw_band_radius_frac=0.25),
}
RECORD_KEYS = ("mapped", "ref_id", "read_start_position", "read_end_position", "read_length", "fragment_start_position",
               "fragment_length", "mapq", "rev")


def whole_project_opts(name, form):
    f = WHOLE_SETS[name]
    opt = ra.MapOpt(dtw_border_constraint=f.get("dtw_border_constraint", 1), dtw_fill_method=f.get("dtw_fill_method", 1),
                    dtw_band_radius_frac=f.get("dtw_band_radius_frac", 0.10), flag=f["flag"] & (EVAL | CIGAR), fused_score=bool(form))
    return opt, M.default_chain_opt(E)


def make_raw_reads():
    """raw reads in pA drawn from the genomes behind make_reference (synth.make_genome_raw_reads), some with a chunk from nowhere in
    front, one from nowhere altogether"""
    rng = np.random.default_rng(REF_SEED + 3)
    reads = []
    for k, spec in enumerate(RAW_SPECS):
        if spec is None:
            reads.append((90.0 + 12.0 * rng.normal(0, 1, 9000)).astype(np.float32))
            continue
        s, st, start, n, kind = spec
        g = synth.make_genome(SEQ_LENS[s], REF_SEED + 1000 * s)   # (the genome of synth.make_reference's sequence s)
        sig = synth.make_genome_raw_reads(g, [start], [n], [st], seed=REF_SEED + 10 + k)[0]
        if kind == "junk":
            sig[:CHUNK_SAMPLES] = (90.0 + 12.0 * np.repeat(rng.normal(0, 1, CHUNK_SAMPLES // 8), 8) + rng.normal(0, 1.2, CHUNK_SAMPLES)).astype(np.float32)
        reads.append(sig)
    return reads


def raw_sha256(raws) -> bytes:
    h = hashlib.sha256()
    for x in raws:
        h.update(np.ascontiguousarray(x, "<f4").tobytes())
    return h.digest()


def raw_chunks(sig):
    return [sig[i:i + CHUNK_SAMPLES] for i in range(0, len(sig), CHUNK_SAMPLES)][:30]


def record_whole_reads(ref, raws):
    """per build: every chunk's events (the reference's detect_events) and seed hits; per option set, build and read: the record
    map_worker_for leaves in reg0 and its tags without the wall-clock mt:f:"""
    out = dict(raw_sha256=np.frombuffer(raw_sha256(raws), np.uint8), n_reads=np.int64(len(raws)), l_sig=np.array([len(x) for x in raws], np.int64))
    cf = [0]
    for sig in raws:
        cf.append(cf[-1] + len(raw_chunks(sig)))
    out["chunk_first"] = np.array(cf, np.int64)
    for form in FORMS:
        rm = _refmap()(ref.forward, ref.reverse, fused=bool(form))
        rm.set_opt(flag=EVAL)
        evs, ev_off, hits, hit_off = [], [0], [], [0]
        for sig in raws:
            for ch in raw_chunks(sig):
                ev = rm.detect_events(ch)
                h = rm.hits(ev) if len(ev) else np.zeros((0, 4), np.uint32)
                evs.append(ev)
                hits.append(h)
                ev_off.append(ev_off[-1] + len(ev))
                hit_off.append(hit_off[-1] + len(h))
        hits = np.concatenate(hits)
        k = "%d/" % form
        out[k + "events"], out[k + "ev_off"], out[k + "hit_off"] = np.concatenate(evs).astype(np.float32), np.array(ev_off, np.int64), np.array(hit_off, np.int64)
        out[k + "hit_seq"], out[k + "hit_strand"] = hits[:, 0].astype(np.uint8), hits[:, 1].astype(np.uint8)
        out[k + "hit_target"], out[k + "hit_query"] = hits[:, 2].astype(np.uint16), hits[:, 3].astype(np.uint16)
        for name, fields in WHOLE_SETS.items():
            rm.set_opt(**fields)
            recs, tags = [], []
            for r, sig in enumerate(raws):
                rec = rm.map_read(sig)
                # the events map_worker_for detected itself are the stored ones, chunk by chunk up to where it stopped
                n = len(rec["events"])
                lo = int(out[k + "ev_off"][cf[r]])
                assert np.array_equal(rec["events"].view(np.uint32), out[k + "events"][lo:lo + n].view(np.uint32)) and lo + n in out[k + "ev_off"][cf[r]:cf[r + 1] + 1]
                recs.append([rec[x] for x in RECORD_KEYS])
                tags.append(rec["tags"])
            out["%s/%d/records" % (name, form)] = np.array(recs, np.uint32)
            out["%s/%d/tags" % (name, form)] = np.array(tags)
    return out


class WholeReads:
    """tests/golden/map_ref_reads.npz behind the interface of mapper.SyntheticSeeds, for one build"""

    def __init__(self, form, z=None, ref=None):
        self.z = np.load(READS) if z is None else z
        self.form = form
        self.ref = ref if ref is not None else make_reference()
        self.lens = np.array([len(x) for x in self.ref.forward])
        self.n_reads = int(self.z["n_reads"])
        self.chunk_first = self.z["chunk_first"]
        k = "%d/" % form
        self.ev_off, self.events, self.hit_off = self.z[k + "ev_off"], self.z[k + "events"], self.z[k + "hit_off"]
        self.hits = list(zip(self.z[k + "hit_seq"].tolist(), self.z[k + "hit_strand"].tolist(), self.z[k + "hit_target"].tolist(), self.z[k + "hit_query"].tolist()))

    def n_chunks(self, r):
        return int(self.chunk_first[r + 1] - self.chunk_first[r])

    def chunk(self, r, c):
        ci = int(self.chunk_first[r]) + c
        return self.events[int(self.ev_off[ci]):int(self.ev_off[ci + 1])], self.hits[int(self.hit_off[ci]):int(self.hit_off[ci + 1])]

    def read_job(self, r):
        from rawalign_amd.mapper import ReadJob

        return ReadJob("read_%d" % r, qlen=int(self.z["l_sig"][r]), n_chunks_available=self.n_chunks(r))

    def expected_line(self, name, r):
        """the PAF line the reference prints for the record (rmap.cpp:961-965), with the project's mt:f: (0) in front of the tags"""
        rec = dict(zip(RECORD_KEYS, (int(x) for x in self.z["%s/%d/records" % (name, self.form)][r])))
        tags = "mt:f:0.000000\t" + str(self.z["%s/%d/tags" % (name, self.form)][r])
        if not rec["mapped"]:
            return "read_%d\t%u\t*\t*\t*\t*\t*\t*\t*\t*\t*\t%d\t%s" % (r, rec["read_length"], rec["mapq"], tags)
        fs, fl, rs, re_ = rec["fragment_start_position"], rec["fragment_length"], rec["read_start_position"], rec["read_end_position"]
        return "read_%d\t%u\t%u\t%u\t%s\tseq%d\t%u\t%u\t%u\t%u\t%u\t%d\t%s" % (
            r, rec["read_length"], rs, re_, "-" if rec["rev"] else "+", rec["ref_id"], int(self.lens[rec["ref_id"]]), fs, (fs + fl) & 0xFFFFFFFF,
            (re_ - rs - 1) & 0xFFFFFFFF, fl, rec["mapq"], tags)
