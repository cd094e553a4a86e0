"""The resident chunk round's entries (include/rawdtw.h: rawdtw_seed_resident_begin / _end / _fetch,
rawdtw_chain_round_begin_resident, rawdtw_mapper_round_seeded_resident, rawdtw_mapper_resident_stats) without a device: the
symbols and their signatures, and the refusal of a mapper that cannot run a resident round -- which must leave it untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rawalign_amd import mapper
from rawalign_amd._lib import SYMBOLS, ChainOpt, load_library
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex
from tests import map_ref_cases as mc
from tests.test_mapper_cpu import _oracle_scorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 5
VP, U64, U32, I32, F32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_float
# the declared signatures, written out from the header's C types
DECLARED = {
    "rawdtw_seed_resident_begin": ("rawdtw_ctx *ctx, uint32_t n_chunks, const uint64_t *ev_start, const uint32_t *ev_len, uint64_t *hit_off",
                                   [VP, U32, VP, VP, VP]),
    "rawdtw_seed_resident_end": ("rawdtw_ctx *ctx, float *kernel_ms", [VP, C.POINTER(F32)]),
    "rawdtw_seed_resident_fetch": ("rawdtw_ctx *ctx, rawdtw_seed_hit_t *hits, uint64_t hits_cap", [VP, VP, U64]),
    "rawdtw_chain_round_begin_resident": (
        "rawdtw_ctx *ctx, const rawdtw_chain_opt_t *opt, uint64_t n_reads, const uint64_t *seed_off, const uint64_t *prev_off, "
        "const rawdtw_seed_t *prev_seeds, const uint32_t *chunk_start, const uint8_t *sits_out, const uint32_t *read_base, uint32_t n_keys, "
        "const uint64_t *key_base, uint64_t *chain_off, uint64_t *anchor_off, rawdtw_chain_rec_t *recs, uint64_t chains_cap, rawdtw_anchor_t *anchors",
        [VP, C.POINTER(ChainOpt), U64, VP, VP, VP, VP, VP, VP, U32, VP, VP, VP, VP, U64, VP]),
    "rawdtw_mapper_round_seeded_resident": (
        "rawdtw_mapper *m, const rawdtw_seed_index *six, uint32_t n_reads, const uint32_t *read_ids, const uint64_t *event_off, const float *events",
        [VP, VP, U32, VP, VP, VP]),
    "rawdtw_mapper_resident_stats": (
        "const rawdtw_mapper *m, uint64_t *resident_rounds, uint64_t *fallback_rounds, uint64_t *hit_bytes_to_host, uint64_t *seed_bytes_to_device",
        [VP, VP, VP, VP, VP]),
}


def _norm(s):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", s, flags=re.S)).replace("( ", "(").replace(" )", ")").strip()


def test_the_resident_entries_exist_with_the_declared_signatures():
    lib = load_library()
    header = _norm(open(os.path.join(ROOT, "include", "rawdtw.h")).read())
    for name, (params, argtypes) in DECLARED.items():
        assert hasattr(lib, name), name
        assert "int %s(%s);" % (name, _norm(params)) in header, name
        res, args = SYMBOLS[name]
        assert res is I32 and args == argtypes, name
    assert lib.rawdtw_abi_version() == 2   # (entries were added; nothing that exists changed)
    # null handles are refused, not dereferenced
    assert lib.rawdtw_seed_resident_begin(None, 0, None, None, None) == INVALID
    assert lib.rawdtw_seed_resident_end(None, None) == INVALID
    assert lib.rawdtw_seed_resident_fetch(None, None, 0) == INVALID
    assert lib.rawdtw_mapper_round_seeded_resident(None, None, 0, None, None, None) == INVALID
    assert lib.rawdtw_mapper_resident_stats(None, None, None, None, None) == INVALID


def _mapper(fx, opt, copt, scorer):
    cm = mapper.CMapper(None, opt, StopOpt(), ["seq%d" % s for s in range(len(fx.lens))], [int(x) for x in fx.lens], slot_events=2048,
                        max_reads=fx.n_reads + 1, chain_opt=copt, output_chains=True, threads=2)
    cm.set_scorer(scorer)
    return cm


def test_a_scorer_only_mapper_refuses_the_resident_round_and_stays_as_it_was(oracle):
    ref = mc.make_reference()
    six = SeedIndex.from_signals(ref.forward, ref.reverse, threads=3)
    fx = mc.Fixture(ref=ref)
    opt, copt = mc.project_opts("default", 0)
    score = _oracle_scorer(oracle, ref, opt)
    reads = list(range(0, fx.n_reads, 2))
    cm = _mapper(fx, opt, copt, score)
    want, rounds = mapper.map_reads_c(fx, reads, cm, seed_index=six)
    cm.close()
    assert sum("\t*\t" not in ln for ln in want) >= len(reads) // 2

    cm = _mapper(fx, opt, copt, score)
    lib = cm.lib
    ids = [cm.add_read("read_%d" % r, fx.n_chunks(r) * 4000, fx.n_chunks(r)) for r in reads]
    chunks = [np.ascontiguousarray(fx.chunk(r, 0)[0], np.float32) for r in reads]
    eoff = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint64)
    ev = np.concatenate(chunks)
    rid = np.array(ids, np.uint32)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert lib.rawdtw_mapper_round_seeded_resident(cm._h, six._h, len(rid), vp(rid), vp(eoff), vp(ev)) == UNSUPPORTED
    assert b"rawdtw_mapper_round_seeded" in lib.rawdtw_mapper_last_error(cm._h)
    assert all(cm.state(i) == (False, 0) for i in ids) and cm.stats()[0] == 0
    assert cm.resident_stats() == dict(resident_rounds=0, fallback_rounds=0, hit_bytes_to_host=0, seed_bytes_to_device=0)
    with pytest.raises(RuntimeError, match="status 5"):
        cm.round(ids, [(c, []) for c in chunks], seed_index=six, resident=True)
    cm.close()
    # the same rounds through _seeded on a mapper that saw the refused call first: the lines of one that never did
    cm = _mapper(fx, opt, copt, score)
    first = {}

    orig_round = cm.round

    def round_(act, chs, seed_index=None, resident=False):
        if not first:
            first["st"] = lib.rawdtw_mapper_round_seeded_resident(
                cm._h, seed_index._h, len(act), vp(np.array(act, np.uint32)),
                vp(np.concatenate([[0], np.cumsum([len(c[0]) for c in chs])]).astype(np.uint64)),
                vp(np.concatenate([np.ascontiguousarray(c[0], np.float32) for c in chs])))
        return orig_round(act, chs, seed_index=seed_index)

    cm.round = round_
    got, rounds_g = mapper.map_reads_c(fx, reads, cm, seed_index=six)
    assert first["st"] == UNSUPPORTED and got == want and rounds_g == rounds
    assert cm.resident_stats()["resident_rounds"] == 0
    cm.close()
