"""The round from signal's entries (include/rawdtw.h: rawdtw_detect_resident_begin / rawdtw_detect_raw_resident_begin /
rawdtw_detect_resident_end, rawdtw_seed_detected_begin, rawdtw_mapper_round_signal_resident / rawdtw_mapper_round_raw_resident,
rawdtw_mapper_signal_stats) without a device: the symbols and their signatures, null arguments, and the refusal of a mapper that
cannot run such a round -- which must leave it untouched."""
import ctypes as C
import os
import re

import numpy as np

from rawalign_amd import mapper
from rawalign_amd._lib import SYMBOLS, EventOpt, load_library
from rawalign_amd.mapping import StopOpt
from rawalign_amd.rawsig import CHANNEL_DTYPE
from rawalign_amd.seeding import SeedIndex
from tests import map_ref_cases as mc
from tests.test_mapper_cpu import _oracle_scorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 5
VP, U64, U32, I32, F32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_float
EO = C.POINTER(EventOpt)
# the declared signatures, written out from the header's C types
DECLARED = {
    "rawdtw_detect_resident_begin": (
        "rawdtw_ctx *ctx, const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *sig_off, const float *sig, "
        "const uint64_t *dst_start, const uint32_t *room, uint64_t events_cap", [VP, EO, U32, VP, VP, VP, VP, U64]),
    "rawdtw_detect_raw_resident_begin": (
        "rawdtw_ctx *ctx, const rawdtw_event_opt_t *opt, uint32_t n_chunks, const uint64_t *raw_off, const int16_t *raw, "
        "const rawdtw_channel_t *chan, const uint64_t *dst_start, const uint32_t *room, uint64_t events_cap", [VP, EO, U32, VP, VP, VP, VP, VP, U64]),
    "rawdtw_detect_resident_end": ("rawdtw_ctx *ctx, uint32_t *s_len, uint32_t *ev_len, uint64_t *total, float *kernel_ms",
                                   [VP, VP, VP, C.POINTER(U64), C.POINTER(F32)]),
    "rawdtw_seed_detected_begin": ("rawdtw_ctx *ctx, uint64_t *hit_off", [VP, VP]),
    "rawdtw_mapper_round_signal_resident": (
        "rawdtw_mapper *m, const rawdtw_seed_index *six, const rawdtw_event_opt_t *ev_opt, uint32_t n_reads, const uint32_t *read_ids, "
        "const uint64_t *sig_off, const float *sig", [VP, VP, EO, U32, VP, VP, VP]),
    "rawdtw_mapper_round_raw_resident": (
        "rawdtw_mapper *m, const rawdtw_seed_index *six, const rawdtw_event_opt_t *ev_opt, uint32_t n_reads, const uint32_t *read_ids, "
        "const uint64_t *raw_off, const int16_t *raw, const rawdtw_channel_t *chan", [VP, VP, EO, U32, VP, VP, VP, VP]),
    "rawdtw_mapper_signal_stats": (
        "const rawdtw_mapper *m, uint64_t *rounds, uint64_t *retried_rounds, uint64_t *sample_bytes_to_device, uint64_t *event_bytes_crossed",
        [VP, VP, VP, VP, VP]),
}


def _norm(s):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", s, flags=re.S)).replace("( ", "(").replace(" )", ")").replace(" ,", ",").strip()


def test_the_signal_entries_exist_with_the_declared_signatures():
    lib = load_library()
    header = _norm(open(os.path.join(ROOT, "include", "rawdtw.h")).read())
    for name, (params, argtypes) in DECLARED.items():
        assert hasattr(lib, name), name
        assert "int %s(%s);" % (name, _norm(params)) in header, name
        res, args = SYMBOLS[name]
        assert res is I32 and args == argtypes, name
    # null handles are refused, not dereferenced
    assert lib.rawdtw_detect_resident_begin(None, None, 0, None, None, None, None, 0) == INVALID
    assert lib.rawdtw_detect_raw_resident_begin(None, None, 0, None, None, None, None, None, 0) == INVALID
    assert lib.rawdtw_detect_resident_end(None, None, None, None, None) == INVALID
    assert lib.rawdtw_seed_detected_begin(None, None) == INVALID
    assert lib.rawdtw_mapper_round_signal_resident(None, None, None, 0, None, None, None) == INVALID
    assert lib.rawdtw_mapper_round_raw_resident(None, None, None, 0, None, None, None, None) == INVALID
    assert lib.rawdtw_mapper_signal_stats(None, None, None, None, None) == INVALID


def test_a_mapper_without_a_context_refuses_both_rounds_and_stays_as_it_was(oracle):
    ref = mc.make_reference()
    six = SeedIndex.from_signals(ref.forward, ref.reverse, threads=3)
    fx = mc.Fixture(ref=ref)
    opt, copt = mc.project_opts("default", 0)
    reads = list(range(0, fx.n_reads, 2))

    def fresh():
        cm = mapper.CMapper(None, opt, StopOpt(), ["seq%d" % s for s in range(len(fx.lens))], [int(x) for x in fx.lens], slot_events=2048,
                            max_reads=fx.n_reads + 1, chain_opt=copt, output_chains=True, threads=2)
        cm.set_scorer(_oracle_scorer(oracle, ref, opt))
        return cm

    cm = fresh()
    want, rounds = mapper.map_reads_c(fx, reads, cm, seed_index=six)
    cm.close()

    cm = fresh()
    lib = cm.lib
    ids = [cm.add_read("read_%d" % r, fx.n_chunks(r) * 4000, fx.n_chunks(r)) for r in reads]
    rid = np.array(ids, np.uint32)
    n = len(rid)
    off = np.arange(n + 1, dtype=np.uint64) * 100
    sig = (90.0 + np.arange(100 * n) % 17).astype(np.float32)
    raw = (500 + np.arange(100 * n) % 17).astype(np.int16)
    chan = np.zeros(n, CHANNEL_DTYPE)
    chan[:] = (8192.0, 1450.0, 3.0)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    # null arguments: RAWDTW_ERR_INVALID, whatever the mapper could have done with them
    assert lib.rawdtw_mapper_round_signal_resident(cm._h, None, None, n, vp(rid), vp(off), vp(sig)) == INVALID
    assert lib.rawdtw_mapper_round_signal_resident(cm._h, six._h, None, n, None, vp(off), vp(sig)) == INVALID
    assert lib.rawdtw_mapper_round_signal_resident(cm._h, six._h, None, n, vp(rid), None, vp(sig)) == INVALID
    assert lib.rawdtw_mapper_round_signal_resident(cm._h, six._h, None, n, vp(rid), vp(off), None) == INVALID
    assert lib.rawdtw_mapper_round_raw_resident(cm._h, six._h, None, n, vp(rid), vp(off), None, vp(chan)) == INVALID
    assert lib.rawdtw_mapper_round_raw_resident(cm._h, six._h, None, n, vp(rid), vp(off), vp(raw), None) == INVALID
    # no context: RAWDTW_ERR_UNSUPPORTED, and the message names the calls that do map the round
    for st in (lib.rawdtw_mapper_round_signal_resident(cm._h, six._h, None, n, vp(rid), vp(off), vp(sig)),
               lib.rawdtw_mapper_round_raw_resident(cm._h, six._h, None, n, vp(rid), vp(off), vp(raw), vp(chan))):
        assert st == UNSUPPORTED
        msg = lib.rawdtw_mapper_last_error(cm._h)
        assert b"rawdtw_detect_raw_begin" in msg and b"rawdtw_mapper_round_seeded_resident" in msg
    assert all(cm.state(i) == (False, 0) for i in ids) and cm.stats()[0] == 0
    assert cm.signal_stats() == dict(rounds=0, retried_rounds=0, sample_bytes_to_device=0, event_bytes_crossed=0)
    assert lib.rawdtw_mapper_signal_stats(cm._h, None, None, None, None) == 0   # (any pointer may be null)
    r = C.c_uint64(7)
    assert lib.rawdtw_mapper_signal_stats(cm._h, None, C.byref(r), None, None) == 0 and r.value == 0
    cm.close()
    # a mapper that saw the refused calls first maps the reads as one that never did
    cm = fresh()
    first = {}
    orig_round = cm.round

    def round_(act, chs, seed_index=None, resident=False):
        if not first:
            a = np.array(act, np.uint32)
            o = np.arange(len(a) + 1, dtype=np.uint64) * 100
            first["st"] = lib.rawdtw_mapper_round_signal_resident(cm._h, seed_index._h, None, len(a), vp(a), vp(o), vp(sig))
        return orig_round(act, chs, seed_index=seed_index)

    cm.round = round_
    got, rounds_g = mapper.map_reads_c(fx, reads, cm, seed_index=six)
    assert first["st"] == UNSUPPORTED and got == want and rounds_g == rounds
    cm.close()


def test_signal_events_cap_reads_back_where_a_context_can_be_made():
    lib = load_library()
    n = I32()
    assert lib.rawdtw_device_count(C.byref(n)) == 0
    ctx = VP()
    if n.value == 0 or lib.rawdtw_create(0, C.byref(ctx)) != 0:
        # no device: the option has nowhere to live; a null context is refused
        v = C.c_int64(5)
        assert lib.rawdtw_get_option(None, b"signal_events_cap", C.byref(v)) == INVALID
        return
    try:
        v = C.c_int64(-1)
        assert lib.rawdtw_get_option(ctx, b"signal_events_cap", C.byref(v)) == 0 and v.value == 0
        assert lib.rawdtw_set_option(ctx, b"signal_events_cap", 12345) == 0
        assert lib.rawdtw_get_option(ctx, b"signal_events_cap", C.byref(v)) == 0 and v.value == 12345
        assert lib.rawdtw_set_option(ctx, b"signal_events_cap", -3) == 0
        assert lib.rawdtw_get_option(ctx, b"signal_events_cap", C.byref(v)) == 0 and v.value == 0
    finally:
        lib.rawdtw_destroy(ctx)
