"""Engine: Python face of the C ABI, with the reference's dtw.hpp function names
(src/dtw.hpp:21-29) as methods so that parity tests read like src/check_dtw.cpp."""
from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass

import numpy as np

from ._lib import PlanInfo, RawDTWError, load_library

RAWDTW_FULL = -1

# rawdtw_job_t (include/rawdtw.h), 32 bytes
JOB_DTYPE = np.dtype(
    [
        ("ref_off", "<u8"),
        ("read_off", "<u4"),
        ("n", "<u4"),
        ("m", "<u4"),
        ("band_radius", "<i4"),
        ("exclude_last", "<u4"),
        ("reserved", "<u4"),
    ]
)
assert JOB_DTYPE.itemsize == 32
# ri_anchor_t (src/rmap.h:21-27)
ANCHOR_DTYPE = np.dtype([("target_position", "<u4"), ("query_position", "<u4")])
# rawdtw_chain_rec_t (a chain's record as rawdtw_chain_round leaves it: key = sequence * 2 + strand) and rawdtw_round_out_t
CHAIN_REC_DTYPE = np.dtype([("chaining_score", "<f4"), ("key", "<u4"), ("start_position", "<u4"), ("end_position", "<u4"), ("n_anchors", "<u4")])
ROUND_OUT_DTYPE = np.dtype([("n_primary", "<u4"), ("mapq", "<u4"), ("flags", "<u4")])
ROUND_HIGH, ROUND_DECLINED, NO_PRIMARY = 1, 2, 0xFFFFFFFF
# rawdtw_seed_t (a chaining seed: key = sequence * 2 + strand) and the kept chains' sentinels (include/rawdtw.h)
SEED_DTYPE = np.dtype([("key", "<u4"), ("target_position", "<u4"), ("query_position", "<u4")])
NOT_KEPT = NO_KEEP = PREV_HOST = 0xFFFFFFFF


@dataclass
class DtwResult:
    """dtw_result (src/dtw.hpp:16-19): cost + alignment as (i, j, difference) columns."""

    cost: np.float32
    i: np.ndarray
    j: np.ndarray
    difference: np.ndarray

    def __len__(self):
        return len(self.i)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _f32(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32)


def _round_end(lib, ctx, check, select_opt, chain_off, recs, score, keep):
    chain_off = np.ascontiguousarray(chain_off, np.uint64)
    n, nc = len(chain_off) - 1, int(chain_off[-1])
    recs, score = np.ascontiguousarray(recs, CHAIN_REC_DTYPE), np.ascontiguousarray(score, np.float32)
    keep = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    if len(recs) < nc or len(score) < nc or (keep is not None and len(keep) < nc):
        raise ValueError("recs, score and keep hold chain_off[-1] chains")
    out, primary = np.zeros(max(n, 1), ROUND_OUT_DTYPE), np.zeros(max(nc, 1), np.uint32)
    args = (C.byref(select_opt), n, _ptr(chain_off), _ptr(recs), _ptr(score), _ptr(keep) if keep is not None else None, _ptr(out), _ptr(primary))
    check(lib.rawdtw_round_end_host(*args) if ctx is None else lib.rawdtw_round_end(ctx, *args))
    return out[:n], primary[:nc]


def round_end_host(select_opt, chain_off, recs, score, keep=None):
    """rawdtw_round_end_host: the host restatement of Engine.round_end (never declines); no device is touched"""
    def check(st):
        if st != 0:
            raise RawDTWError(st, "rawdtw_round_end_host")
    return _round_end(load_library(), None, check, select_opt, chain_off, recs, score, keep)


def _keep_arrays(chain_off, recs, anchor_off, anchors, out, primary):
    chain_off = np.ascontiguousarray(chain_off, np.uint64)
    n, nc = len(chain_off) - 1, int(chain_off[-1])
    recs, anchor_off = np.ascontiguousarray(recs, CHAIN_REC_DTYPE), np.ascontiguousarray(anchor_off, np.uint64)
    anchors, out, primary = np.ascontiguousarray(anchors, ANCHOR_DTYPE), np.ascontiguousarray(out, ROUND_OUT_DTYPE), np.ascontiguousarray(primary, np.uint32)
    if len(recs) < nc or len(primary) < nc or len(anchor_off) < nc + 1 or len(out) < n or len(anchors) < int(anchor_off[nc]):
        raise ValueError("recs and primary hold chain_off[-1] chains, anchor_off one more, out a read, anchors anchor_off[-1]")
    return n, nc, chain_off, recs, anchor_off, anchors, out, primary


def round_keep_host(chain_off, recs, anchor_off, anchors, out, primary, cap):
    """rawdtw_round_keep_host: what a round keeps as the next round's previous seeds, on the host: (kept_count: uint32 a read, NOT_KEPT for
    a declined read and one above `cap`; seed_off: uint64, n + 1; seeds: SEED_DTYPE, the kept reads' lists, dense)"""
    n, nc, chain_off, recs, anchor_off, anchors, out, primary = _keep_arrays(chain_off, recs, anchor_off, anchors, out, primary)
    kept, soff, seeds = np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.uint64), np.zeros(max(int(anchor_off[nc]), 1), SEED_DTYPE)
    st = load_library().rawdtw_round_keep_host(n, _ptr(chain_off), _ptr(recs), _ptr(anchor_off), _ptr(anchors), _ptr(out), _ptr(primary), int(cap),
                                               _ptr(kept), _ptr(soff), _ptr(seeds))
    if st != 0:
        raise RawDTWError(st, "rawdtw_round_keep_host")
    return kept[:n], soff, seeds[:int(soff[n])]


def chain_decline_host(chain_opt, per_read, seed_cap: int = 0, long_seeds: int = 0, max_chains: int = 0):
    """rawdtw_chain_decline_host: which reads of a round (`per_read`: a SEED_DTYPE array a read) the device chaining declines under
    "chain_decline_reads", and why, without a device.  chain_opt: a ChainOpt (mapping.default_chain_opt); seed_cap: the cap on seeds a read
    (0: 2 048; the tests' RAWDTW_CHAIN_MAX_SEEDS); long_seeds, max_chains: the context's "chain_long_seeds" and "chain_max_chains".
    Returns (why: uint32 a read -- 0 chained, bit 1 seeds, 2 chains, 4 ties --, n_chains: uint32 a read)."""
    n = len(per_read)
    seed_off = np.zeros(n + 1, np.uint64)
    seed_off[1:] = np.cumsum([len(s) for s in per_read])
    seeds = np.ascontiguousarray(np.concatenate([np.asarray(s, SEED_DTYPE) for s in per_read] + [np.zeros(1, SEED_DTYPE)]))
    why, n_chains = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    st = load_library().rawdtw_chain_decline_host(C.byref(chain_opt), n, _ptr(seed_off), _ptr(seeds), int(seed_cap), int(long_seeds), int(max_chains),
                                                  _ptr(why), _ptr(n_chains))
    if st != 0:
        raise RawDTWError(st, "rawdtw_chain_decline_host")
    return why[:n], n_chains[:n]


def plan_dry_run(jobs: np.ndarray, n_events: int, n_reference: int, threads: int = 0, options=None):
    """Host half of plan creation only (include/rawdtw.h: rawdtw_plan_dry_run): bins `jobs`, checks the plan's
    invariants and returns (info dict, n_tiles).  Touches no device and scores nothing."""
    lib = load_library()
    jobs = np.ascontiguousarray(jobs, JOB_DTYPE)
    options = dict(options or {})
    names = (C.c_char_p * max(len(options), 1))(*[k.encode() for k in options])
    vals = (C.c_int64 * max(len(options), 1))(*[int(v) for v in options.values()])
    info = PlanInfo()
    n_tiles = C.c_uint64()
    msg = C.create_string_buffer(512)
    st = lib.rawdtw_plan_dry_run(int(n_events), int(n_reference), _ptr(jobs), len(jobs), int(threads),
                                 C.cast(names, C.c_void_p), C.cast(vals, C.c_void_p), len(options), C.byref(info),
                                 C.byref(n_tiles), C.cast(msg, C.c_void_p), 512)
    if st != 0:
        raise RawDTWError(st, msg.value.decode())
    return {f: getattr(info, f) for f, _ in PlanInfo._fields_}, int(n_tiles.value)


class Plan:
    """A size-binned batch resident on the device (rawdtw_plan)."""

    def __init__(self, engine: "Engine", handle, n_jobs: int):
        self.engine = engine
        self._h = handle
        self.n_jobs = n_jobs
        engine._children.add(self)

    def info(self) -> dict:
        pi = PlanInfo()
        self.engine._check(self.engine.lib.rawdtw_plan_info(self._h, C.byref(pi)))
        return {k: int(getattr(pi, k)) for k, _ in PlanInfo._fields_}

    def run(self):
        self.engine._check(self.engine.lib.rawdtw_plan_run(self.engine._ctx, self._h))

    def run_timed(self):
        """Run once with a HIP event around every launch (on the engine's stream).
        Returns [(kind, param, ms), ...]."""
        n = self.info()["n_launches"]
        ms = np.zeros(max(n, 1), np.float32)
        kind = np.zeros(max(n, 1), np.uint32)
        self.engine._check(
            self.engine.lib.rawdtw_plan_run_timed(self.engine._ctx, self._h, _ptr(ms), _ptr(kind), n)
        )
        return [(int(kind[k] & 0xFF), int(kind[k] >> 8), float(ms[k])) for k in range(n)]

    def fetch(self) -> np.ndarray:
        out = np.empty(self.n_jobs, np.float32)
        self.engine._check(self.engine.lib.rawdtw_plan_fetch(self.engine._ctx, self._h, _ptr(out)))
        return out

    def close(self):
        if self._h is not None:
            self.engine.lib.rawdtw_plan_destroy(self._h)  # (safe in any order: rawdtw_destroy detaches live plans)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResidentSeeding:
    """An ended resident seeding of an Engine (Engine.seed_resident): its hit offsets; the hits are on the device."""

    def __init__(self, engine, hit_off, kernel_ms):
        self.engine, self.hit_off, self.kernel_ms = engine, hit_off, kernel_ms

    def fetch(self, pinned: bool = True):
        """the hits as seeding.HIT_DTYPE, in rawdtw_seed_begin's order (valid until the engine's next seeding)"""
        from .events import PinnedArray
        from .seeding import HIT_DTYPE

        n = int(self.hit_off[-1])
        keep = PinnedArray(n, HIT_DTYPE) if pinned else None
        hits = keep.array if pinned else np.zeros(max(n, 1), HIT_DTYPE)
        self.engine._check(self.engine.lib.rawdtw_seed_resident_fetch(self.engine._ctx, hits.ctypes.data, n))
        return hits[:n].copy()


class ResidentDetection:
    """A resident detection begun on an Engine (Engine.detect_resident(..., wait=False)): end() waits and returns what came home."""

    def __init__(self, engine, n, keep):
        self.engine, self.n, self._keep = engine, n, keep

    def end(self, kernel_ms: bool = False):
        """rawdtw_detect_resident_end: (ev_len, s_len, total), and the launches' device time in ms too when kernel_ms.  A declined
        detection (a chunk over its room, or the total over events_cap) raises RawDTWError with ev_len, s_len and total set on it."""
        e = self.engine
        ev_len, s_len = np.zeros(max(self.n, 1), np.uint32), np.zeros(max(self.n, 1), np.uint32)
        total, ms = C.c_uint64(), C.c_float()
        st = e.lib.rawdtw_detect_resident_end(e._ctx, _ptr(s_len), _ptr(ev_len), C.byref(total), C.byref(ms))
        self._keep = None
        if st != 0:
            err = RawDTWError(st, e.lib.rawdtw_last_error(e._ctx).decode())
            err.ev_len, err.s_len, err.total = ev_len[:self.n], s_len[:self.n], int(total.value)
            raise err
        out = (ev_len[:self.n], s_len[:self.n], int(total.value))
        return out + (float(ms.value),) if kernel_ms else out


class DetectedSeeding:
    """A seeding begun behind a resident detection (Engine.seed_detected(wait=False)): end() waits and returns the ResidentSeeding."""

    def __init__(self, engine, hit_off):
        self.engine, self.hit_off = engine, hit_off

    def end(self):
        e = self.engine
        ms = C.c_float()
        e._check(e.lib.rawdtw_seed_resident_end(e._ctx, C.byref(ms)))
        return ResidentSeeding(e, self.hit_off, float(ms.value))


class Engine:
    """One rawdtw_ctx (one HIP device, one stream)."""

    KIND_NAMES = {1: "band_lane", 2: "band_wave_lds", 3: "full_wave", 4: "full_tb", 5: "tb_walk", 6: "chain_fold",
                  7: "read_select", 8: "band_wreg", 9: "band_lane_hi", 10: "band_merged", 11: "semi_wave"}

    def __init__(self, device: int = 0):
        self.lib = load_library()
        ctx = C.c_void_p()
        st = self.lib.rawdtw_create(int(device), C.byref(ctx))
        if st != 0:
            raise RawDTWError(st, self.lib.rawdtw_status_string(st).decode())
        self._ctx = ctx
        self.device = device
        self._keep = []  # arrays / tensors the context points at
        # plans and batches of this context: closed with it, so that their device memory goes back at a known point (the
        # C ABI itself tolerates any order: rawdtw_destroy detaches what is still alive)
        self._children = weakref.WeakSet()

    # -- plumbing ---------------------------------------------------------------
    def _check(self, st: int):
        if st != 0:
            raise RawDTWError(st, self.lib.rawdtw_last_error(self._ctx).decode() or
                              self.lib.rawdtw_status_string(st).decode())

    def close(self):
        if getattr(self, "_ctx", None) is not None:
            for child in list(self._children):
                child.close()
            self.lib.rawdtw_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(self.lib.rawdtw_sync(self._ctx))

    def set_option(self, name: str, value: int):
        self._check(self.lib.rawdtw_set_option(self._ctx, name.encode(), int(value)))

    def set_border_local(self, on: bool = True):
        """rawdtw_set_border_local: the batch entry points and rawdtw_mapper_create on this context accept border constraint 2 (local:
        include/rawdtw.h, "local border").  A setter, not an option; off by default."""
        self._check(self.lib.rawdtw_set_border_local(self._ctx, int(bool(on))))

    def get_border_local(self) -> bool:
        v = C.c_int()
        self._check(self.lib.rawdtw_get_border_local(self._ctx, C.byref(v)))
        return bool(v.value)

    def set_semiglobal_window(self, columns: int = 0):
        """rawdtw_set_semiglobal_window: semiglobal tracebacks on this context (semiglobal_traceback, DTW_semiglobal_tb, a mapper's local
        finish) keep one window of `columns` columns of directions a job and checkpoint columns in place of n x m directions
        (include/rawdtw.h, "semiglobal, in windows").  0: off, the default; else a multiple of 64 in [64, 2^20]."""
        if not 0 <= int(columns) < 1 << 32:
            raise RawDTWError(1, "semiglobal window: 0 or a multiple of 64 in [64, 2^20]")
        self._check(self.lib.rawdtw_set_semiglobal_window(self._ctx, int(columns)))

    def get_semiglobal_window(self) -> int:
        v = C.c_uint32()
        self._check(self.lib.rawdtw_get_semiglobal_window(self._ctx, C.byref(v)))
        return int(v.value)

    def semiglobal_window_stats(self) -> dict:
        """rawdtw_semiglobal_window_stats of the context's most recent semiglobal traceback call"""
        j, w, mx, ck = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.rawdtw_semiglobal_window_stats(self._ctx, C.byref(j), C.byref(w), C.byref(mx), C.byref(ck)))
        return {"jobs_windowed": j.value, "windows": w.value, "max_windows_a_job": mx.value, "checkpoint_bytes": ck.value}

    def get_option(self, name: str) -> int:
        """rawdtw_get_option: any option of include/rawdtw.h's option block -- a settable one as it is stored (what set_option made of its
        value, or the default), and the read-only "tb_sub_batches", "round_end_kernel_us" and "round_keep_kernel_us" """
        v = C.c_int64()
        self._check(self.lib.rawdtw_get_option(self._ctx, name.encode(), C.byref(v)))
        return int(v.value)

    def chain_round_stats(self) -> dict:
        """rawdtw_chain_round_stats: chaining rounds begun on this context, the reads and seeds its long path ("chain_long_seeds") chained, and
        the long path's 64-candidate steps that read beyond its LDS ring -- cumulative"""
        v = [C.c_uint64() for _ in range(4)]
        self._check(self.lib.rawdtw_chain_round_stats(self._ctx, *[C.byref(x) for x in v]))
        return dict(zip(("rounds", "long_reads", "long_seeds", "far_steps"), (int(x.value) for x in v)))

    def chain_order_stats(self) -> dict:
        """rawdtw_chain_order_stats: over this context's chaining rounds that were not declined, the reads with more than 32 chains, the reads
        with more than 16 that "chain_max_chains" ordered with the restated std::sort, and the most chains a read had -- cumulative"""
        v = [C.c_uint64() for _ in range(3)]
        self._check(self.lib.rawdtw_chain_order_stats(self._ctx, *[C.byref(x) for x in v]))
        return dict(zip(("reads_above_32", "reads_ordered_restated", "max_chains_a_read"), (int(x.value) for x in v)))

    def chain_round_declined(self):
        """rawdtw_chain_round_declined: (reads, why) of the ended chaining round -- the reads "chain_decline_reads" declined alone, ascending,
        and their reasons' bits (1 seeds, 2 chains, 4 an order only std::sort knows); copies.  Empty with the option off."""
        n, reads, why = C.c_uint64(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.rawdtw_chain_round_declined(self._ctx, C.byref(n), C.byref(reads), C.byref(why)))
        if not n.value:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        get = lambda p: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n.value,)).copy()  # noqa: E731
        return get(reads), get(why)

    def chain_round_declined_seeds(self, cap=None):
        """rawdtw_chain_round_declined_seeds: (seed_off, seeds as SEED_DTYPE) of the declined reads, from the device's seed list.  cap: the
        array's size in seeds (default: what the reads need; a smaller one raises with the status RAWDTW_ERR_RANGE)."""
        reads, _ = self.chain_round_declined()
        seed_off = np.zeros(len(reads) + 1, np.uint64)
        if cap is None:  # (the offsets are filled whatever the cap)
            st = self.lib.rawdtw_chain_round_declined_seeds(self._ctx, _ptr(seed_off), None, 0)
            if st not in (0, 4):
                self._check(st)
            cap = int(seed_off[-1])
        seeds = np.zeros(max(int(cap), 1), SEED_DTYPE)
        self._check(self.lib.rawdtw_chain_round_declined_seeds(self._ctx, _ptr(seed_off), _ptr(seeds), int(cap)))
        return seed_off, seeds[:int(seed_off[-1])]

    def chain_round_append(self, n_reads: int, n_chains: int, chain_off, recs, anchor_off, anchors):
        """rawdtw_chain_round_append: the host's chains of the declined reads (chain_off / anchor_off from 0, CHAIN_REC_DTYPE records, anchors
        end-first) behind the round's own n_chains in device memory.  Returns (chain_off_ext of n_reads + n_declined + 1 entries,
        anchor_off_ext of n_chains + the appended chains + 1, (d_anchors, d_ref_base, d_read_base)): what rawdtw_batch_submit_device takes."""
        chain_off, anchor_off = np.ascontiguousarray(chain_off, np.uint64), np.ascontiguousarray(anchor_off, np.uint64)
        recs, anchors = np.ascontiguousarray(recs), np.ascontiguousarray(anchors)
        n = len(chain_off) - 1
        ext, aext = np.zeros(int(n_reads) + n + 1, np.uint64), np.zeros(int(n_chains) + int(chain_off[-1]) + 1, np.uint64)
        d = [C.c_void_p() for _ in range(3)]
        self._check(self.lib.rawdtw_chain_round_append(self._ctx, n, _ptr(chain_off), _ptr(recs), _ptr(anchor_off), _ptr(anchors), _ptr(ext), _ptr(aext),
                                                       *[C.byref(x) for x in d]))
        return ext, aext, tuple(d)

    def round_end(self, select_opt, chain_off, recs, score, keep=None):
        """rawdtw_round_end: gen_primary_chains, comp_mapq and the stop rule for every read of a round in one launch.  `select_opt` is a
        SelectOpt (mapping.StopOpt.c_struct); read r's candidates are [chain_off[r], chain_off[r+1]) of recs (CHAIN_REC_DTYPE), score and
        keep.  Returns (out: ROUND_OUT_DTYPE a read, primary: uint32 a chain); a read with flag ROUND_DECLINED is the caller's to end with
        round_end_host."""
        return _round_end(self.lib, self._ctx, self._check, select_opt, chain_off, recs, score, keep)

    def chain_keep_reserve(self, n_slots: int, seeds_per_half: int):
        """rawdtw_chain_keep_reserve: the context's store of kept chains, grow-only (a store that grows loses its contents)"""
        self._check(self.lib.rawdtw_chain_keep_reserve(self._ctx, int(n_slots), int(seeds_per_half)))

    def round_keep(self, chain_off, recs, anchor_off, anchors, out, primary, dst):
        """rawdtw_round_keep: the host arrays go up, one launch keeps read r's primary chains' anchors as seeds in the store's half dst[r]
        (NO_KEEP: nowhere).  Returns kept_count (uint32 a read; NOT_KEPT: declined, above the store's seeds a half, or no destination)."""
        n, nc, chain_off, recs, anchor_off, anchors, out, primary = _keep_arrays(chain_off, recs, anchor_off, anchors, out, primary)
        dst = np.ascontiguousarray(dst, np.uint32)
        if len(dst) < n:
            raise ValueError("dst holds an entry a read")
        kept = np.zeros(max(n, 1), np.uint32)
        self._check(self.lib.rawdtw_round_keep(self._ctx, n, _ptr(chain_off), _ptr(recs), _ptr(anchor_off), _ptr(anchors), _ptr(out), _ptr(primary), _ptr(dst),
                                               _ptr(kept)))
        return kept[:n]

    def chain_kept_fetch(self, addr: int, cap: int):
        """rawdtw_chain_kept_fetch: (the half's count, NOT_KEPT included; its first `cap` seeds as SEED_DTYPE, whatever the count says)"""
        seeds, n = np.zeros(max(int(cap), 1), SEED_DTYPE), C.c_uint32()
        self._check(self.lib.rawdtw_chain_kept_fetch(self._ctx, int(addr), _ptr(seeds), int(cap), C.byref(n)))
        return n.value, seeds[:int(cap)]

    def chain_round_recs(self) -> int:
        """rawdtw_chain_round_recs: the device address of the ended chaining round's records (valid until the next chaining round)"""
        p = C.c_void_p()
        self._check(self.lib.rawdtw_chain_round_recs(self._ctx, C.byref(p)))
        return p.value or 0

    def stream_handle(self) -> int:
        s = C.c_void_p()
        self._check(self.lib.rawdtw_stream(self._ctx, C.byref(s)))
        return s.value or 0

    # -- arenas -----------------------------------------------------------------
    def upload_reference(self, forward_signals, reverse_signals):
        """ri_idx_t.forward_signals / reverse_signals (src/rawindex.h:32-34), one array per sequence."""
        fwd = [_f32(x) for x in forward_signals]
        rev = [_f32(x) for x in reverse_signals]
        assert len(fwd) == len(rev) and all(len(f) == len(r) for f, r in zip(fwd, rev))
        n = len(fwd)
        fp = (C.c_void_p * n)(*[x.ctypes.data for x in fwd])
        rp = (C.c_void_p * n)(*[x.ctypes.data for x in rev])
        ln = np.array([len(x) for x in fwd], np.uint32)
        self._check(self.lib.rawdtw_upload_reference(self._ctx, n, fp, rp, _ptr(ln)))

    def reference_offset(self, seq: int, strand: int) -> int:
        off = C.c_uint64()
        self._check(self.lib.rawdtw_reference_offset(self._ctx, seq, strand, C.byref(off)))
        return off.value

    def reference_from_bases(self, seqs, pore, k: int, contracted: bool = True):
        """rawdtw_reference_from_bases: upload_reference from bases (str, bytes or uint8 arrays) and a model of 4^k levels -- ri_seq_to_sig
        for both strands of every sequence on the device, straight into the arena"""
        from .refsig import as_bases

        b = [as_bases(s) for s in seqs]
        pore = _f32(pore)
        if len(pore) < 4 ** int(k) and 1 <= int(k) <= 12:
            raise ValueError("the model has 4^k levels")
        n = len(b)
        bp = (C.c_void_p * max(n, 1))(*[x.ctypes.data for x in b])
        ln = np.array([len(x) for x in b] or [0], np.uint64)
        self._check(self.lib.rawdtw_reference_from_bases(self._ctx, n, bp, _ptr(ln), _ptr(pore), int(k), int(bool(contracted))))
        self._ref_lens = [max(len(x) - int(k) + 1, 0) for x in b]

    def reference_fetch(self, seq: int, strand: int, length=None) -> np.ndarray:
        """rawdtw_reference_fetch: one strand of the context's reference (`length`: the strand's, where the reference did not come
        from reference_from_bases)"""
        if length is None:
            length = self._ref_lens[seq]
        out = np.zeros(max(int(length), 1), np.float32)
        self._check(self.lib.rawdtw_reference_fetch(self._ctx, int(seq), int(strand), _ptr(out), int(length)))
        return out[:int(length)]

    def reference_build_stats(self) -> dict:
        """rawdtw_reference_build_stats: the most recent reference_from_bases -- steps of sum [0] and sum2 [1] that went fast and slow,
        and the two launches' device time"""
        fast, slow, ms = np.zeros(2, np.uint64), np.zeros(2, np.uint64), np.zeros(2, np.float32)
        self._check(self.lib.rawdtw_reference_build_stats(self._ctx, _ptr(fast), _ptr(slow), _ptr(ms)))
        return {"fast_steps": fast, "slow_steps": slow, "sums_ms": float(ms[0]), "write_ms": float(ms[1])}

    def seed_build_stats(self) -> dict:
        """rawdtw_seed_index_build_stats: the phases of the most recent SeedIndex.from_device on this engine, in ms"""
        ms = np.zeros(5, np.float32)
        self._check(self.lib.rawdtw_seed_index_build_stats(self._ctx, _ptr(ms)))
        return dict(zip(("filter_ms", "emit_ms", "sort_ms", "home_ms", "fill_table_ms"), (float(x) for x in ms)))

    def seed_build_min_stats(self) -> dict:
        """rawdtw_seed_index_build_min_stats: the most recent SeedIndex.from_device(minimizer=True) with w > 0 on this engine -- e-mers over
        all strands, entries emitted, and the device time of the hash, count + scan and write launches in ms"""
        emers, entries, ms = C.c_uint64(), C.c_uint64(), np.zeros(3, np.float32)
        self._check(self.lib.rawdtw_seed_index_build_min_stats(self._ctx, C.byref(emers), C.byref(entries), _ptr(ms)))
        return {"emers": emers.value, "entries": entries.value, "hash_ms": float(ms[0]), "count_scan_ms": float(ms[1]), "write_ms": float(ms[2])}

    def seed_build_resident_stats(self) -> dict:
        """rawdtw_seed_index_build_resident_stats: the most recent SeedIndex.from_device(resident=True) or from_entries(engine=...) on
        this engine -- the filter's tile size and tiles, kept events, entries, keys, the keys not in their home slot, and device ms"""
        from ._lib import SeedResidentStats

        st = SeedResidentStats()
        self._check(self.lib.rawdtw_seed_index_build_resident_stats(self._ctx, C.byref(st)))
        return {name: getattr(st, name) for name, _ in SeedResidentStats._fields_}

    def set_reference_device(self, data_ptr: int, n_floats: int, keepalive=None):
        self._check(self.lib.rawdtw_set_reference_device(self._ctx, C.c_void_p(data_ptr), n_floats))
        self._keep_ref = keepalive

    def upload_events(self, events):
        ev = _f32(events)
        self._check(self.lib.rawdtw_upload_events(self._ctx, _ptr(ev), len(ev)))

    def set_events_device(self, data_ptr: int, n_floats: int, keepalive=None):
        self._check(self.lib.rawdtw_set_events_device(self._ctx, C.c_void_p(data_ptr), n_floats))
        self._keep_ev = keepalive

    # -- event detection (detect_events, src/revent.c:190-210) ---------------------
    def detect_events(self, sig, sig_off, opt=None, pinned: bool = True, events_cap=None, kernel_ms: bool = False):
        """Every chunk k = sig[sig_off[k] .. sig_off[k+1]) on the device: rawdtw_detect_begin, then _end.  The samples go up
        from, and the results come back into, page-locked staging that the engine keeps (pinned=False: pageable arrays, which
        _end copies into).  Returns (event_off, events), and the launches' device time in ms too when kernel_ms."""
        from .events import PinnedArray, _opt

        sig = np.asarray(sig, np.float32)
        off = np.ascontiguousarray(sig_off, np.uint64)
        n = len(off) - 1
        cap = int(off[-1]) if events_cap is None else int(events_cap)
        if pinned:
            st = getattr(self, "_ev_stage", None)
            if st is None or st["sig"].array.size < len(sig) or st["off"].array.size < n + 1 or st["ev"].array.size < cap:
                st = self._ev_stage = {"sig": PinnedArray(len(sig), np.float32), "off": PinnedArray(n + 1, np.uint64),
                                       "eoff": PinnedArray(n + 1, np.uint64), "ev": PinnedArray(cap, np.float32)}
            if st["eoff"].array.size < n + 1:
                st["eoff"] = PinnedArray(n + 1, np.uint64)
            h_sig, h_off, eoff, ev = st["sig"].array, st["off"].array, st["eoff"].array, st["ev"].array
            h_sig[:len(sig)] = sig
            h_off[:n + 1] = off
        else:
            h_sig, h_off = np.ascontiguousarray(sig), off
            eoff, ev = np.zeros(n + 1, np.uint64), np.empty(max(cap, 1), np.float32)
        ms = C.c_float()
        self._check(self.lib.rawdtw_detect_begin(self._ctx, _opt(opt), n, h_off.ctypes.data, h_sig.ctypes.data, eoff.ctypes.data,
                                                 ev.ctypes.data, cap))
        st = self.lib.rawdtw_detect_end(self._ctx, C.byref(ms))
        if st != 0:
            err = RawDTWError(st, self.lib.rawdtw_last_error(self._ctx).decode())
            err.event_off = eoff[:n + 1].copy()
            raise err
        out = (eoff[:n + 1].copy(), ev[:int(eoff[n])].copy())
        return out + (float(ms.value),) if kernel_ms else out

    def detect_events_raw(self, raw, raw_off, chan, opt=None, pinned: bool = True, events_cap=None, kernel_ms: bool = False):
        """Every window k = raw[raw_off[k] .. raw_off[k+1]) of int16 DAC samples with channel chan[k] on the device:
        rawdtw_detect_raw_begin (pA conversion and outlier filter of src/rsig.cpp:216-224, then the detection), then _end.
        Staging as detect_events keeps it.  Returns (s_len, event_off, events), and the launches' device time in ms too when
        kernel_ms."""
        from .events import PinnedArray, _opt
        from .rawsig import CHANNEL_DTYPE, channels

        raw = np.asarray(raw, np.int16)
        off = np.ascontiguousarray(raw_off, np.uint64)
        n = len(off) - 1
        ch = channels(chan, n)
        cap = int(off[-1] - off[0]) if events_cap is None else int(events_cap)
        if pinned:
            st = getattr(self, "_raw_stage", None)
            if st is None or st["raw"].array.size < len(raw) or st["off"].array.size < n + 1 or st["ev"].array.size < cap:
                st = self._raw_stage = {"raw": PinnedArray(len(raw), np.int16), "off": PinnedArray(n + 1, np.uint64),
                                        "chan": PinnedArray(n, CHANNEL_DTYPE), "slen": PinnedArray(n, np.uint32),
                                        "eoff": PinnedArray(n + 1, np.uint64), "ev": PinnedArray(cap, np.float32)}
            h_raw, h_off, h_ch = st["raw"].array, st["off"].array, st["chan"].array
            s_len, eoff, ev = st["slen"].array, st["eoff"].array, st["ev"].array
            h_raw[:len(raw)] = raw
            h_off[:n + 1] = off
            h_ch[:n] = ch
        else:
            h_raw, h_off, h_ch = np.ascontiguousarray(raw), off, ch
            s_len, eoff, ev = np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.uint64), np.empty(max(cap, 1), np.float32)
        ms = C.c_float()
        self._check(self.lib.rawdtw_detect_raw_begin(self._ctx, _opt(opt), n, h_off.ctypes.data, h_raw.ctypes.data, h_ch.ctypes.data,
                                                     s_len.ctypes.data, eoff.ctypes.data, ev.ctypes.data, cap))
        st = self.lib.rawdtw_detect_end(self._ctx, C.byref(ms))
        if st != 0:
            err = RawDTWError(st, self.lib.rawdtw_last_error(self._ctx).decode())
            err.event_off, err.s_len = eoff[:n + 1].copy(), s_len[:n].copy()
            raise err
        out = (s_len[:n].copy(), eoff[:n + 1].copy(), ev[:int(eoff[n])].copy())
        return out + (float(ms.value),) if kernel_ms else out

    def detect_resident(self, data, off, dst_start, room, chan=None, opt=None, events_cap=None, wait: bool = True):
        """Detection whose events stay on the device: window k = data[off[k] .. off[k+1]) -- pA samples (float32), or with `chan` int16
        DAC samples and a channel a window -- is detected into the context's event arena at dst_start[k] .., at most room[k] events
        (rawdtw_detect_resident_begin / rawdtw_detect_raw_resident_begin).  All or nothing: a chunk over its room, or a total above
        events_cap (None: the samples' count, which always suffices), writes nothing and raises RawDTWError (status 4) from the end with
        ev_len, s_len and total set on it.  Returns (ev_len, s_len, total); wait=False: a ResidentDetection to end() later, so that
        seed_detected can be enqueued behind it first."""
        from .events import _opt

        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        dst, rm = np.ascontiguousarray(dst_start, np.uint64), np.ascontiguousarray(room, np.uint32)
        if len(dst) != n or len(rm) != n:
            raise ValueError("dst_start and room need one entry a window")
        cap = int(off[-1] - off[0]) if events_cap is None else int(events_cap)
        if chan is None:
            data = np.ascontiguousarray(data, np.float32)
            self._check(self.lib.rawdtw_detect_resident_begin(self._ctx, _opt(opt), n, _ptr(off), _ptr(data), _ptr(dst), _ptr(rm), cap))
            keep = (off, data, dst, rm)
        else:
            from .rawsig import channels

            data = np.ascontiguousarray(data, np.int16)
            ch = channels(chan, n)
            self._check(self.lib.rawdtw_detect_raw_resident_begin(self._ctx, _opt(opt), n, _ptr(off), _ptr(data), _ptr(ch), _ptr(dst), _ptr(rm), cap))
            keep = (off, data, ch, dst, rm)
        det = ResidentDetection(self, n, keep)
        return det.end() if wait else det

    # -- seeding (ri_sketch + ri_idx_get, src/rmap.cpp:364-391) ---------------------
    def upload_seed_index(self, index):
        """The table of a seeding.SeedIndex into this context's device memory (replaces an earlier one)."""
        self._check(self.lib.rawdtw_seed_index_upload(self._ctx, index._h))

    def seed_hits(self, events, event_off, pinned: bool = True, hits_cap=None, kernel_ms: bool = False):
        """Every chunk k = events[event_off[k] .. event_off[k+1]) on the device: rawdtw_seed_begin, then _end.  Staging as
        detect_events keeps it.  hits_cap None: a first guess, and one more call with the exact total when it was too small.
        Returns (hit_off, hits as seeding.HIT_DTYPE), and the launches' device time in ms too when kernel_ms."""
        from .events import PinnedArray
        from .seeding import HIT_DTYPE

        ev = np.asarray(events, np.float32)
        off = np.ascontiguousarray(event_off, np.uint64)
        n = len(off) - 1
        cap = max(4 * len(ev), 1024) if hits_cap is None else int(hits_cap)
        while True:
            if pinned:
                st = getattr(self, "_seed_stage", None)
                if st is None or st["ev"].array.size < len(ev) or st["off"].array.size < n + 1 or st["hits"].array.size < cap:
                    st = self._seed_stage = {"ev": PinnedArray(len(ev), np.float32), "off": PinnedArray(n + 1, np.uint64),
                                             "hoff": PinnedArray(n + 1, np.uint64), "hits": PinnedArray(cap, HIT_DTYPE)}
                h_ev, h_off, hoff, hits = st["ev"].array, st["off"].array, st["hoff"].array, st["hits"].array
                h_ev[:len(ev)] = ev
                h_off[:n + 1] = off
            else:
                h_ev, h_off = np.ascontiguousarray(ev), off
                hoff, hits = np.zeros(n + 1, np.uint64), np.zeros(max(cap, 1), HIT_DTYPE)
            ms = C.c_float()
            self._check(self.lib.rawdtw_seed_begin(self._ctx, n, h_off.ctypes.data, h_ev.ctypes.data, hoff.ctypes.data,
                                                   hits.ctypes.data if cap else None, cap))
            st = self.lib.rawdtw_seed_end(self._ctx, C.byref(ms))
            if st == 4 and hits_cap is None:  # RAWDTW_ERR_RANGE: hit_off is filled
                cap = int(hoff[n])
                continue
            if st != 0:
                err = RawDTWError(st, self.lib.rawdtw_last_error(self._ctx).decode())
                err.hit_off = hoff[:n + 1].copy()
                raise err
            out = (hoff[:n + 1].copy(), hits[:int(hoff[n])].copy())
            return out + (float(ms.value),) if kernel_ms else out

    def reserve_events(self, n_floats: int):
        """rawdtw_events_reserve: the event arena grown to n_floats (contents kept)"""
        self._check(self.lib.rawdtw_events_reserve(self._ctx, int(n_floats)))

    def append_events(self, new_events, seg_src_off, seg_dst_off):
        """rawdtw_events_append, waited for: new_events[seg_src_off[s] .. seg_src_off[s+1]) to arena offset seg_dst_off[s]"""
        ev, src, dst = _f32(new_events), np.ascontiguousarray(seg_src_off, np.uint64), np.ascontiguousarray(seg_dst_off, np.uint32)
        self._check(self.lib.rawdtw_events_append(self._ctx, _ptr(ev), len(ev), len(dst), _ptr(src), _ptr(dst)))
        self.sync()

    def seed_resident(self, ev_start, ev_len, kernel_ms: bool = False):
        """Chunk k = the event arena's ev_len[k] events from ev_start[k] on, seeded where they are (rawdtw_seed_resident_begin, then
        _end): only the hit counts come home.  Returns a ResidentSeeding -- hit_off, kernel_ms, and fetch() for the hits themselves
        (rawdtw_seed_resident_fetch), which stay on the device until this context's next seeding."""
        start, ln = np.ascontiguousarray(ev_start, np.uint64), np.ascontiguousarray(ev_len, np.uint32)
        n = len(ln)
        if len(start) != n:
            raise ValueError("ev_start and ev_len differ in length")
        hoff = np.zeros(n + 1, np.uint64)
        ms = C.c_float()
        self._check(self.lib.rawdtw_seed_resident_begin(self._ctx, n, _ptr(start), _ptr(ln), _ptr(hoff)))
        self._check(self.lib.rawdtw_seed_resident_end(self._ctx, C.byref(ms)))
        return ResidentSeeding(self, hoff, float(ms.value))

    def seed_detected(self, detection, wait: bool = True):
        """The resident seeding of the chunks of `detection`, a ResidentDetection begun on this engine and not ended yet
        (detect_resident(..., wait=False)), enqueued straight behind it with no host step between: rawdtw_seed_detected_begin.
        Returns the ResidentSeeding (ended with rawdtw_seed_resident_end; RawDTWError status 4 when the detection declined), or with
        wait=False a DetectedSeeding to end() later.  The detection is ended by its own end(), before or after."""
        hoff = np.zeros(detection.n + 1, np.uint64)
        self._check(self.lib.rawdtw_seed_detected_begin(self._ctx, _ptr(hoff)))
        sd = DetectedSeeding(self, hoff)
        return sd.end() if wait else sd

    # -- batches ----------------------------------------------------------------
    def plan(self, jobs) -> Plan:
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        h = C.c_void_p()
        self._check(self.lib.rawdtw_plan_create(self._ctx, _ptr(jobs), len(jobs), C.byref(h)))
        return Plan(self, h, len(jobs))

    def score_batch(self, jobs, events) -> np.ndarray:
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        ev = _f32(events)
        out = np.empty(len(jobs), np.float32)
        self._check(self.lib.rawdtw_score_batch(self._ctx, _ptr(jobs), len(jobs), _ptr(ev), len(ev), _ptr(out)))
        return out

    def traceback_batch(self, jobs, events):
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        ev = _f32(events)
        caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
        off = np.zeros(len(jobs) + 1, np.uint64)
        np.cumsum(caps, out=off[1:])
        total = int(off[-1])
        cost = np.empty(len(jobs), np.float32)
        plen = np.zeros(len(jobs), np.uint32)
        pi = np.zeros(max(total, 1), np.uint32)
        pj = np.zeros(max(total, 1), np.uint32)
        pd = np.zeros(max(total, 1), np.float32)
        self._check(
            self.lib.rawdtw_traceback_batch(
                self._ctx, _ptr(jobs), len(jobs), _ptr(ev), len(ev), _ptr(cost), _ptr(off), _ptr(plen),
                _ptr(pi), _ptr(pj), _ptr(pd),
            )
        )
        res = []
        for k in range(len(jobs)):
            s, e = int(off[k]), int(off[k]) + int(plen[k])
            res.append(DtwResult(cost[k], pi[s:e].copy(), pj[s:e].copy(), pd[s:e].copy()))
        return res

    def traceback_arena_steps(self, jobs, path_off=None):
        """rawdtw_traceback_arena_steps: full-matrix tracebacks whose read_off index the event arena as it lies -- nothing is uploaded,
        nothing in the arena is written.  Returns (cost, path_off, path_len, step, distance): job k's path is the path_len[k] elements
        from path_off[k] on, one step byte (bit 0: i advanced, bit 1: j advanced) and one distance an element.  path_off: the caller's
        layout (n + m - 1 elements of room a job), default dense in job order."""
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
        if path_off is None:
            off = np.zeros(len(jobs) + 1, np.uint64)
            np.cumsum(caps, out=off[1:])
            total = int(off[-1])
        else:
            off = np.ascontiguousarray(path_off, np.uint64)
            if len(off) < len(jobs):
                raise ValueError("path_off is shorter than the job list")
            total = int((off[:len(jobs)] + caps).max()) if len(jobs) else 0
        cost = np.empty(len(jobs), np.float32)
        plen = np.zeros(len(jobs), np.uint32)
        step = np.zeros(max(total, 1), np.uint8)
        pd = np.zeros(max(total, 1), np.float32)
        self._check(self.lib.rawdtw_traceback_arena_steps(self._ctx, _ptr(jobs), len(jobs), _ptr(cost), _ptr(off), _ptr(plen), _ptr(step), _ptr(pd)))
        return cost, off, plen, step, pd

    def aln_text(self, step, distance, path_off, path_len, recs, cap=None, sizes_only=False):
        """rawdtw_aln_text_steps: the aln:s: text of paths given as steps and distances (include/rawdtw.h, "aln text"), made by the device's
        count, scan and write launches -> (text_off, text): job k's text is text[text_off[k]:text_off[k + 1]] (bytes).  cap: the text
        buffer's size (default: exactly what a first, sizes-only call reports); sizes_only: text is None."""
        a = _aln_args(step, distance, path_off, path_len, recs)
        return _aln_call(lambda toff, text, tcap, nb: self.lib.rawdtw_aln_text_steps(self._ctx, *[_ptr(x) for x in a], len(a[4]), toff, text, tcap, nb), len(a[4]), cap, sizes_only, self._check)

    def traceback_text(self, jobs, recs, events=None, cap=None, sizes_only=False):
        """rawdtw_traceback_batch_text (events None: rawdtw_traceback_arena_text, over the arena as it lies) -> (cost, path_len, text_off,
        text): full-matrix tracebacks whose paths stay on the device and come home as the aln:s: text.  cap: the text buffer's size
        (default aln_text_bound(jobs, recs)); sizes_only: text is None."""
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        recs = np.ascontiguousarray(recs, dtype=ALN_REC_DTYPE)
        if len(recs) != len(jobs):
            raise ValueError("one rec a job")
        ev = None if events is None else _f32(events)
        cost = np.empty(len(jobs), np.float32)
        plen = np.zeros(len(jobs), np.uint32)

        def call(toff, text, tcap, nb):
            if ev is None:
                return self.lib.rawdtw_traceback_arena_text(self._ctx, _ptr(jobs), len(jobs), _ptr(recs), _ptr(cost), _ptr(plen), toff, text, tcap, nb)
            return self.lib.rawdtw_traceback_batch_text(self._ctx, _ptr(jobs), len(jobs), _ptr(ev), len(ev), _ptr(recs), _ptr(cost), _ptr(plen), toff, text, tcap, nb)

        toff, text = _aln_call(call, len(jobs), aln_text_bound(jobs, recs) if cap is None else cap, sizes_only, self._check)
        return cost, plen, toff, text

    def aln_text_timing(self) -> dict:
        """device time of the text launches of the context's most recent aln_text / traceback_text call, and the bytes they made"""
        c, w, b = C.c_float(), C.c_float(), C.c_uint64()
        self._check(self.lib.rawdtw_aln_text_timing(self._ctx, C.byref(c), C.byref(w), C.byref(b)))
        return {"count_ms": c.value, "write_ms": w.value, "text_bytes": b.value}

    def events_fetch(self, starts, lens):
        """rawdtw_events_fetch: the arena's stretches [starts[q], starts[q] + lens[q]) as one array a segment, in order"""
        start, ln = np.ascontiguousarray(starts, np.uint32), np.ascontiguousarray(lens, np.uint32)
        if len(start) != len(ln):
            raise ValueError("starts and lens differ in length")
        off = np.zeros(len(ln) + 1, np.uint64)
        cap = int(ln.astype(np.uint64).sum())
        out = np.empty(max(cap, 1), np.float32)
        self._check(self.lib.rawdtw_events_fetch(self._ctx, len(ln), _ptr(start), _ptr(ln), _ptr(off), _ptr(out), cap))
        return [out[int(off[q]):int(off[q + 1])].copy() for q in range(len(ln))]

    # -- the reference's own function names (src/dtw.hpp:21,25,28) -----------------
    def DTW_global(self, a_values, b_values, exclude_last_element=False) -> np.float32:
        a, b = _f32(a_values), _f32(b_values)
        c = C.c_float()
        self._check(self.lib.rawdtw_dtw_global(self._ctx, _ptr(a), len(a), _ptr(b), len(b),
                                               int(exclude_last_element), C.byref(c)))
        return np.float32(c.value)

    def DTW_global_slantedbanded_antidiagonalwise(self, a_values, b_values, band_radius,
                                                  exclude_last_element=False) -> np.float32:
        a, b = _f32(a_values), _f32(b_values)
        c = C.c_float()
        self._check(self.lib.rawdtw_dtw_global_slantedbanded_antidiagonalwise(
            self._ctx, _ptr(a), len(a), _ptr(b), len(b), int(band_radius), int(exclude_last_element), C.byref(c)))
        return np.float32(c.value)

    def DTW_global_tb(self, a_values, b_values, exclude_last_element=False) -> DtwResult:
        a, b = _f32(a_values), _f32(b_values)
        cap = len(a) + len(b) - 1
        pi = np.zeros(max(cap, 1), np.uint32)
        pj = np.zeros(max(cap, 1), np.uint32)
        pd = np.zeros(max(cap, 1), np.float32)
        c = C.c_float()
        ln = C.c_uint32()
        self._check(self.lib.rawdtw_dtw_global_tb(self._ctx, _ptr(a), len(a), _ptr(b), len(b),
                                                  int(exclude_last_element), C.byref(c), C.byref(ln),
                                                  _ptr(pi), _ptr(pj), _ptr(pd)))
        k = ln.value
        return DtwResult(np.float32(c.value), pi[:k].copy(), pj[:k].copy(), pd[:k].copy())

    def DTW_semiglobal(self, a_values, b_values, exclude_last_element=False) -> DtwResult:
        """DTW_semiglobal (src/dtw.cpp:526-550): a end to end against the best-matching substring of b.  The cost (the flag is ignored, as
        its namesake ignores it); no path: i, j and difference are empty."""
        a, b = _f32(a_values), _f32(b_values)
        c = C.c_float()
        self._check(self.lib.rawdtw_dtw_semiglobal(self._ctx, _ptr(a), len(a), _ptr(b), len(b), int(exclude_last_element), C.byref(c)))
        return DtwResult(np.float32(c.value), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32))

    def DTW_semiglobal_tb(self, a_values, b_values, exclude_last_element=False) -> DtwResult:
        """DTW_semiglobal_tb (src/dtw.cpp:669-753): the cost and the path from (0, j0) to (n - 1, end_j)"""
        a, b = _f32(a_values), _f32(b_values)
        cap = len(a) + len(b) - 1
        pi = np.zeros(max(cap, 1), np.uint32)
        pj = np.zeros(max(cap, 1), np.uint32)
        pd = np.zeros(max(cap, 1), np.float32)
        c = C.c_float()
        ln = C.c_uint32()
        self._check(self.lib.rawdtw_dtw_semiglobal_tb(self._ctx, _ptr(a), len(a), _ptr(b), len(b), int(exclude_last_element), C.byref(c),
                                                      C.byref(ln), _ptr(pi), _ptr(pj), _ptr(pd)))
        k = ln.value
        return DtwResult(np.float32(c.value), pi[:k].copy(), pj[:k].copy(), pd[:k].copy())

    def semiglobal_batch(self, jobs, events=None):
        """rawdtw_semiglobal_batch -> (cost, end_j), one of each a job (band_radius must be -1).  events None: the jobs' read_off index
        the context's event arena as it lies; else the arena is replaced by `events` first."""
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        ev = None if events is None else _f32(events)
        cost = np.empty(len(jobs), np.float32)
        end_j = np.zeros(len(jobs), np.uint32)
        self._check(self.lib.rawdtw_semiglobal_batch(self._ctx, _ptr(jobs), len(jobs), None if ev is None else _ptr(ev),
                                                     0 if ev is None else len(ev), _ptr(cost), _ptr(end_j)))
        return cost, end_j

    def semiglobal_traceback(self, jobs, events=None):
        """rawdtw_semiglobal_traceback_steps -> (cost, j0, path_off, path_len, step, distance): job k's path is the path_len[k] elements
        from path_off[k] on, start first -- element 0 is (0, j0[k]) with step byte 0, then one byte an element (bit 0: i advanced,
        bit 1: j advanced) -- and one distance an element.  `expand_steps` turns a path into (i, j).  events: as semiglobal_batch."""
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        ev = None if events is None else _f32(events)
        caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
        off = np.zeros(len(jobs) + 1, np.uint64)
        np.cumsum(caps, out=off[1:])
        total = int(off[-1])
        cost = np.empty(len(jobs), np.float32)
        j0 = np.zeros(len(jobs), np.uint32)
        plen = np.zeros(len(jobs), np.uint32)
        step = np.zeros(max(total, 1), np.uint8)
        pd = np.zeros(max(total, 1), np.float32)
        self._check(self.lib.rawdtw_semiglobal_traceback_steps(self._ctx, _ptr(jobs), len(jobs), None if ev is None else _ptr(ev),
                                                               0 if ev is None else len(ev), _ptr(cost), _ptr(j0), _ptr(off), _ptr(plen),
                                                               _ptr(step), _ptr(pd)))
        return cost, j0, off, plen, step, pd

    def semiglobal_timing(self) -> dict:
        """device time of the context's most recent semiglobal call: its fill kernels, its walk and finish kernels (0 without paths)"""
        f, w, d, e = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.rawdtw_semiglobal_timing(self._ctx, C.byref(f), C.byref(w), C.byref(d), C.byref(e)))
        return {"fill_ms": f.value, "walk_ms": w.value, "direction_bytes": d.value, "path_elements": e.value}

    def semiglobal_span(self, jobs, events=None):
        """rawdtw_semiglobal_span_batch -> (cost, j0, end_j), one of each a job: cost and end_j as semiglobal_batch, j0 the column in which
        DTW_semiglobal_tb's path starts (semiglobal_traceback's j0), from one pass without a direction matrix.  events: as semiglobal_batch."""
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        ev = None if events is None else _f32(events)
        cost = np.empty(len(jobs), np.float32)
        j0 = np.zeros(len(jobs), np.uint32)
        end_j = np.zeros(len(jobs), np.uint32)
        self._check(self.lib.rawdtw_semiglobal_span_batch(self._ctx, _ptr(jobs), len(jobs), None if ev is None else _ptr(ev),
                                                          0 if ev is None else len(ev), _ptr(cost), _ptr(j0), _ptr(end_j)))
        return cost, j0, end_j

    def DTW_semiglobal_span(self, a_values, b_values, exclude_last_element=False):
        """rawdtw_dtw_semiglobal_span -> (cost, j0, end_j): DTW_semiglobal_tb's cost and the columns of its path's first and last element"""
        a, b = _f32(a_values), _f32(b_values)
        c, j0, ej = C.c_float(), C.c_uint32(), C.c_uint32()
        self._check(self.lib.rawdtw_dtw_semiglobal_span(self._ctx, _ptr(a), len(a), _ptr(b), len(b), int(exclude_last_element), C.byref(c),
                                                        C.byref(j0), C.byref(ej)))
        return np.float32(c.value), j0.value, ej.value

    def semiglobal_place(self, reads, targets, exclude_last=False, paths=False) -> dict:
        """Seed-free placement: every read window (read_off, n) of the event arena against every target window (ref_off, m) of the
        reference arena (both strands of every sequence, say) in one semiglobal_span call of len(reads) x len(targets) jobs, read-major;
        then, on the host, `semiglobal_place_reduce` over each read's row -> {target, cost, j0, end_j, second}, one of each a read.
        paths: the winners, one job a read (a read without a winner: its target 0), go through semiglobal_traceback -- in windows where
        set_semiglobal_window is on -- and the dict gains path_off, path_len, step and distance, and the traceback's own cost and j0 as
        tb_cost and tb_j0; nothing is compared here."""
        reads = np.asarray(reads, np.int64).reshape(-1, 2)
        targets = np.asarray(targets, np.int64).reshape(-1, 2)
        jobs = np.zeros(len(reads) * len(targets), JOB_DTYPE)
        jobs["read_off"] = np.repeat(reads[:, 0], len(targets))
        jobs["n"] = np.repeat(reads[:, 1], len(targets))
        jobs["ref_off"] = np.tile(targets[:, 0], len(reads))
        jobs["m"] = np.tile(targets[:, 1], len(reads))
        jobs["band_radius"], jobs["exclude_last"] = RAWDTW_FULL, int(bool(exclude_last))
        shape = (len(reads), len(targets))
        cost, j0, end_j = self.semiglobal_span(jobs)
        placed = semiglobal_place_reduce(cost.reshape(shape), j0.reshape(shape), end_j.reshape(shape))
        if not paths:
            return placed
        winners = jobs[np.arange(len(reads)) * len(targets) + np.maximum(placed["target"], 0)] if len(targets) else jobs[:0]
        tb_cost, tb_j0, off, plen, step, pd = self.semiglobal_traceback(winners)
        placed.update(path_off=off, path_len=plen, step=step, distance=pd, tb_cost=tb_cost, tb_j0=tb_j0)
        return placed

    def DTW_global_banded_tb(self, a_values, b_values, band_radius, exclude_last=False) -> DtwResult:
        """The banded cost of DTW_global_slantedbanded_antidiagonalwise and the path DTW_global_tb's walk takes through the band's cells
        (include/rawdtw.h, "banded traceback"); a job without a path has empty i, j and difference"""
        a, b = _f32(a_values), _f32(b_values)
        cap = len(a) + len(b) - 1
        pi = np.zeros(max(cap, 1), np.uint32)
        pj = np.zeros(max(cap, 1), np.uint32)
        pd = np.zeros(max(cap, 1), np.float32)
        c = C.c_float()
        ln = C.c_uint32()
        self._check(self.lib.rawdtw_dtw_global_banded_tb(self._ctx, _ptr(a), len(a), _ptr(b), len(b), int(band_radius), int(exclude_last),
                                                         C.byref(c), C.byref(ln), _ptr(pi), _ptr(pj), _ptr(pd)))
        k = ln.value
        return DtwResult(np.float32(c.value), pi[:k].copy(), pj[:k].copy(), pd[:k].copy())

    def banded_traceback(self, jobs, events=None, path_off=None, out=None):
        """rawdtw_banded_traceback_steps -> (cost, path_off, path_len, step, distance): job k's path is the path_len[k] elements from
        path_off[k] on, start first at (0, 0), one step byte (bit 0: i advanced, bit 1: j advanced) and one distance an element;
        path_len 0: the job has no path.  events None: the jobs' read_off index the event arena as it lies.  path_off: the caller's
        layout (n + m - 1 elements of room a job), default dense in job order.  out: (cost, path_len, step, distance) to write into."""
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        ev = None if events is None else _f32(events)
        caps = jobs["n"].astype(np.uint64) + jobs["m"].astype(np.uint64) - 1
        if path_off is None:
            off = np.zeros(len(jobs) + 1, np.uint64)
            np.cumsum(caps, out=off[1:])
            total = int(off[-1])
        else:
            off = np.ascontiguousarray(path_off, np.uint64)
            if len(off) < len(jobs):
                raise ValueError("path_off is shorter than the job list")
            total = int((off[:len(jobs)] + caps).max()) if len(jobs) else 0
        if out is None:
            cost, plen = np.empty(len(jobs), np.float32), np.zeros(len(jobs), np.uint32)
            step, pd = np.zeros(max(total, 1), np.uint8), np.zeros(max(total, 1), np.float32)
        else:
            cost, plen, step, pd = out
        self._check(self.lib.rawdtw_banded_traceback_steps(self._ctx, _ptr(jobs), len(jobs), None if ev is None else _ptr(ev),
                                                           0 if ev is None else len(ev), _ptr(cost), _ptr(off), _ptr(plen), _ptr(step),
                                                           _ptr(pd)))
        return cost, off, plen, step, pd

    def banded_traceback_timing(self) -> dict:
        """device time of the context's most recent banded traceback call: its fill kernel, its walk and finish kernels"""
        f, w, d, e = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.rawdtw_banded_traceback_timing(self._ctx, C.byref(f), C.byref(w), C.byref(d), C.byref(e)))
        return {"fill_ms": f.value, "walk_ms": w.value, "direction_bytes": d.value, "path_elements": e.value}


# rawdtw_aln_rec_t (include/rawdtw.h, "aln text")
ALN_REC_DTYPE = np.dtype([("off_i", np.uint64), ("off_j", np.uint64), ("j0", np.uint32), ("mode", np.uint32), ("pad", np.uint64)])
assert ALN_REC_DTYPE.itemsize == 32


def _aln_args(step, distance, path_off, path_len, recs):
    step = np.ascontiguousarray(step, np.uint8)
    pd = np.ascontiguousarray(distance, np.float32)
    off = np.ascontiguousarray(path_off, np.uint64)
    plen = np.ascontiguousarray(path_len, np.uint32)
    recs = np.ascontiguousarray(recs, dtype=ALN_REC_DTYPE)
    if len(off) < len(plen) or len(recs) != len(plen) or len(step) != len(pd):
        raise ValueError("one offset, one length and one rec a job; one step byte a distance")
    if len(plen) and int((off[:len(plen)] + plen)[plen > 0].max(initial=0)) > len(step):
        raise ValueError("a path lies beyond the step array")
    return step, pd, off, plen, recs


def _aln_call(call, n_jobs, cap, sizes_only, check):
    """(text_off, text) of one of the aln text entry points: `call(text_off, text, text_cap, text_bytes)`.  cap None: sized by a first,
    sizes-only call.  The text buffer is exactly cap bytes."""
    toff = np.zeros(n_jobs + 1, np.uint64)
    nb = C.c_uint64(0)
    if cap is None or sizes_only:
        check(call(_ptr(toff), None, 0, C.byref(nb)))
        if sizes_only:
            return toff, None
        cap = nb.value
    text = np.zeros(max(int(cap), 1), np.uint8)
    check(call(_ptr(toff), _ptr(text), int(cap), C.byref(nb)))
    return toff, text[:nb.value]


def aln_text_host(step, distance, path_off, path_len, recs, threads: int = 0, cap=None, sizes_only=False):
    """rawdtw_aln_text_host: the aln text's definition (include/rawdtw.h) restated on host threads, no device -> (text_off, text) as
    Engine.aln_text"""
    from ._lib import load_library

    lib = load_library()
    a = _aln_args(step, distance, path_off, path_len, recs)

    def check(st):
        if st != 0:
            raise RawDTWError(st, "rawdtw_aln_text_host")

    return _aln_call(lambda toff, text, tcap, nb: lib.rawdtw_aln_text_host(*[_ptr(x) for x in a], len(a[4]), threads, toff, text, tcap, nb),
                     len(a[4]), cap, sizes_only, check)


def aln_text_bound(jobs, recs) -> int:
    """rawdtw_aln_text_bound: an upper bound on the text of these jobs' paths, whatever the paths are"""
    from ._lib import load_library

    jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
    recs = np.ascontiguousarray(recs, dtype=ALN_REC_DTYPE)
    if len(recs) != len(jobs):
        raise ValueError("one rec a job")
    return int(load_library().rawdtw_aln_text_bound(_ptr(jobs), _ptr(recs), len(jobs)))


def expand_steps(step, j0: int = 0):
    """a path's step bytes (bit 0: i advanced, bit 1: j advanced; element 0's byte is 0) -> (i, j), starting at (0, j0)"""
    s = np.asarray(step, np.uint8)
    i = np.cumsum(s & 1, dtype=np.uint64).astype(np.uint32)
    j = (np.cumsum(s >> 1, dtype=np.uint64) + np.uint64(j0)).astype(np.uint32)
    return i, j


def semiglobal_host(a_values, b_values, exclude_last_element=False, traceback=False):
    """rawdtw_semiglobal_host / rawdtw_semiglobal_tb_host: the recurrence restated on the host, no device.  -> (cost, end_j), with
    traceback (DtwResult, end_j)."""
    lib = load_library()
    a, b = _f32(a_values), _f32(b_values)
    c, ej = C.c_float(), C.c_uint32()
    if not traceback:
        st = lib.rawdtw_semiglobal_host(_ptr(a), len(a), _ptr(b), len(b), int(exclude_last_element), C.byref(c), C.byref(ej))
        if st != 0:
            raise RawDTWError(st, "rawdtw_semiglobal_host refused its arguments")
        return np.float32(c.value), ej.value
    cap = max(len(a) + len(b) - 1, 1)
    pi, pj, pd = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.float32)
    ln = C.c_uint32()
    st = lib.rawdtw_semiglobal_tb_host(_ptr(a), len(a), _ptr(b), len(b), int(exclude_last_element), C.byref(c), C.byref(ej), C.byref(ln),
                                       _ptr(pi), _ptr(pj), _ptr(pd))
    if st != 0:
        raise RawDTWError(st, "rawdtw_semiglobal_tb_host refused its arguments")
    k = ln.value
    return DtwResult(np.float32(c.value), pi[:k].copy(), pj[:k].copy(), pd[:k].copy()), ej.value


def semiglobal_tb_window_host(a_values, b_values, columns, exclude_last_element=False):
    """rawdtw_semiglobal_tb_window_host: the traceback in windows (include/rawdtw.h, "semiglobal, in windows") restated on the host in
    O(n m / C + n C) memory, no device -> (DtwResult, end_j, windows entered)"""
    lib = load_library()
    a, b = _f32(a_values), _f32(b_values)
    c, ej, ln, wn = C.c_float(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    cap = max(len(a) + len(b) - 1, 1)
    pi, pj, pd = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.float32)
    if not 0 <= int(columns) < 1 << 32:
        raise RawDTWError(1, "rawdtw_semiglobal_tb_window_host refused its arguments")
    st = lib.rawdtw_semiglobal_tb_window_host(_ptr(a), len(a), _ptr(b), len(b), int(exclude_last_element), int(columns), C.byref(c), C.byref(ej),
                                              C.byref(ln), _ptr(pi), _ptr(pj), _ptr(pd), C.byref(wn))
    if st != 0:
        raise RawDTWError(st, "rawdtw_semiglobal_tb_window_host refused its arguments")
    k = ln.value
    return DtwResult(np.float32(c.value), pi[:k].copy(), pj[:k].copy(), pd[:k].copy()), ej.value, wn.value


def semiglobal_span_host(a_values, b_values, exclude_last_element=False):
    """rawdtw_semiglobal_span_host: the span's definition (include/rawdtw.h) restated on the host in O(m) memory, no device
    -> (cost, j0, end_j)"""
    lib = load_library()
    a, b = _f32(a_values), _f32(b_values)
    c, j0, ej = C.c_float(), C.c_uint32(), C.c_uint32()
    st = lib.rawdtw_semiglobal_span_host(_ptr(a), len(a), _ptr(b), len(b), int(exclude_last_element), C.byref(c), C.byref(j0), C.byref(ej))
    if st != 0:
        raise RawDTWError(st, "rawdtw_semiglobal_span_host refused its arguments")
    return np.float32(c.value), j0.value, ej.value


def semiglobal_place_reduce(cost, j0, end_j) -> dict:
    """The reduction of Engine.semiglobal_place over tables [read, target]: per read the target of the lowest cost -- compared with <,
    so the lowest target index wins a tie; a NaN cost never wins, a read whose costs are all NaN gets target -1 (cost NaN, j0 and
    end_j 0) -- that target's cost, j0 and end_j, and `second`, the smallest non-NaN cost among the other targets (+inf without one)."""
    cost = np.asarray(cost, np.float32)
    j0, end_j = np.asarray(j0, np.uint32), np.asarray(end_j, np.uint32)
    n_reads, n_targets = cost.shape
    target = np.full(n_reads, -1, np.int32)
    best = np.full(n_reads, np.nan, np.float32)
    for t in range(n_targets):
        c = cost[:, t]
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(c) & ((target < 0) | (c < best))
        target[take], best[take] = t, c[take]
    rows, col = np.arange(n_reads), np.maximum(target, 0)
    found = target >= 0
    others = np.where(np.isnan(cost), np.float32(np.inf), cost)
    others[rows[found], col[found]] = np.inf
    second = others.min(axis=1) if n_targets else np.full(n_reads, np.inf, np.float32)
    pick = lambda table: np.where(found, table[rows, col], 0).astype(np.uint32) if n_targets else np.zeros(n_reads, np.uint32)  # noqa: E731
    return {"target": target, "cost": best, "j0": pick(j0), "end_j": pick(end_j), "second": second.astype(np.float32)}


def banded_tb_host(a_values, b_values, band_radius, exclude_last=False) -> DtwResult:
    """rawdtw_banded_tb_host: the banded traceback's definition (include/rawdtw.h) restated on the host, no device.  A job without a
    path has empty i, j and difference; its cost is still the banded cost."""
    lib = load_library()
    a, b = _f32(a_values), _f32(b_values)
    cap = max(len(a) + len(b) - 1, 1)
    pi, pj, pd = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.float32)
    c, ln = C.c_float(), C.c_uint32()
    st = lib.rawdtw_banded_tb_host(_ptr(a), len(a), _ptr(b), len(b), int(band_radius), int(exclude_last), C.byref(c), C.byref(ln),
                                   _ptr(pi), _ptr(pj), _ptr(pd))
    if st != 0:
        raise RawDTWError(st, "rawdtw_banded_tb_host refused its arguments")
    k = ln.value
    return DtwResult(np.float32(c.value), pi[:k].copy(), pj[:k].copy(), pd[:k].copy())
