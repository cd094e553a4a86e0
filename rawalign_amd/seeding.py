"""Seeding: a chunk's events to seed hits -- ri_sketch (src/rsketch.c) followed by ri_idx_get (src/rawindex.cpp:256-273) as
gen_chains calls them (src/rmap.cpp:364-391) -- through the C ABI (include/rawdtw.h, rawdtw_seed_*).

SeedIndex, sketch and seed_hits_host run the library's host code; Engine.upload_seed_index / Engine.seed_hits run the device
path (rawdtw_seed.hip).  Both give the reference's hits, value for value and in its order."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import RawDTWError, SeedPars, load_library

HIT_DTYPE = np.dtype([("ref_seq", "<u4"), ("strand", "<i4"), ("target_position", "<u4"), ("query_position", "<u4")])  # rawdtw_seed_hit_t
assert HIT_DTYPE.itemsize == 16


@dataclass
class SeedParams:
    """rawdtw_seed_pars_t; defaults of ri_idxopt_init (src/rawindex.cpp:465-472)"""
    w: int = 0
    e: int = 6
    n: int = 0
    q: int = 9
    lq: int = 3
    k: int = 6

    def c(self) -> SeedPars:
        return SeedPars(self.w, self.e, self.n, self.q, self.lq, self.k)


def _pars(p):
    return p.c() if isinstance(p, SeedParams) else p if isinstance(p, SeedPars) else SeedParams(**(p or {})).c()


def _check(st: int):
    if st != 0:
        raise RawDTWError(st, load_library().rawdtw_status_string(st).decode())


class SeedIndex:
    """rawdtw_seed_index: what ri_idx_get answers from, built from signal arrays or read from a .ind file's buckets."""

    def __init__(self, handle):
        self.lib = load_library()
        self._h = handle
        n_seq, keys, npos, nbytes, p = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64(), SeedPars()
        _check(self.lib.rawdtw_seed_index_info(handle, C.byref(n_seq), C.byref(keys), C.byref(npos), C.byref(nbytes), C.byref(p)))
        self.n_seq, self.n_keys, self.n_positions, self.table_bytes = n_seq.value, keys.value, npos.value, nbytes.value
        self.pars = SeedParams(p.w, p.e, p.n, p.q, p.lq, p.k)

    @classmethod
    def from_signals(cls, forward, reverse, pars=None, threads: int = 1) -> "SeedIndex":
        lib = load_library()
        fwd = [np.ascontiguousarray(x, np.float32) for x in forward]
        rev = [np.ascontiguousarray(x, np.float32) for x in reverse]
        assert len(fwd) == len(rev) and all(len(a) == len(b) for a, b in zip(fwd, rev))
        pf = (C.c_void_p * max(len(fwd), 1))(*[x.ctypes.data for x in fwd])
        pr = (C.c_void_p * max(len(rev), 1))(*[x.ctypes.data for x in rev])
        lens = np.array([len(x) for x in fwd] or [0], np.uint32)
        h = C.c_void_p()
        _check(lib.rawdtw_seed_index_build(len(fwd), pf, pr, lens.ctypes.data, C.byref(_pars(pars)), int(threads), C.byref(h)))
        return cls(h)

    @classmethod
    def from_index(cls, index) -> "SeedIndex":
        """the buckets of an opened .ind file (rawalign_amd.index.Index)"""
        h = C.c_void_p()
        _check(load_library().rawdtw_seed_index_load(index._h, C.byref(h)))
        return cls(h)

    @classmethod
    def from_device(cls, engine, pars=None, minimizer: bool = False, resident: bool = False) -> "SeedIndex":
        """rawdtw_seed_index_build_device: from_signals of the arrays the engine's reference holds, built on the device (w = 0 only).
        `minimizer`: rawdtw_seed_index_build_device_min, which takes w > 0 too (ri_sketch_min's windows over whole strands).
        `resident`: rawdtw_seed_index_build_resident (any w): the table is built and kept on the device as the engine's seed table;
        the index has no host copy until fetch()."""
        h = C.c_void_p()
        lib = engine.lib
        build = lib.rawdtw_seed_index_build_resident if resident else lib.rawdtw_seed_index_build_device_min if minimizer else lib.rawdtw_seed_index_build_device
        engine._check(build(engine._ctx, C.byref(_pars(pars)), C.byref(h)))
        return cls(h)

    @classmethod
    def from_entries(cls, pars, n_seq: int, hashes, ys, engine=None) -> "SeedIndex":
        """The table of entries (hash, y) sorted by (hash, y): rawdtw_seed_index_from_entries on the host, or with an engine
        rawdtw_seed_table_from_entries -- the device's table launches alone, a resident index on that engine."""
        hs, y = np.ascontiguousarray(hashes, np.uint32), np.ascontiguousarray(ys, np.uint64)
        assert hs.ndim == y.ndim == 1 and len(hs) == len(y)
        h = C.c_void_p()
        if engine is None:
            _check(load_library().rawdtw_seed_index_from_entries(C.byref(_pars(pars)), int(n_seq), len(hs), hs.ctypes.data, y.ctypes.data, C.byref(h)))
        else:
            engine._check(engine.lib.rawdtw_seed_table_from_entries(engine._ctx, C.byref(_pars(pars)), int(n_seq), len(hs), hs.ctypes.data, y.ctypes.data, C.byref(h)))
        return cls(h)

    @property
    def resident(self) -> bool:
        """the index has no host copy: its table is the seed table of the engine that built it"""
        return bool(self.lib.rawdtw_seed_index_is_resident(self._h))

    def fetch(self, engine) -> "SeedIndex":
        """rawdtw_seed_index_fetch: a resident index's slots and lists come home; from then on an ordinary index"""
        engine._check(self.lib.rawdtw_seed_index_fetch(engine._ctx, self._h))
        return self

    def get(self, hash_value: int) -> np.ndarray:
        """ri_idx_get: the packed positions id << 32 | pos << 1 | strand of a hash, in the index's order (empty: not there)"""
        p, n = C.c_void_p(), C.c_uint32()
        _check(self.lib.rawdtw_seed_index_get(self._h, int(hash_value), C.byref(p), C.byref(n)))
        if not n.value:
            return np.zeros(0, np.uint64)
        return np.ctypeslib.as_array((C.c_uint64 * n.value).from_address(p.value)).copy()

    def keys(self) -> np.ndarray:
        out = np.zeros(max(self.n_keys, 1), np.uint32)
        _check(self.lib.rawdtw_seed_index_keys(self._h, out.ctypes.data))
        return out[:self.n_keys]

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.lib.rawdtw_seed_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sketch(events, pars=None):
    """ri_sketch for one chunk: (hash, pos) of its sketch elements in emission order"""
    lib = load_library()
    ev = np.ascontiguousarray(events, np.float32)
    h, p, n = np.zeros(max(len(ev), 1), np.uint32), np.zeros(max(len(ev), 1), np.uint32), C.c_uint32()
    _check(lib.rawdtw_seed_sketch(C.byref(_pars(pars)), ev.ctypes.data, len(ev), h.ctypes.data, p.ctypes.data, C.byref(n)))
    return h[:n.value].copy(), p[:n.value].copy()


def sketch_windowed(events, pars=None, cap=None):
    """rawdtw_seed_sketch_windowed: the sketch of one strand or chunk in the form the device build of a minimizer table runs -- every
    e-mer's step on its own.  Equal to sketch().  With `cap` too small the RawDTWError carries the true count as .n."""
    lib = load_library()
    ev = np.ascontiguousarray(events, np.float32)
    n = C.c_uint32()
    if cap is None:  # count first: the minimizer sketch may emit more elements than events
        st = lib.rawdtw_seed_sketch_windowed(C.byref(_pars(pars)), ev.ctypes.data, len(ev), None, None, 0, C.byref(n))
        if st not in (0, 4):
            _check(st)
        cap = n.value
    h, p = np.zeros(max(int(cap), 1), np.uint32), np.zeros(max(int(cap), 1), np.uint32)
    st = lib.rawdtw_seed_sketch_windowed(C.byref(_pars(pars)), ev.ctypes.data, len(ev), h.ctypes.data, p.ctypes.data, int(cap), C.byref(n))
    if st != 0:
        err = RawDTWError(st, lib.rawdtw_status_string(st).decode())
        err.n = n.value
        raise err
    return h[:n.value].copy(), p[:n.value].copy()


def seed_hits_host(index: SeedIndex, events, event_off, threads: int = 1, hits_cap=None):
    """Many chunks on the host (chunk k = events[event_off[k] .. event_off[k+1])).  Returns (hit_off, hits as HIT_DTYPE).  With
    hits_cap too small the RawDTWError carries hit_off."""
    lib = load_library()
    ev = np.ascontiguousarray(events, np.float32)
    off = np.ascontiguousarray(event_off, np.uint64)
    n = len(off) - 1
    hoff = np.zeros(n + 1, np.uint64)
    cap = hits_cap
    if cap is None:  # count first
        st = lib.rawdtw_seed_hits_host(index._h, n, off.ctypes.data, ev.ctypes.data, hoff.ctypes.data, None, 0, int(threads))
        if st not in (0, 4):
            _check(st)
        cap = int(hoff[n])
    hits = np.zeros(max(int(cap), 1), HIT_DTYPE)
    st = lib.rawdtw_seed_hits_host(index._h, n, off.ctypes.data, ev.ctypes.data, hoff.ctypes.data, hits.ctypes.data, int(cap), int(threads))
    if st != 0:
        err = RawDTWError(st, lib.rawdtw_status_string(st).decode())
        err.hit_off = hoff
        raise err
    return hoff, hits[:int(hoff[n])]
