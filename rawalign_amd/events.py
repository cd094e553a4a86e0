"""Event detection: detect_events (src/revent.c:190-210) through the C ABI (include/rawdtw.h, rawdtw_detect_*).

detect_events and detect_events_host run the library's host restatement; Engine.detect_events runs the device path
(rawdtw_events.hip).  Both are bit for bit the reference's, in the plain form (contracted=False: the source's one rounding per
operation) or the contracted one (contracted=True: as the reference's Makefile builds revent.c on an FMA host)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import EventOpt, RawDTWError, load_library


@dataclass
class EventOptions:
    """rawdtw_event_opt_t; defaults of src/roptions.c:37-41"""
    window_length1: int = 3
    window_length2: int = 6
    threshold1: float = 4.30265
    threshold2: float = 2.57058
    peak_height: float = 1.0
    contracted: bool = False

    def c(self) -> EventOpt:
        return EventOpt(self.window_length1, self.window_length2, self.threshold1, self.threshold2, self.peak_height,
                        int(self.contracted))


def _opt(opt):
    return None if opt is None else C.byref(opt.c() if isinstance(opt, EventOptions) else opt)


def _check(st: int):
    if st != 0:
        raise RawDTWError(st, load_library().rawdtw_status_string(st).decode())


def detect_events(sig, opt=None) -> np.ndarray:
    """One chunk on the host (the reference's name): the chunk's events, empty when no boundary is found."""
    lib = load_library()
    sig = np.ascontiguousarray(sig, np.float32)
    out = np.empty(max(len(sig), 1), np.float32)
    n = C.c_uint32()
    _check(lib.rawdtw_detect_events(_opt(opt), len(sig), sig.ctypes.data, out.ctypes.data, C.byref(n)))
    return out[:n.value].copy()


def detect_events_host(sig, sig_off, opt=None, threads: int = 0, events_cap=None):
    """Many chunks on the host (chunk k = sig[sig_off[k] .. sig_off[k+1])) on `threads` threads.  Returns (event_off, events)."""
    lib = load_library()
    sig = np.ascontiguousarray(sig, np.float32)
    off = np.ascontiguousarray(sig_off, np.uint64)
    cap = int(off[-1]) if events_cap is None else int(events_cap)
    eoff = np.zeros(len(off), np.uint64)
    ev = np.empty(max(cap, 1), np.float32)
    _check(lib.rawdtw_detect_events_host(_opt(opt), len(off) - 1, off.ctypes.data, sig.ctypes.data, eoff.ctypes.data,
                                         ev.ctypes.data, cap, int(threads)))
    return eoff, ev[:int(eoff[-1])].copy()


class PinnedArray:
    """A numpy view of page-locked host memory (rawdtw_host_alloc), freed with the object."""

    def __init__(self, n: int, dtype):
        self.lib = load_library()
        self.dtype = np.dtype(dtype)
        self.nbytes = max(int(n), 1) * self.dtype.itemsize
        p = C.c_void_p()
        _check(self.lib.rawdtw_host_alloc(self.nbytes, C.byref(p)))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr)).view(self.dtype)

    def __del__(self):
        if getattr(self, "ptr", None):
            self.lib.rawdtw_host_free(C.c_void_p(self.ptr))
            self.ptr = None


def chunks_of(sig, chunk_size: int = 4000, max_num_chunk: int = 30) -> np.ndarray:
    """The chunk offsets map_worker_for cuts a read into (src/rmap.cpp:685-690): chunk_size samples each, the last one shorter,
    at most max_num_chunk of them (roptions.c:11, 24).  Returns sig_off (uint64, n_chunks + 1 entries)."""
    qlen = len(sig)
    starts = list(range(0, qlen, chunk_size))[:max_num_chunk]
    return np.array(starts + [min(starts[-1] + chunk_size, qlen)] if starts else [0], np.uint64)
