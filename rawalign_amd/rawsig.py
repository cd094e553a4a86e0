"""Raw signal in: the int16 DAC samples of a signal file to pA and the outlier filter of ri_read_sig (src/rsig.cpp:216-224)
through the C ABI (include/rawdtw.h, rawdtw_signal_* and rawdtw_detect_raw_*).

to_pa, chunk_table and detect_events_raw_host run the library's host restatement; Engine.detect_events_raw runs the device path
(k_raw_count / k_raw_compact in rawdtw_events.hip, then the detection launches).  A channel is (digitisation, range, offset) as
float32: a Channel, a 3-tuple, or a row of a CHANNEL_DTYPE array."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import load_library
from .events import _check, _opt

CHANNEL_DTYPE = np.dtype([("digitisation", np.float32), ("range", np.float32), ("offset", np.float32)])  # rawdtw_channel_t


@dataclass
class Channel:
    """rawdtw_channel_t: ri_sig_t's dig, ran, offset (src/rsig.h:16)"""
    digitisation: float = 8192.0
    range: float = 1450.0
    offset: float = 0.0


def channels(chan, n: int = 1) -> np.ndarray:
    """n channel records as a contiguous CHANNEL_DTYPE array: one channel for all, or one a window."""
    if isinstance(chan, Channel):
        chan = (chan.digitisation, chan.range, chan.offset)
    if isinstance(chan, np.void):  # a row of a CHANNEL_DTYPE array
        chan = tuple(chan)
    if isinstance(chan, np.ndarray) and chan.dtype == CHANNEL_DTYPE:
        out = np.ascontiguousarray(chan).reshape(-1)
    elif isinstance(chan, tuple):
        out = np.zeros(1, CHANNEL_DTYPE)
        out[0] = chan
    else:
        out = np.zeros(len(chan), CHANNEL_DTYPE)
        for k, c in enumerate(chan):
            out[k] = (c.digitisation, c.range, c.offset) if isinstance(c, Channel) else tuple(c)
    if len(out) == 1 and n != 1:
        out = np.repeat(out, n)
    assert len(out) == n, (len(out), n)
    return out


def to_pa(raw, chan) -> np.ndarray:
    """One read on the host: the kept pA samples, in order (float32)."""
    lib = load_library()
    raw = np.ascontiguousarray(raw, np.int16)
    ch = channels(chan)
    pa = np.empty(max(len(raw), 1), np.float32)
    l_sig = C.c_uint64()
    _check(lib.rawdtw_signal_to_pa(ch.ctypes.data, len(raw), raw.ctypes.data, pa.ctypes.data, C.byref(l_sig)))
    return pa[:l_sig.value].copy()


def count_kept(raw, chan) -> int:
    """l_sig alone (rawdtw_signal_to_pa with pa == NULL)."""
    lib = load_library()
    raw = np.ascontiguousarray(raw, np.int16)
    ch = channels(chan)
    l_sig = C.c_uint64()
    _check(lib.rawdtw_signal_to_pa(ch.ctypes.data, len(raw), raw.ctypes.data, None, C.byref(l_sig)))
    return int(l_sig.value)


def chunk_table(raw, chan, chunk_size: int = 4000, max_num_chunk: int = 30):
    """One pass over a read: (l_sig of the whole read, raw_start).  raw_start has n_chunks + 1 entries; the kept samples of
    raw[raw_start[c] .. raw_start[c+1]) are chunk c of map_worker_for (src/rmap.cpp:685-690)."""
    lib = load_library()
    raw = np.ascontiguousarray(raw, np.int16)
    ch = channels(chan)
    start = np.zeros(int(max_num_chunk) + 1, np.uint64)
    l_sig, n = C.c_uint64(), C.c_uint32()
    _check(lib.rawdtw_signal_chunk_table(ch.ctypes.data, len(raw), raw.ctypes.data, int(chunk_size), int(max_num_chunk),
                                         C.byref(l_sig), C.byref(n), start.ctypes.data))
    return int(l_sig.value), start[:n.value + 1].copy()


def detect_events_raw_host(raw, raw_off, chan, opt=None, threads: int = 0, events_cap=None):
    """Many raw windows on the host (window k = raw[raw_off[k] .. raw_off[k+1]) with channel chan[k]) on `threads` threads.
    Returns (s_len, event_off, events)."""
    lib = load_library()
    raw = np.ascontiguousarray(raw, np.int16)
    off = np.ascontiguousarray(raw_off, np.uint64)
    n = len(off) - 1
    ch = channels(chan, n)
    cap = int(off[-1] - off[0]) if events_cap is None else int(events_cap)
    s_len = np.zeros(max(n, 1), np.uint32)
    eoff = np.zeros(n + 1, np.uint64)
    ev = np.empty(max(cap, 1), np.float32)
    st = lib.rawdtw_detect_raw_host(_opt(opt), n, off.ctypes.data, raw.ctypes.data, ch.ctypes.data, s_len.ctypes.data, eoff.ctypes.data,
                                    ev.ctypes.data, cap, int(threads))
    if st != 0:
        from ._lib import RawDTWError

        err = RawDTWError(st, lib.rawdtw_status_string(st).decode())
        err.event_off, err.s_len = eoff, s_len[:n]
        raise err
    return s_len[:n], eoff, ev[:int(eoff[-1])].copy()
