"""The reference from bases: a FASTA and a k-mer pore model to the signal arrays ri_seq_to_sig makes (src/rsig.cpp:7-41), through the
C ABI (include/rawdtw.h).

read_fasta, read_pore_model, seq_to_sig and seq_sums run the library's host code; Engine.reference_from_bases runs the device path
(rawdtw_refsig.hip).  Both give the reference's floats bit for bit, in the plain form and in the form an FMA build contracts to."""
from __future__ import annotations

import ctypes as C
import gzip

import numpy as np

from ._lib import RawDTWError, load_library


def _check(st: int):
    if st != 0:
        raise RawDTWError(st, load_library().rawdtw_status_string(st).decode())


def as_bases(seq) -> np.ndarray:
    """a sequence as the bytes that cross the ABI: str, bytes or a uint8 array"""
    if isinstance(seq, str):
        seq = seq.encode("latin-1")
    if isinstance(seq, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(seq), np.uint8)
    return np.ascontiguousarray(seq, np.uint8)


def read_fasta(path: str):
    """[(name, bases as bytes)]: plain or .gz, the name up to the first white space, records over any number of lines"""
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    out, name, parts = [], None, []
    with (gzip.open(path, "rb") if gz else open(path, "rb")) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            if line.startswith(b">"):
                if name is not None:
                    out.append((name, b"".join(parts)))
                head = line[1:].split()
                name, parts = (head[0].decode() if head else ""), []
            elif name is not None:
                parts.append(line)
    if name is not None:
        out.append((name, b"".join(parts)))
    return out


def read_pore_model(path: str):
    """rawdtw_pore_model_load: (level_mean as float32 of 4^k slots, k)"""
    lib = load_library()
    k = C.c_uint32()
    st = lib.rawdtw_pore_model_load(str(path).encode(), C.byref(k), None, 0)
    if st != 4:  # RAWDTW_ERR_RANGE: k is known, now with room
        _check(st or 1)
    out = np.zeros(4 ** k.value, np.float32)
    _check(lib.rawdtw_pore_model_load(str(path).encode(), C.byref(k), out.ctypes.data, len(out)))
    return out, int(k.value)


def seq_to_sig(seq, pore, k: int, strand: int, contracted: bool = True) -> np.ndarray:
    """rawdtw_seq_to_sig_host: one strand (1: what the index keeps as forward, 0: reverse)"""
    b, pore = as_bases(seq), np.ascontiguousarray(pore, np.float32)
    if 1 <= int(k) <= 12 and len(pore) < 4 ** int(k):
        raise ValueError("the model has 4^k levels")
    out, n = np.zeros(max(len(b) - int(k) + 1, 1), np.float32), C.c_uint32()
    _check(load_library().rawdtw_seq_to_sig_host(b.ctypes.data, len(b), pore.ctypes.data, int(k), int(strand), int(bool(contracted)),
                                                 out.ctypes.data, C.byref(n)))
    return out[:n.value]


def seq_sums(values):
    """rawdtw_seq_sums_restated: (sum, sum2, fast steps [sum, sum2], slow steps [sum, sum2]) of float32 values"""
    v = np.ascontiguousarray(values, np.float32)
    s, s2, fast, slow = C.c_double(), C.c_double(), np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    _check(load_library().rawdtw_seq_sums_restated(v.ctypes.data, len(v), C.byref(s), C.byref(s2), fast.ctypes.data, slow.ctypes.data))
    return s.value, s2.value, fast, slow
