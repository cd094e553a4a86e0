"""RawAlign `.ind` index files: reader for what the DTW path needs (sequence table + per-strand
reference signal arrays, src/rawindex.cpp:317-377) and a writer of the same format
(src/rawindex.cpp:275-315) used to make synthetic indices for tests and benchmarks.  The hash
buckets are written empty unless write_index is asked for them (buckets=); seeding.SeedIndex.from_index reads them."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from ._lib import load_library

RI_IDX_MAGIC = b"RI"  # src/rawindex.h:7-8, two bytes


class Index:
    def __init__(self, path: str):
        self.lib = load_library()
        h = C.c_void_p()
        st = self.lib.rawdtw_index_open(path.encode(), C.byref(h))
        if st != 0:
            raise ValueError(f"{path}: not a RawAlign index (status {st})")
        self._h = h
        n = C.c_uint32()
        pars = (C.c_uint32 * 8)()
        self.lib.rawdtw_index_info(h, C.byref(n), pars)
        self.n_seq = n.value
        self.w, self.e, self.n, self.q, self.lq, self.k, _, self.flag = [int(x) for x in pars]
        self.names, self.lens = [], []
        for i in range(self.n_seq):
            name, ln = C.c_char_p(), C.c_uint32()
            self.lib.rawdtw_index_seq(h, i, C.byref(name), C.byref(ln))
            self.names.append((name.value or b"").decode())
            self.lens.append(ln.value)

    def signal(self, seq: int, strand: int) -> np.ndarray:
        out = np.empty(self.lens[seq], np.float32)
        st = self.lib.rawdtw_index_read_signal(self._h, seq, strand, out.ctypes.data_as(C.c_void_p))
        if st != 0:
            raise IOError("short index file")
        return out

    def upload(self, engine):
        """Stream every sequence's forward/reverse signal into the engine's reference arena."""
        engine._check(self.lib.rawdtw_index_upload(engine._ctx, self._h))

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.lib.rawdtw_index_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _bucket_bytes(seed_index, b: int) -> bytes:
    """ri_idx_dump's bucket part (src/rawindex.cpp:297-312) of a seeding.SeedIndex: per bucket u32 n, n x u64 positions, u32
    size, size x (u64 key, u64 val); key = hash >> b << 1, | 1 with val = the one position, else val = start << 32 | count."""
    keys = np.sort(seed_index.keys())
    per = [[] for _ in range(1 << b)]
    for h in keys.tolist():
        per[h & ((1 << b) - 1)].append(h)
    out = []
    for hs in per:
        pos, recs = [], []
        for h in hs:
            y = seed_index.get(h)
            if len(y) == 1:
                recs.append((h >> b << 1 | 1, int(y[0])))
            else:
                recs.append((h >> b << 1, len(pos) << 32 | len(y)))
                pos.extend(int(v) for v in y)
        out.append(struct.pack("<I", len(pos)) + np.array(pos, "<u8").tobytes() + struct.pack("<I", len(recs))
                   + np.array(recs, "<u8").reshape(-1, 2).tobytes())
    return b"".join(out)


def write_index(path: str, names, forward, reverse, w=0, e=6, n=0, q=9, lq=3, k=6, flag=0, b=14, buckets=None):
    """ri_idx_dump's layout.  buckets None: empty hash buckets (2^b of them: u32 n=0, u32 size=0).  buckets True: the seed
    index of the signals (seeding.SeedIndex.from_signals with these parameters); a seeding.SeedIndex: that one.  ri_idx_load
    reads 2^14 buckets whatever wrote the file, so a file with buckets needs b = 14."""
    if buckets is not None and buckets is not False:
        from .seeding import SeedIndex, SeedParams

        assert b == 14, "ri_idx_load always reads 2^14 buckets (src/rawindex.cpp:330)"
        six = buckets if isinstance(buckets, SeedIndex) else SeedIndex.from_signals(forward, reverse, SeedParams(w, e, n, q, lq, k))
        tail = _bucket_bytes(six, b)
    else:
        tail = b"\x00" * (8 * (1 << b))
    with open(path, "wb") as f:
        f.write(RI_IDX_MAGIC)
        f.write(struct.pack("<8I", w, e, n, q, lq, k, len(names), flag))
        for name, fw, rv in zip(names, forward, reverse):
            nb = name.encode()
            assert len(nb) < 256 and len(fw) == len(rv)
            f.write(struct.pack("<B", len(nb)))
            f.write(nb)
            f.write(struct.pack("<I", len(fw)))
            f.write(np.ascontiguousarray(fw, "<f4").tobytes())
            f.write(np.ascontiguousarray(rv, "<f4").tobytes())
        f.write(tail)
