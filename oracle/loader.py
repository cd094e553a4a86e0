"""ctypes loaders for the CPU oracle (TEST INFRASTRUCTURE).

Only tests/, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may
import this module; the product package ``rawalign_amd`` never does.

* ``Oracle``  -- our C restatement (oracle/liboracle.so, built from source anywhere gcc is).
* ``RefDTW``  -- the reference's own ``src/dtw.cpp`` (oracle/_ref/libref_dtw.so), prebuilt in the
                 build container where /root/reference exists; ``None`` when the file is absent.
* ``RefMap``  -- the reference's own mapping code, ``src/rmap.cpp`` and the units it calls (oracle/_ref/libref_map0.so with
                 contraction off, libref_map1.so as an FMA host builds it), behind oracle/ref_map_wrap.cpp: an index from signal
                 arrays, seed hits, one chunk round (``gen_chains`` + the stop rule), ``align_chain``, ``map_worker_for``.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")

# must match rawdtw_job_t in include/rawdtw.h (and orc_job_t / ref_job)
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

ANCHOR_DTYPE = np.dtype([("target_position", "<u4"), ("query_position", "<u4")])


class OrcOpt(C.Structure):
    _fields_ = [
        ("border_constraint", C.c_int),
        ("fill_method", C.c_int),
        ("band_radius_frac", C.c_float),
        ("match_bonus", C.c_float),
        ("min_score", C.c_float),
        ("fused_score", C.c_int),
    ]


class OrcStats(C.Structure):
    _fields_ = [("dtw_calls", C.c_uint64), ("cells", C.c_uint64)]


def build_oracle(march_native: bool = False) -> str:
    """(Re)build oracle/liboracle.so with gcc; returns its path."""
    args = ["make", "-C", HERE, "liboracle.so"]
    if march_native:
        args.append("ORC_MARCH=-march=native")
    subprocess.run(args, check=True, capture_output=True)
    return os.path.join(HERE, "liboracle.so")


def build_ref() -> str | None:
    """Build oracle/_ref from /root/reference (only where it exists)."""
    if not os.path.isdir("/root/reference/src"):
        return None
    subprocess.run(["make", "-C", HERE, "ref"], check=True, capture_output=True)
    return os.path.join(HERE, "_ref", "libref_dtw.so")


def _as_f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


class Oracle:
    def __init__(self, path: str | None = None):
        path = path or os.path.join(HERE, "liboracle.so")
        if not os.path.exists(path):
            build_oracle()
        L = C.CDLL(path)
        self.lib = L
        L.orc_dtw_global.restype = C.c_float
        L.orc_dtw_global.argtypes = [f32p, C.c_uint32, f32p, C.c_uint32, C.c_int]
        L.orc_dtw_banded.restype = C.c_float
        L.orc_dtw_banded.argtypes = [f32p, C.c_uint32, f32p, C.c_uint32, C.c_int, C.c_int]
        L.orc_dtw_banded_cellset.restype = C.c_float
        L.orc_dtw_banded_cellset.argtypes = [
            f32p, C.c_uint32, f32p, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_void_p,
        ]
        L.orc_banded_cells.restype = C.c_uint64
        L.orc_banded_cells.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
        L.orc_dtw_global_tb.restype = C.c_float
        L.orc_dtw_global_tb.argtypes = [
            f32p, C.c_uint32, f32p, C.c_uint32, C.c_int, u32p, u32p, f32p, C.POINTER(C.c_uint32),
        ]
        L.orc_dtw_directions.restype = None
        L.orc_dtw_directions.argtypes = [f32p, C.c_uint32, f32p, C.c_uint32, u8p]
        L.orc_align_chain.restype = C.c_float
        L.orc_align_chain.argtypes = [
            C.c_void_p, C.c_uint32, f32p, f32p, C.POINTER(OrcOpt), C.c_float, C.POINTER(OrcStats),
        ]
        L.orc_align_chain_cigar.restype = C.c_float
        L.orc_align_chain_cigar.argtypes = [
            C.c_void_p, C.c_uint32, f32p, f32p, C.POINTER(OrcOpt), u64p, u64p, f32p,
            C.POINTER(C.c_uint64), C.POINTER(C.c_float),
        ]
        L.orc_batch_costs.restype = None
        L.orc_batch_costs.argtypes = [C.c_void_p, C.c_uint64, f32p, f32p, f32p, C.c_int]
        L.orc_batch_costs_reps.restype = None
        L.orc_batch_costs_reps.argtypes = [C.c_void_p, C.c_uint64, f32p, f32p, f32p, C.c_int, C.c_int]

    # --- single calls -------------------------------------------------------
    def dtw_global(self, a, b, exclude_last=False) -> np.float32:
        a, b = _as_f32(a), _as_f32(b)
        return np.float32(self.lib.orc_dtw_global(a, len(a), b, len(b), int(exclude_last)))

    def dtw_banded(self, a, b, band_radius, exclude_last=False) -> np.float32:
        a, b = _as_f32(a), _as_f32(b)
        return np.float32(
            self.lib.orc_dtw_banded(a, len(a), b, len(b), int(band_radius), int(exclude_last))
        )

    def dtw_banded_cellset(self, a, b, band_radius, exclude_last=False):
        a, b = _as_f32(a), _as_f32(b)
        n_long, n_short = max(len(a), len(b)), min(len(a), len(b))
        mask = np.zeros((n_long, n_short), dtype=np.uint8)
        cells = C.c_uint64(0)
        cost = self.lib.orc_dtw_banded_cellset(
            a, len(a), b, len(b), int(band_radius), int(exclude_last), C.byref(cells),
            mask.ctypes.data_as(C.c_void_p),
        )
        return np.float32(cost), int(cells.value), mask

    def banded_cells(self, n, m, band_radius) -> int:
        return int(self.lib.orc_banded_cells(int(n), int(m), int(band_radius)))

    def dtw_global_tb(self, a, b, exclude_last=False):
        a, b = _as_f32(a), _as_f32(b)
        cap = len(a) + len(b) - 1
        pi = np.zeros(cap, np.uint32)
        pj = np.zeros(cap, np.uint32)
        pd = np.zeros(cap, np.float32)
        ln = C.c_uint32(0)
        cost = self.lib.orc_dtw_global_tb(a, len(a), b, len(b), int(exclude_last), pi, pj, pd, C.byref(ln))
        k = ln.value
        return np.float32(cost), pi[:k].copy(), pj[:k].copy(), pd[:k].copy()

    def dtw_directions(self, a, b) -> np.ndarray:
        a, b = _as_f32(a), _as_f32(b)
        d = np.zeros((len(a), len(b)), np.uint8)
        self.lib.orc_dtw_directions(a, len(a), b, len(b), d)
        return d

    # --- chains ---------------------------------------------------------------
    def align_chain(self, anchors, ref_events, read_events, opt: OrcOpt, min_score=-1e10, stats=None):
        anchors = np.ascontiguousarray(anchors, dtype=ANCHOR_DTYPE)
        st = stats if stats is not None else OrcStats()
        return np.float32(
            self.lib.orc_align_chain(
                anchors.ctypes.data_as(C.c_void_p), len(anchors), _as_f32(ref_events),
                _as_f32(read_events), C.byref(opt), C.c_float(min_score), C.byref(st),
            )
        )

    def align_chain_cigar(self, anchors, ref_events, read_events, opt: OrcOpt):
        anchors = np.ascontiguousarray(anchors, dtype=ANCHOR_DTYPE)
        cap = 0
        parts = len(anchors) - 1
        if opt.border_constraint == 0:
            cap = int(anchors[0]["query_position"] - anchors[-1]["query_position"] + 1) + int(
                anchors[0]["target_position"] - anchors[-1]["target_position"] + 1
            )
        else:
            for p in range(parts):
                s, e = anchors[parts - p], anchors[parts - p - 1]
                cap += int(e["query_position"] - s["query_position"] + 1) + int(
                    e["target_position"] - s["target_position"] + 1
                )
        cap = max(cap, 1)
        pi = np.zeros(cap, np.uint64)
        pj = np.zeros(cap, np.uint64)
        pd = np.zeros(cap, np.float32)
        ln = C.c_uint64(0)
        cost = C.c_float(0)
        score = self.lib.orc_align_chain_cigar(
            anchors.ctypes.data_as(C.c_void_p), len(anchors), _as_f32(ref_events), _as_f32(read_events),
            C.byref(opt), pi, pj, pd, C.byref(ln), C.byref(cost),
        )
        if ln.value == 2**64 - 1:
            raise AssertionError("global+banded+cigar is not implemented (rmap.cpp:223-225)")
        k = ln.value
        return np.float32(score), np.float32(cost.value), pi[:k].copy(), pj[:k].copy(), pd[:k].copy()

    def batch_costs(self, jobs, events, ref, nthreads=1, reps=1) -> np.ndarray:
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        out = np.zeros(len(jobs), np.float32)
        self.lib.orc_batch_costs_reps(
            jobs.ctypes.data_as(C.c_void_p), len(jobs), _as_f32(events), _as_f32(ref), out, int(nthreads), int(reps)
        )
        return out


class RefDTW:
    """The reference's own compiled dtw.cpp (oracle/_ref/libref_dtw.so)."""

    def __init__(self, path: str | None = None):
        path = path or os.path.join(HERE, "_ref", "libref_dtw.so")
        L = C.CDLL(path)
        self.lib = L
        for name in ("ref_dtw_global", "ref_dtw_global_slow"):
            fn = getattr(L, name)
            fn.restype = C.c_float
            fn.argtypes = [f32p, C.c_uint32, f32p, C.c_uint32, C.c_int]
        for name in ("ref_dtw_banded", "ref_dtw_slantedbanded"):
            fn = getattr(L, name)
            fn.restype = C.c_float
            fn.argtypes = [f32p, C.c_uint32, f32p, C.c_uint32, C.c_int, C.c_int]
        L.ref_dtw_global_tb.restype = C.c_float
        L.ref_dtw_global_tb.argtypes = [
            f32p, C.c_uint32, f32p, C.c_uint32, C.c_int, u32p, u32p, f32p, C.POINTER(C.c_uint32),
        ]
        L.ref_batch_costs.restype = None
        L.ref_batch_costs.argtypes = [C.c_void_p, C.c_uint64, f32p, f32p, f32p, C.c_int]
        L.ref_batch_costs_reps.restype = None
        L.ref_batch_costs_reps.argtypes = [C.c_void_p, C.c_uint64, f32p, f32p, f32p, C.c_int, C.c_int]

    @staticmethod
    def available(path: str | None = None) -> bool:
        return os.path.exists(path or os.path.join(HERE, "_ref", "libref_dtw.so"))

    def dtw_global(self, a, b, exclude_last=False):
        a, b = _as_f32(a), _as_f32(b)
        return np.float32(self.lib.ref_dtw_global(a, len(a), b, len(b), int(exclude_last)))

    def dtw_global_slow(self, a, b, exclude_last=False):
        a, b = _as_f32(a), _as_f32(b)
        return np.float32(self.lib.ref_dtw_global_slow(a, len(a), b, len(b), int(exclude_last)))

    def dtw_banded(self, a, b, band_radius, exclude_last=False):
        a, b = _as_f32(a), _as_f32(b)
        return np.float32(self.lib.ref_dtw_banded(a, len(a), b, len(b), int(band_radius), int(exclude_last)))

    def dtw_slantedbanded(self, a, b, band_radius, exclude_last=False):
        a, b = _as_f32(a), _as_f32(b)
        return np.float32(
            self.lib.ref_dtw_slantedbanded(a, len(a), b, len(b), int(band_radius), int(exclude_last))
        )

    def dtw_global_tb(self, a, b, exclude_last=False):
        a, b = _as_f32(a), _as_f32(b)
        cap = len(a) + len(b) - 1
        pi = np.zeros(cap, np.uint32)
        pj = np.zeros(cap, np.uint32)
        pd = np.zeros(cap, np.float32)
        ln = C.c_uint32(0)
        cost = self.lib.ref_dtw_global_tb(a, len(a), b, len(b), int(exclude_last), pi, pj, pd, C.byref(ln))
        k = ln.value
        return np.float32(cost), pi[:k].copy(), pj[:k].copy(), pd[:k].copy()

    def batch_costs(self, jobs, events, ref, nthreads=1, reps=1) -> np.ndarray:
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        out = np.zeros(len(jobs), np.float32)
        self.lib.ref_batch_costs_reps(
            jobs.ctypes.data_as(C.c_void_p), len(jobs), _as_f32(events), _as_f32(ref), out, int(nthreads), int(reps)
        )
        return out


class RefMapOpt(C.Structure):
    """rm_opt of oracle/ref_map_wrap.cpp: the ri_mapopt_t fields the mapping code reads, laid over ri_mapopt_init"""
    _fields_ = [
        ("flag", C.c_int64),
        ("chunk_size", C.c_uint32), ("min_events", C.c_uint32), ("max_num_chunk", C.c_uint32),
        ("max_gap_length", C.c_uint32), ("max_target_gap_length", C.c_uint32), ("chaining_band_length", C.c_uint32),
        ("max_num_skips", C.c_uint32), ("min_num_anchors", C.c_uint32), ("num_best_chains", C.c_uint32),
        ("min_chaining_score", C.c_float),
        ("min_chain_anchor", C.c_uint32), ("dtw_border_constraint", C.c_uint32), ("dtw_fill_method", C.c_uint32),
        ("dtw_band_radius_frac", C.c_float), ("dtw_match_bonus", C.c_float), ("dtw_min_score", C.c_float),
        ("min_bestmap_ratio", C.c_float), ("min_meanmap_ratio", C.c_float),
    ]


class RefMap:
    """The reference's own mapping code (oracle/_ref/libref_map{0,1}.so: src/rmap.cpp and the units it calls, compiled where
    they lie; oracle/ref_map_wrap.cpp is the glue).  `fused` picks the build: False = contraction off (the source's
    arithmetic), True = the reference's flags on an FMA target (rmap.cpp:306 is one fused multiply-subtract).  One index a
    handle, built in memory from signal arrays with the parameters of ri_idxopt_init (rawindex.cpp:465-472)."""

    CHAIN_FIELDS = ("reference_sequence_index", "strand", "start_position", "end_position", "n_anchors", "mapq")

    def __init__(self, forward, reverse, names=None, fused: bool = False, e=6, q=9, lq=3, k=6, w=0, n=0, b=14):
        L = C.CDLL(self.path(fused))
        self.lib = L
        VP, U32, U64, F32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        L.rm_create.restype = VP
        L.rm_create.argtypes = [U32, VP, VP, u32p, VP] + [C.c_int] * 7
        L.rm_opt_defaults.argtypes = [C.POINTER(RefMapOpt)]
        L.rm_set_opt.argtypes = [VP, C.POINTER(RefMapOpt)]
        L.rm_reset_reads.argtypes = [VP]
        L.rm_new_read.restype = U32
        L.rm_new_read.argtypes = [VP]
        L.rm_hits.restype = U64
        L.rm_hits.argtypes = [VP, f32p, U32]
        L.rm_hits_get.argtypes = [VP, u32p]
        L.rm_round.restype = C.c_int
        L.rm_round.argtypes = [VP, U32, f32p, U32]
        L.rm_chain_counts.argtypes = [VP, U32, C.POINTER(U32), C.POINTER(U64), C.POINTER(U32)]
        L.rm_chains_get.argtypes = [VP, U32, f32p, f32p, u32p, u32p]
        L.rm_align_chain.restype = F32
        L.rm_align_chain.argtypes = [VP, u32p, U32, U32, C.c_int, f32p, U32, C.c_int, F32]
        L.rm_tb_len.restype = U64
        L.rm_tb_len.argtypes = [VP, C.POINTER(F32)]
        L.rm_tb_get.argtypes = [VP, u64p, u64p, f32p]
        L.rm_map_read.argtypes = [VP, f32p, U32, u32p]
        L.rm_read_events.restype = U32
        L.rm_read_events.argtypes = [VP, U32, VP]
        L.rm_last_read.restype = U32
        L.rm_last_read.argtypes = [VP]
        L.rm_tags.restype = C.c_char_p
        L.rm_tags.argtypes = [VP]
        L.rm_detect_events.restype = U32
        L.rm_detect_events.argtypes = [VP, f32p, U32, f32p]
        self.fused = bool(fused)
        fwd = [_as_f32(x) for x in forward]
        rev = [_as_f32(x) for x in reverse]
        names = list(names) if names is not None else [f"seq{s}" for s in range(len(fwd))]
        pf = (C.c_void_p * len(fwd))(*[x.ctypes.data for x in fwd])
        pr = (C.c_void_p * len(rev))(*[x.ctypes.data for x in rev])
        pn = (C.c_char_p * len(names))(*[s.encode() for s in names])
        lens = np.array([len(x) for x in fwd], np.uint32)
        self._h = L.rm_create(len(fwd), pf, pr, lens, pn, b, w, e, n, q, lq, k)
        self.n_seq = len(fwd)

    @staticmethod
    def path(fused: bool = False) -> str:
        return os.path.join(HERE, "_ref", "libref_map1.so" if fused else "libref_map0.so")

    @staticmethod
    def available() -> bool:
        return os.path.exists(RefMap.path(False)) and os.path.exists(RefMap.path(True))

    def default_opt(self) -> RefMapOpt:
        o = RefMapOpt()
        self.lib.rm_opt_defaults(C.byref(o))
        return o

    def set_opt(self, **fields) -> RefMapOpt:
        """ri_mapopt_init, then the named fields"""
        o = self.default_opt()
        for k, v in fields.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        self.lib.rm_set_opt(self._h, C.byref(o))
        return o

    def reset_reads(self):
        self.lib.rm_reset_reads(self._h)

    def new_read(self) -> int:
        return int(self.lib.rm_new_read(self._h))

    def hits(self, events) -> np.ndarray:
        """seed hits of a chunk's events, in the order gen_chains meets them: rows (sequence, strand, target, query in the chunk)"""
        ev = _as_f32(events)
        n = int(self.lib.rm_hits(self._h, ev, len(ev)))
        out = np.zeros(max(n, 1) * 4, np.uint32)
        self.lib.rm_hits_get(self._h, out)
        return out[:n * 4].reshape(n, 4)

    def round(self, rid: int, chunk_events) -> bool:
        """one chunk round (the events are appended, gen_chains runs unless the chunk is shorter than min_events); the stop rule"""
        ev = _as_f32(chunk_events)
        ev_ = ev if len(ev) else np.zeros(1, np.float32)
        return bool(self.lib.rm_round(self._h, int(rid), ev_, len(ev)))

    def chains(self, rid: int):
        """reg->chains: (list of dicts with chaining_score / alignment_score as float32, the CHAIN_FIELDS, anchors), reg->offset"""
        nc, na, off = C.c_uint32(), C.c_uint64(), C.c_uint32()
        self.lib.rm_chain_counts(self._h, int(rid), C.byref(nc), C.byref(na), C.byref(off))
        n = nc.value
        cs, al = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
        fields = np.zeros(max(n, 1) * 6, np.uint32)
        anch = np.zeros(max(na.value, 1) * 2, np.uint32)
        self.lib.rm_chains_get(self._h, int(rid), cs, al, fields, anch)
        out, at = [], 0
        for c in range(n):
            d = dict(zip(self.CHAIN_FIELDS, (int(x) for x in fields[6 * c:6 * c + 6])))
            d["chaining_score"], d["alignment_score"] = cs[c], al[c]
            a = np.zeros(d["n_anchors"], ANCHOR_DTYPE)
            a["target_position"] = anch[2 * at:2 * (at + d["n_anchors"]):2]
            a["query_position"] = anch[2 * at + 1:2 * (at + d["n_anchors"]):2]
            d["anchors"] = a
            at += d["n_anchors"]
            out.append(d)
        return out, off.value

    def align_chain(self, anchors, seq: int, strand: int, read_events, cigar: bool = False, min_score: float = -1e10):
        """the reference's align_chain (rmap.cpp:181); score as float32, with cigar also (cost, i, j, difference)"""
        a = np.ascontiguousarray(anchors, ANCHOR_DTYPE)
        flat = np.zeros(max(len(a), 1) * 2, np.uint32)
        flat[0:2 * len(a):2] = a["target_position"]
        flat[1:2 * len(a):2] = a["query_position"]
        ev = _as_f32(read_events)
        s = np.float32(self.lib.rm_align_chain(self._h, flat, len(a), int(seq), int(strand), ev, len(ev), int(bool(cigar)),
                                               C.c_float(min_score)))
        if not cigar:
            return s
        cost = C.c_float()
        n = int(self.lib.rm_tb_len(self._h, C.byref(cost)))
        pi, pj, pd = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.float32)
        self.lib.rm_tb_get(self._h, pi, pj, pd)
        return s, (np.float32(cost.value), pi[:n], pj[:n], pd[:n])

    def detect_events(self, sig) -> np.ndarray:
        """the reference's detect_events (revent.c:190) on one chunk of raw signal, with the handle's options"""
        s = _as_f32(sig)
        out = np.zeros(len(s) + 1, np.float32)
        n = int(self.lib.rm_detect_events(self._h, s, len(s), out))
        return out[:n].copy()

    def map_read(self, sig):
        """a whole raw read through map_worker_for (rmap.cpp:667): the record left in reg0, the tags without mt:f:, the read's events"""
        s = _as_f32(sig)
        out = np.zeros(9, np.uint32)
        self.lib.rm_map_read(self._h, s, len(s), out)
        keys = ("mapped", "ref_id", "read_start_position", "read_end_position", "read_length", "fragment_start_position",
                "fragment_length", "mapq", "rev")
        rec = dict(zip(keys, (int(x) for x in out)))
        rec["tags"] = self.lib.rm_tags(self._h).decode()
        rid = int(self.lib.rm_last_read(self._h))
        n = int(self.lib.rm_read_events(self._h, rid, None))
        ev = np.zeros(max(n, 1), np.float32)
        self.lib.rm_read_events(self._h, rid, ev.ctypes.data_as(C.c_void_p))
        rec["events"] = ev[:n]
        return rec
