"""Access to tests/golden/dtw_golden.npz (captured from the reference by scripts/make_golden.py) and to the vectors
scripts/make_golden_ref.py records (dtw_ref_random.npz, find_outlier_ref.npz)."""
import hashlib
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


@dataclass
class GoldenCase:
    a: np.ndarray
    b: np.ndarray
    R0: int
    exclude_last: int
    global_bits: int
    banded_bits: int
    tb: tuple | None  # (cost_bits, i, j, d_bits)


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "dtw_golden.npz"))
    vals = z["vals"]
    out = []
    for k, (n, m, R0, ex, off, tb_off) in enumerate(z["cases"]):
        a = np.ascontiguousarray(vals[off:off + n])
        b = np.ascontiguousarray(vals[off + n:off + n + m])
        tb = None
        if tb_off >= 0:
            ln = int(z["tb_len"][k])
            tb = (int(z["tb_cost"][k]), z["tb_i"][tb_off:tb_off + ln], z["tb_j"][tb_off:tb_off + ln],
                  z["tb_d"][tb_off:tb_off + ln])
        out.append(GoldenCase(a, b, int(R0), int(ex), int(z["global_"][k]), int(z["banded"][k]), tb))
    return out


def bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def golden_path(name: str) -> str:
    return os.path.join(HERE, "golden", name)


def path_digest(i, j, d) -> bytes:
    """SHA-256 of a traceback path: positions as little-endian uint32, differences as the bits of little-endian float32."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(i, "<u4").tobytes())
    h.update(np.ascontiguousarray(j, "<u4").tobytes())
    h.update(np.ascontiguousarray(d, "<f4").view("<u4").tobytes())
    return h.digest()


def dtw_random_inputs(n_cases: int = 3000, seed: int = 99):
    """The fresh random inputs test_oracle.py compares with the reference: (a, b, R0, exclude_last) per case, and the
    SHA-256 of all of them (the recorded answers are only meaningful for the same inputs)."""
    rng = np.random.default_rng(seed)
    h = hashlib.sha256()
    cases = []
    for t in range(n_cases):
        n, m = int(rng.integers(1, 120)), int(rng.integers(1, 120))
        a = rng.normal(size=n).astype(np.float32)
        b = rng.normal(size=m).astype(np.float32)
        R0 = int(rng.integers(0, 14))
        ex = t & 1
        h.update(a.astype("<f4").tobytes())
        h.update(b.astype("<f4").tobytes())
        h.update(np.array([n, m, R0, ex], "<i8").tobytes())
        cases.append((a, b, R0, ex))
    return cases, h.digest()


def load_find_outlier_golden():
    """[(x, bits of find_outlier with contraction off, bits as built on an FMA host)] (find_outlier_ref.npz)"""
    z = np.load(golden_path("find_outlier_ref.npz"))
    out, off = [], 0
    for k, (rows, cols) in enumerate(z["shapes"]):
        x = np.ascontiguousarray(z["vals"][off:off + rows * cols].reshape(rows, cols))
        off += rows * cols
        out.append((x, int(z["plain"][k]), int(z["contracted"][k])))
    return out
