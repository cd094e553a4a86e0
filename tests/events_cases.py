"""Seeded inputs of the event-detection fixture (tests/golden/detect_events_ref.npz, scripts/make_golden_events.py): the cases
every form of detect_events (src/revent.c:190-210) is held to.  A case is (name, signal float32, options as the tuple
(window_length1, window_length2, threshold1, threshold2, peak_height)).  The fixture records the SHA-256 of all of them, so
a generator that drifts fails loudly instead of comparing against answers to other questions."""
import hashlib

import numpy as np

DEFAULT = (3, 6, 4.30265, 2.57058, 1.0)  # roptions.c:37-41
OPTION_SETS = {
    "alt": (7, 14, 2.5, 9.0, 1.0),        # roptions.c:56-60
    "w1_gt_w2": (6, 3, 4.30265, 2.57058, 1.0),
    "w1": (1, 6, 4.30265, 2.57058, 1.0),
    "w2": (2, 2, 4.30265, 2.57058, 1.0),
    "w1_w2": (1, 2, 4.30265, 2.57058, 1.0),
    "ph0.2": (3, 6, 4.30265, 2.57058, 0.2),
    "ph0": (3, 6, 4.30265, 2.57058, 0.0),
    "thr0": (3, 6, 0.0, 0.0, 1.0),
    "thr0_ph0": (3, 6, 0.0, 0.0, 0.0),
}
EDGE_LENGTHS = (1, 2, 5, 6, 7, 11, 12, 13, 24, 25)


def cases():
    from rawalign_amd.synth import make_raw_reads

    out = []
    rng = np.random.default_rng(2024)
    for i, s in enumerate(make_raw_reads(100, 4000, seed=1)):
        out.append((f"chunk{i}", s, DEFAULT))
    tails = rng.integers(1, 4000, 40)
    for i, s in enumerate(make_raw_reads(40, tails, seed=2)):
        out.append((f"tail{i}_{len(s)}", s, DEFAULT))
    for i, s in enumerate(make_raw_reads(len(EDGE_LENGTHS), list(EDGE_LENGTHS), seed=3)):
        out.append((f"len{len(s)}", s, DEFAULT))
    out.append(("const500", np.full(500, 90.0, np.float32), DEFAULT))
    out.append(("const4000", np.full(4000, 100.5, np.float32), DEFAULT))
    step = np.concatenate([np.full(200, 80.0), np.full(200, 110.0)]).astype(np.float32)
    out.append(("step1", step, DEFAULT))
    out.append(("step1_noisy", (step + rng.normal(0, 1.0, len(step))).astype(np.float32), DEFAULT))
    step2 = np.concatenate([np.full(150, 80.0), np.full(150, 120.0), np.full(150, 90.0)]).astype(np.float32)
    out.append(("step2", step2, DEFAULT))
    out.append(("step2_noisy", (step2 + rng.normal(0, 1.0, len(step2))).astype(np.float32), DEFAULT))
    base = make_raw_reads(6, 4000, seed=4)
    for s, off in zip(base, (1e3, 5e3, 1e4, 3e4, -300.0, -1e4)):
        out.append((f"offset{off:g}", (s.astype(np.float64) + off).astype(np.float32), DEFAULT))
    out.append(("negated", -base[0], DEFAULT))
    flat = np.full(2000, 100.0, np.float32)
    out.append(("tiny_noise", (flat + rng.normal(0, 1e-5, 2000)).astype(np.float32), DEFAULT))
    out.append(("ulp_alternate", np.where(np.arange(2000) % 2 == 0, np.float32(100.0), np.nextafter(np.float32(100.0), np.float32(200.0))).astype(np.float32), DEFAULT))
    out.append(("tiny_steps", np.repeat(np.float32(100.0) + np.float32(1e-5) * rng.integers(0, 3, 250).astype(np.float32), 8)[:2000].astype(np.float32), DEFAULT))
    for L in (65536, 250000):
        out.append((f"long{L}", make_raw_reads(1, L, seed=L)[0], DEFAULT))
    for j, (name, opt) in enumerate(OPTION_SETS.items()):
        lens = [4000] * 10 + list(rng.integers(1, 1200, 4)) + [13]
        for i, s in enumerate(make_raw_reads(len(lens), lens, seed=100 + j)):
            out.append((f"{name}_{i}_{len(s)}", s, opt))
    return out


def inputs_sha256(cs) -> str:
    h = hashlib.sha256()
    for name, sig, opt in cs:
        h.update(name.encode())
        h.update(np.asarray(opt, np.float64).tobytes())
        h.update(np.ascontiguousarray(sig, np.float32).tobytes())
    return h.hexdigest()


def events_sha256(ev) -> bytes:
    """SHA-256 of the events' bits with every NaN made one canonical NaN (any NaN equals any NaN)."""
    b = np.ascontiguousarray(ev, np.float32).view(np.uint32).copy()
    b[np.isnan(np.asarray(ev, np.float32))] = 0x7FC00000
    return hashlib.sha256(b.tobytes()).digest()
