"""Record tests/golden/detect_events_ref.npz: detect_events (src/revent.c:190-210) of the reference itself on every case of
tests/events_cases.py, in two builds:
  plain       gcc -O3 -ffp-contract=off -march=x86-64-v3   (one rounding per operation, as the source reads)
  contracted  gcc -O3 -march=x86-64-v3                     (GCC fuses multiply-adds, as the reference's Makefile builds C on an FMA host)
revent.c and kalloc.c are compiled where they lie, with a small shim of our own, into a temporary directory outside the
tree; nothing compiled is kept.  Per case and build the fixture holds n_events and the SHA-256 of the events' bits with
every NaN canonicalised, and once the SHA-256 of all inputs.  Usage: python scripts/make_golden_events.py [REFERENCE_SRC]"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.events_cases import cases, events_sha256, inputs_sha256  # noqa: E402

SHIM = r"""
#include <stdlib.h>
#include <string.h>
#include "roptions.h"
#include "revent.h"
uint32_t shim_detect(uint32_t s_len, const float *sig, uint32_t w1, uint32_t w2, float t1, float t2, float ph, float *out)
{
    ri_mapopt_t opt;
    memset(&opt, 0, sizeof opt);
    opt.window_length1 = w1; opt.window_length2 = w2;
    opt.threshold1 = t1; opt.threshold2 = t2; opt.peak_height = ph;
    uint32_t n = 0; /* rmap.cpp:547 */
    float *ev = detect_events(0, s_len, sig, &opt, &n);
    if (ev) { memcpy(out, ev, (size_t)n * sizeof(float)); free(ev); }
    return n;
}
"""
FORMS = {"plain": ["-O3", "-ffp-contract=off", "-march=x86-64-v3"], "contracted": ["-O3", "-march=x86-64-v3"]}
OUT = os.path.join(ROOT, "tests", "golden", "detect_events_ref.npz")


def build(src, tmp, form):
    shim = os.path.join(tmp, "shim.c")
    with open(shim, "w") as f:
        f.write(SHIM)
    so = os.path.join(tmp, f"ref_events_{form}.so")
    subprocess.run(["gcc", *FORMS[form], "-shared", "-fPIC", "-I", src, "-o", so, shim, os.path.join(src, "revent.c"),
                    os.path.join(src, "kalloc.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.shim_detect.restype = C.c_uint32
    lib.shim_detect.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p]
    return lib


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    if not os.path.isfile(os.path.join(src, "revent.c")):
        sys.exit(f"{src}/revent.c not found: the reference's sources are needed to record the fixture")
    cs = cases()
    rec = {"names": np.array([c[0] for c in cs]), "inputs_sha256": np.array(inputs_sha256(cs))}
    with tempfile.TemporaryDirectory() as tmp:
        for form in FORMS:
            lib = build(src, tmp, form)
            n = np.zeros(len(cs), np.uint32)
            dig = np.zeros((len(cs), 32), np.uint8)
            for k, (_, sig, o) in enumerate(cs):
                sig = np.ascontiguousarray(sig, np.float32)
                out = np.zeros(len(sig), np.float32)
                n[k] = lib.shim_detect(len(sig), sig.ctypes.data, o[0], o[1], o[2], o[3], o[4], out.ctypes.data)
                dig[k] = np.frombuffer(events_sha256(out[:n[k]]), np.uint8)
            rec[f"n_events_{form}"] = n
            rec[f"sha256_{form}"] = dig
    np.savez_compressed(OUT, **rec)
    differ = int(np.sum(np.any(rec["sha256_plain"] != rec["sha256_contracted"], axis=1)))
    print(f"{OUT}: {len(cs)} cases, {int(rec['n_events_plain'].sum())} events (plain), {differ} cases differ between the forms, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
