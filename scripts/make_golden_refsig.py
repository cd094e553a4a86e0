"""Record tests/golden/seq_to_sig_ref.npz: ri_seq_to_sig (src/rsig.cpp:7-41) of the reference itself on every case of
tests/refsig_cases.py, in two builds:
  plain       g++ -O3 -ffp-contract=off -march=x86-64-v3   (one rounding per operation, as the source reads)
  contracted  g++ -O3 -march=x86-64-v3                     (GCC fuses multiply-adds, as the reference's Makefile builds on an FMA host)
rsig.cpp as a whole needs HDF5; the function alone does not.  At generation time it is cut out of rsig.cpp by name into a temporary
directory outside the tree, given a declaration of seq_nt4_table and compiled with rutils.c where that lies; nothing of the
reference's text and nothing compiled is kept.  Per case and build the fixture holds the SHA-256 of every strand's length and bits with
every NaN canonicalised, and once the SHA-256 of all inputs.  Usage: python scripts/make_golden_refsig.py [REFERENCE_SRC]"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.refsig_cases import cases, inputs_sha256, outputs_sha256  # noqa: E402

HEAD = """
#include <math.h>
#include <stdint.h>
extern "C" unsigned char seq_nt4_table[256];
extern "C" {
"""
FORMS = {"plain": ["-O3", "-ffp-contract=off", "-march=x86-64-v3"], "contracted": ["-O3", "-march=x86-64-v3"]}
OUT = os.path.join(ROOT, "tests", "golden", "seq_to_sig_ref.npz")


def cut_function(text: str, name: str) -> str:
    """the definition of `name` from its return type to its closing brace"""
    at = text.index("void " + name + "(")
    depth, i = 0, text.index("{", at)
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[at:j + 1]
    raise ValueError(name + ": no closing brace")


def build(src, tmp, form):
    with open(os.path.join(src, "rsig.cpp")) as f:
        body = cut_function(f.read(), "ri_seq_to_sig")
    cut = os.path.join(tmp, "cut.cpp")
    with open(cut, "w") as f:
        f.write(HEAD + body + "\n}\n")
    obj = os.path.join(tmp, f"rutils_{form}.o")
    subprocess.run(["gcc", *FORMS[form], "-fPIC", "-I", src, "-c", "-o", obj, os.path.join(src, "rutils.c")], check=True)
    so = os.path.join(tmp, f"ref_refsig_{form}.so")
    subprocess.run(["g++", *FORMS[form], "-shared", "-fPIC", "-o", so, cut, obj, "-lm"], check=True)
    lib = C.CDLL(so)
    lib.ri_seq_to_sig.restype = None
    lib.ri_seq_to_sig.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_void_p]
    return lib


def run(lib, seq: bytes, pore, k: int, strand: int) -> np.ndarray:
    out, n = np.zeros(max(len(seq), 1), np.float32), C.c_uint32()
    lib.ri_seq_to_sig(seq, len(seq), pore.ctypes.data, k, strand, C.byref(n), out.ctypes.data)
    return out[:n.value]


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    if not os.path.isfile(os.path.join(src, "rsig.cpp")):
        sys.exit(f"{src}/rsig.cpp not found: the reference's sources are needed to record the fixture")
    cs = cases()
    rec = {"names": np.array([c[0] for c in cs]), "inputs_sha256": np.array(inputs_sha256(cs))}
    total = 0
    with tempfile.TemporaryDirectory() as tmp:
        for form in FORMS:
            lib = build(src, tmp, form)
            dig = np.zeros((len(cs), 32), np.uint8)
            for i, (_, seqs, pore, k) in enumerate(cs):
                pore = np.ascontiguousarray(pore, np.float32)
                arrays = [run(lib, s, pore, k, strand) for s in seqs for strand in (1, 0)]
                total += sum(len(a) for a in arrays)
                dig[i] = np.frombuffer(outputs_sha256(arrays), np.uint8)
            rec[f"sha256_{form}"] = dig
    np.savez_compressed(OUT, **rec)
    differ = int(np.sum(np.any(rec["sha256_plain"] != rec["sha256_contracted"], axis=1)))
    print(f"{OUT}: {len(cs)} cases, {total // 2} floats a form, {differ} cases differ between the forms, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
