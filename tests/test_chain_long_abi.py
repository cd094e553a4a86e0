"""rawdtw_chain_round_stats and rawdtw_get_option (include/rawdtw.h) without a device: the symbols, their declared signatures, the binding
table's entries, the refusal of a null context, and the header still compiling as C99."""
import ctypes as C
import os
import re
import subprocess

from rawalign_amd._lib import SYMBOLS, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
VP, I32 = C.c_void_p, C.c_int


def _norm(s):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", s, flags=re.S)).replace("( ", "(").replace(" )", ")").strip()


def test_the_stats_entry_exists_with_the_declared_signature():
    lib = load_library()
    text = open(os.path.join(ROOT, "include", "rawdtw.h")).read()
    header = _norm(text)
    assert hasattr(lib, "rawdtw_chain_round_stats") and hasattr(lib, "rawdtw_get_option")
    assert "int rawdtw_chain_round_stats(const rawdtw_ctx *ctx, uint64_t *rounds, uint64_t *long_reads, uint64_t *long_seeds, uint64_t *far_steps);" in header
    assert "int rawdtw_get_option(const rawdtw_ctx *ctx, const char *name, int64_t *value);" in header
    assert SYMBOLS["rawdtw_chain_round_stats"] == (I32, [VP, VP, VP, VP, VP])
    assert SYMBOLS["rawdtw_get_option"] == (I32, [VP, C.c_char_p, C.POINTER(C.c_int64)])
    assert '"chain_long_seeds"' in text   # (the option is documented there)


def test_a_null_context_is_refused():
    lib = load_library()
    v = C.c_uint64(7)
    assert lib.rawdtw_chain_round_stats(None, C.byref(v), None, None, None) == INVALID and v.value == 7
    assert lib.rawdtw_chain_round_stats(None, None, None, None, None) == INVALID
    x = C.c_int64(7)
    assert lib.rawdtw_get_option(None, b"chain_long_seeds", C.byref(x)) == INVALID and x.value == 7


def test_the_header_still_compiles_as_c99():
    subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "abi", "c99_include.c")], check=True)
