"""The restated std::sort (rawalign_amd/csrc/rawdtw_sort_order.h, exported as rawdtw_sort_by_chaining_score_restated: the order the device's
chaining gives a read's chains under "chain_max_chains") against the yardstick, rawdtw_sort_by_chaining_score, which calls std::sort itself --
permutation for permutation.  Every n from 0 to 300, 1 000 and 4 096; scores from alphabets of 1, 2, 3, 5, 17 and n values; random,
ascending, descending, all equal and organ-pipe.

The heap phase is reached only by inputs built against the sort: ADVERSARY_100 is McIlroy's adversary run against std::sort
(tests/abi/sort_adversary.cpp: a comparator that decides values lazily), its assigned values frozen here so that the test does not
depend on rebuilding it; the helper is rebuilt as well and what it gives on this machine's library must reach the heap phase too.

tests/abi/sort_order.cpp is the same comparison as a program of its own, built plain and with AddressSanitizer +
UndefinedBehaviorSanitizer (its own main, exact-size arrays for the permutation and the stack: nothing is preloaded)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rawalign_amd as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")
RAN_PARTITION, RAN_HEAP = 1, 2
SIZES = list(range(301)) + [1000, 4096]
RANDOM_DRAWS = 8
CASES = len(SIZES) * 6 * (RANDOM_DRAWS + 4)

# ./sort_adversary 100 against libstdc++'s std::sort, frozen
ADVERSARY_100 = [107, 199, 129, 197, 115, 195, 131, 193, 100, 191, 133, 189, 117, 187, 135, 185, 109, 183, 137, 181, 119, 179, 176, 177, 102, 104, 106,
                 108, 110, 112, 114, 116, 118, 120, 122, 124, 126, 128, 130, 132, 134, 136, 105, 121, 111, 123, 103, 125, 113, 127, 200, 198, 196, 194,
                 192, 190, 188, 186, 184, 182, 180, 178, 138, 141, 140, 143, 142, 145, 144, 147, 146, 149, 148, 151, 150, 153, 152, 155, 154, 157, 156,
                 159, 158, 161, 160, 163, 162, 165, 164, 167, 166, 169, 168, 171, 170, 173, 172, 175, 174, 139]


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def both(lib, scores):
    s = np.ascontiguousarray(scores, np.float32)
    want, got = np.zeros(len(s) + 1, np.uint32), np.full(len(s) + 1, 0xffffffff, np.uint32)
    phases = C.c_uint32(99)
    assert lib.rawdtw_sort_by_chaining_score(vp(s), len(s), vp(want)) == 0
    assert lib.rawdtw_sort_by_chaining_score_restated(vp(s), len(s), vp(got), C.byref(phases)) == 0
    assert got[len(s)] == 0xffffffff   # (nothing written behind the permutation)
    return want[:len(s)], got[:len(s)], phases.value


def cases():
    rng = np.random.default_rng(512)
    for n in SIZES:
        i = np.arange(n)
        for alphabet in (1, 2, 3, 5, 17, max(n, 1)):
            for _ in range(RANDOM_DRAWS):
                yield n, alphabet, "random", rng.integers(0, alphabet, n)
            yield n, alphabet, "ascending", i * alphabet // max(n, 1)
            yield n, alphabet, "descending", (n - 1 - i) * alphabet // max(n, 1)
            yield n, alphabet, "equal", np.full(n, alphabet - 1)
            yield n, alphabet, "organ-pipe", (np.minimum(i, n - 1 - i) * 2 * alphabet // max(n, 1)) % alphabet


def test_the_restated_sort_gives_std_sorts_permutation():
    lib = ra.load_library()
    count, partitioned, heaped = 0, 0, 0
    for n, alphabet, order, x in cases():
        want, got, phases = both(lib, 10.0 + x)
        assert np.array_equal(want, got), (n, alphabet, order)
        assert bool(phases & RAN_PARTITION) == (n > 16), (n, phases)   # (the introsort loop runs exactly above 16 elements)
        count += 1
        partitioned += bool(phases & RAN_PARTITION)
        heaped += bool(phases & RAN_HEAP)
    assert count == CASES and count >= 20000
    assert partitioned > 10000
    print("cases", count, "partitioned", partitioned, "reached the heap phase", heaped)


def test_the_frozen_adversary_reaches_the_heap_phase_and_the_orders_agree():
    lib = ra.load_library()
    want, got, phases = both(lib, ADVERSARY_100)
    assert len(ADVERSARY_100) >= 64 and phases & RAN_HEAP and phases & RAN_PARTITION
    assert np.array_equal(want, got)
    for d in (2, 3, 7):   # the same shape with ties in it
        want_d, got_d, _ = both(lib, np.asarray(ADVERSARY_100) // d)
        assert np.array_equal(want_d, got_d), d
    # a NULL phases word, no elements
    s = np.asarray(ADVERSARY_100, np.float32)
    out = np.zeros(len(s), np.uint32)
    assert lib.rawdtw_sort_by_chaining_score_restated(vp(s), len(s), vp(out), None) == 0 and np.array_equal(out, want)
    assert lib.rawdtw_sort_by_chaining_score_restated(None, 0, None, None) == 0
    assert lib.rawdtw_sort_by_chaining_score_restated(None, 3, vp(out), None) == 1   # RAWDTW_ERR_INVALID


@pytest.fixture(scope="module")
def adversary_exe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("adversary")), "sort_adversary")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "abi", "sort_adversary.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("n", [64, 100, 300, 1000, 4096])
def test_an_adversary_built_against_this_machines_std_sort(adversary_exe, n):
    run = subprocess.run([adversary_exe, str(n)], capture_output=True, text=True, timeout=60, check=True)
    scores = [int(x) for x in run.stdout.split()]
    assert len(scores) == n
    want, got, phases = both(ra.load_library(), scores)
    assert phases & RAN_HEAP, (n, phases)
    assert np.array_equal(want, got), n


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_the_header_in_a_program_of_its_own(tmp_path, flags):
    exe = os.path.join(str(tmp_path), "sort_order")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "abi", "sort_order.cpp"), "-o", exe], check=True)
    frozen = os.path.join(str(tmp_path), "adversary_100.txt")
    with open(frozen, "w") as f:
        f.write("\n".join(str(x) for x in ADVERSARY_100) + "\n")
    run = subprocess.run([exe, frozen], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    words = run.stdout.split()
    assert words[0] == "ok" and int(words[1]) == CASES + 1 and int(words[3]) >= 1, run.stdout + run.stderr
