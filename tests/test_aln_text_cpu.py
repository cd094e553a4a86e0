"""The aln text without a device (include/rawdtw.h, "aln text").  The shared formatter rawalign_amd/csrc/rawdtw_fmt_g.h against the C
library: tests/abi/fmt_g.cpp, a stand-alone program built with g++ together with the host unit rawdtw_aln_text.cpp, plain and with
AddressSanitizer + UndefinedBehaviorSanitizer (its own main: nothing is preloaded), takes the lattice of tests/aln_text_cases.py as a file
of bit patterns and compares every value's bytes with snprintf("%g"); nothing is left out and nothing is declined.  Then
rawdtw_aln_text_host in the built library against a plain Python model, rawdtw_aln_text_bound on every case, and the mapper's setter
on mappers that never reach a device."""
import os
import subprocess

import numpy as np
import pytest

import rawalign_amd as ra
from rawalign_amd import mapper, synth
from rawalign_amd.mapping import StopOpt
from tests import aln_text_cases as A
from tests.test_mapper_cpu import _oracle_scorer
from tests.util import OracleScorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rawalign_amd", "csrc")
BUILDS = {"plain": ("-O2",), "asan_ubsan": ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")}


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request, tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("fmt_g_" + request.param)), "fmt_g")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", *BUILDS[request.param], "-I", CSRC, os.path.join(ROOT, "tests", "abi", "fmt_g.cpp"),
                    os.path.join(CSRC, "rawdtw_aln_text.cpp"), "-o", out], check=True)
    return out


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def test_lattice_holds_what_it_says():
    v = A.value_lattice()
    assert v.dtype == np.uint32 and len(np.unique(v)) == len(v) and 6_000_000 < len(v) < 16_000_000
    have = set(v[np.isin(v >> 23, [0, 1, 254, 255, 256, 511])].tolist())
    for f in (0, 1, 254, 255, 256, 511):
        for m in A.FIXED_MANTISSAS:
            assert (f << 23 | m) in have
    for x in (100000.5, 999999.5, 1000005.0, 16777205.0, 1e-45, 1e38, 1e-5, 1e6):
        b = int(np.float32(x).view(np.uint32))
        i = np.searchsorted(v, b)
        assert v[i] == b and v[i - 1] == b - 1 and v[i + 1] == b + 1, x


def test_fmt_g_against_snprintf_on_the_lattice(exe, tmp_path):
    v = A.value_lattice()
    path = os.path.join(str(tmp_path), "lattice.u32")
    v.tofile(path)
    assert run(exe, "values", path) == "ok %d" % len(v)


def test_u64_to_decimal(exe):
    assert run(exe, "u64") == "ok 68"


def test_host_text_in_exact_buffers(exe):
    assert run(exe, "host") == "ok 8"


def test_the_python_model_prints_the_literal_cases():
    for x, text in A.LITERALS:
        assert A.fmt_g(np.float32(x)) == text, x
    assert A.fmt_g(np.uint32(0xffc00000).view(np.float32)) == "-nan" and A.fmt_g(np.uint32(0x7fc00000).view(np.float32)) == "nan"


def jobs_for(plen):
    """job records whose n + m - 1 is the path's length (n + m - 1 >= 1: an empty path gets the smallest job)"""
    jobs = np.zeros(len(plen), ra.JOB_DTYPE)
    jobs["n"] = np.maximum(1, (np.asarray(plen, np.int64) + 1) // 2)
    jobs["m"] = np.maximum(1, np.asarray(plen, np.int64) + 1 - jobs["n"].astype(np.int64))
    assert np.all(jobs["n"].astype(np.int64) + jobs["m"] - 1 >= plen)
    return jobs


def check_host(step, d, off, plen, recs):
    want_off, want = A.model_text(step, d, off, plen, recs)
    for threads in (1, 3):
        toff, text = ra.aln_text_host(step, d, off, plen, recs, threads=threads)
        assert np.array_equal(toff, want_off) and text.tobytes() == want
    toff, none = ra.aln_text_host(step, d, off, plen, recs, sizes_only=True)     # text == NULL
    assert none is None and np.array_equal(toff, want_off)
    if len(want):
        with pytest.raises(ra.RawDTWError) as err:                               # a cap one byte short
            ra.aln_text_host(step, d, off, plen, recs, cap=len(want) - 1)
        assert err.value.status == 4
    toff, text = ra.aln_text_host(step, d, off, plen, recs, cap=len(want))       # ... and the exact one
    assert text.tobytes() == want
    bound = ra.aln_text_bound(jobs_for(plen), recs)
    assert bound >= len(want)
    # every job alone: its bound holds for it, too
    for k in range(len(plen)):
        assert ra.aln_text_bound(jobs_for(plen[k:k + 1]), recs[k:k + 1]) >= int(want_off[k + 1] - want_off[k]), k
    return want_off, want


def test_host_text_against_the_python_model_on_the_edge_paths():
    step, d, off, plen, recs = A.edge_paths()
    want_off, want = check_host(step, d, off, plen, recs)
    assert set(plen.tolist()) >= set(A.PATH_LENS) and {0, 1} == set(recs["mode"].tolist()) and (recs["j0"] != 0).any()
    assert np.all(want_off[1:][plen == 0] == want_off[:-1][plen == 0])           # an empty job occupies nothing
    text = want.decode()
    for s in (",9,", ",10,", "(9,", "(10,", "(999,", "(1000,", "(4294967295,", "(4294967296,", ",4294967295,", ",4294967296,"):
        assert s in text, s
    # mode 0: only the last element moved, by len * offset in 64-bit arithmetic
    k = int(np.nonzero((recs["mode"] == 0) & (plen == 129))[0][-1])
    last = text[int(want_off[k]):int(want_off[k + 1])].rsplit("(", 1)[1]
    pi = int(np.sum(step[int(off[k]):int(off[k]) + 129] & 1))
    assert int(last.split(",")[0]) == pi + 129 * int(recs["off_i"][k]) > (1 << 32) and text[int(want_off[k]):].startswith("(0,0,")


def test_exclude_last_is_a_shorter_path():
    """what the traceback's exclude_last does before the text is made: the job's last element is gone, and under mode 0 len is the shortened length"""
    rng = np.random.default_rng(3)
    step, d, off, plen = A.random_paths([65, 2, 130], rng)
    recs = np.concatenate([A.rec(7, 9, 0, 0), A.rec(7, 9, 0, 0), A.rec(11, 1 << 33, 4, 1)])
    full_off, full = A.model_text(step, d, off, plen, recs)
    short_off, short = check_host(step, d, off, plen - 1, recs)
    t0 = full[int(full_off[2]):int(full_off[3])].decode()
    assert short[int(short_off[2]):].decode() == t0[:t0.rindex("(")]              # mode 1: a prefix
    a, b = full[:int(full_off[1])].decode(), short[:int(short_off[1])].decode()
    assert a.count("(") == 65 and b.count("(") == 64 and b.rsplit("(", 1)[1].split(",")[0] == str(int(np.sum(step[:64] & 1)) + 64 * 7)


def test_host_text_refuses_what_it_cannot_read():
    step, d, off, plen = A.random_paths([3], np.random.default_rng(1))
    with pytest.raises(ra.RawDTWError) as err:
        ra.aln_text_host(step, d, off, plen, A.rec(mode=2))
    assert err.value.status == 1
    toff, text = ra.aln_text_host(step[:0], d[:0], [0], np.zeros(0, np.uint32), np.zeros(0, ra.ALN_REC_DTYPE))
    assert toff.tolist() == [0] and len(text) == 0


@pytest.mark.parametrize("setter", [None, False, True])
def test_scorer_only_mappers_are_what_they_were(oracle, setter):
    """tests/test_mapper_cpu.py's workload, flags 0x2 | 0x8 on four threads: the lines and the log of a mapper whose setter was never
    called, was called with off and -- no device, no flag 0x4: the finish has nothing to do -- with on are the Python mirror's"""
    ref = synth.make_reference([29903, 12000], seed=20231005 + 1)
    n = 30
    seeds = mapper.SyntheticSeeds(ref, n, seed=11, max_chunks=4)
    opt, stop = ra.MapOpt(flag=0x2 | 0x8), StopOpt(min_events=300)
    lo = []
    want, rounds = mapper.map_reads(seeds, list(range(n)), OracleScorer(oracle, ref), opt, stop, log=lo)
    cm = mapper.CMapper(None, opt, stop, [f"seq{s}" for s in range(ref.n_seq)], [len(x) for x in ref.forward],
                        slot_events=max(rd["n_ev"] for rd in seeds.reads) + 8, max_reads=n, carry=True, threads=4)
    cm.set_scorer(_oracle_scorer(oracle, ref, opt))
    if setter is False:
        cm.set_device_text(False)
    got, rounds_c = mapper.map_reads_c(seeds, list(range(n)), cm, device_text=bool(setter))
    assert got == want and rounds_c == rounds and cm.log() == "".join(lo)
    cm.close()
