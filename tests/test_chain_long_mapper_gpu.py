"""The mapper with the device chaining's long path on (rawdtw_set_option "chain_long_seeds" on the mapper's context): rounds that a lowered
RAWDTW_CHAIN_MAX_SEEDS used to send back to the host are chained on the device, plain and resident, with the reference's recorded lines
(tests/golden/); a second group's context inherits the option."""
import pytest

import rawalign_amd as ra
from rawalign_amd import mapper
from rawalign_amd.mapping import StopOpt
from rawalign_amd.seeding import SeedIndex
from tests import map_ref_cases as K
from tests.test_map_ref import check_lines_after_c_chunks, check_lines_default_stop, run_c_mapper, whole_read_lines_c
from tests.test_resident_round_gpu import _whole_mapper

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return K.make_reference()


@pytest.mark.parametrize("name", ["default", "nofilter", "global_full"])
def test_device_mapper_chains_the_rounds_above_a_lowered_cap_itself(ref, name, monkeypatch):
    """tests/test_map_ref_gpu.py::test_device_mapper_with_rounds_the_device_declines with the option on: a cap of 300 puts a read's later rounds
    (the chains' anchors on top of a chunk's hits) on the long path in the middle of a read"""
    monkeypatch.setenv("RAWDTW_CHAIN_MAX_SEEDS", "300")
    fx = K.Fixture(ref=ref)
    e = ra.Engine(0)
    e.upload_reference(fx.ref.forward, fx.ref.reverse)
    try:
        e.set_option("chain_long_seeds", 65536)
        for groups in (1, 2):
            before = e.chain_round_stats()["long_reads"]
            lines = run_c_mapper(fx, name, 1, StopOpt(**K.NEVER), engine=e, threads=3, groups=groups, carry=False, device_chain=True)
            check_lines_after_c_chunks(fx, name, 1, 99, lines, "device mapper, long path")
            check_lines_default_stop(fx, name, 1, run_c_mapper(fx, name, 1, StopOpt(), engine=e, threads=3, groups=groups, carry=False, device_chain=True),
                                     "device mapper, long path")
            assert e.chain_round_stats()["long_reads"] > before, groups
    finally:
        e.close()


def test_resident_rounds_above_a_lowered_cap_stay_resident(ref, monkeypatch):
    """tests/test_resident_round_gpu.py::test_a_lowered_seed_cap_falls_back_to_the_host_with_the_same_lines with the option on: a cap of 60 under
    chunks of up to 147 hits, and no round falls back, no hit comes home"""
    monkeypatch.setenv("RAWDTW_CHAIN_MAX_SEEDS", "60")
    six = SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)
    wr = K.WholeReads(0, ref=ref)
    want = [wr.expected_line("default", r) for r in range(wr.n_reads)]
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        e.set_option("chain_long_seeds", 65536)
        opt, copt = K.whole_project_opts("default", 0)
        cm = _whole_mapper(e, wr, opt, copt, groups=1, device_chain=True)
        got, rounds = mapper.map_reads_c(wr, list(range(wr.n_reads)), cm, seed_index=six, resident=True)
        st = cm.resident_stats()
        cm.close()
        print(rounds, st, e.chain_round_stats())
        assert got == want
        assert st["fallback_rounds"] == 0 and st["resident_rounds"] == rounds and st["hit_bytes_to_host"] == 0
        assert e.chain_round_stats()["long_reads"] > 0
    finally:
        e.close()


def test_two_groups_with_the_option_on_the_first_context_give_one_groups_lines(ref, monkeypatch):
    monkeypatch.setenv("RAWDTW_CHAIN_MAX_SEEDS", "60")
    wr = K.WholeReads(0, ref=ref)
    want = [wr.expected_line("default", r) for r in range(wr.n_reads)]
    e = ra.Engine(0)
    try:
        e.upload_reference(ref.forward, ref.reverse)
        e.set_option("chain_long_seeds", 65536)
        lines = {}
        for groups in (1, 2):
            before = e.chain_round_stats()["long_reads"]
            lines[groups] = whole_read_lines_c(wr, "default", 0, engine=e, threads=3, groups=groups, carry=False, device_chain=True)
            assert e.chain_round_stats()["long_reads"] > before, groups
        assert lines[2] == lines[1] == want
    finally:
        e.close()
