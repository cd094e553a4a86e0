"""tests/chain_lattice_cases.py through rawdtw_chain_round: every round of constructed probe reads -- the predecessor loop's exit, winner and
carried skip counter on every lane of three blocks, exact ties, the value edges of the scoring, the end filter and the traceback's break
(checked and counted on the host by tests/test_chain_lattice_cpu.py) -- against the host restatement, with tests/test_device_chain.py's
compare: scores bit for bit, positions, every anchor.  Through all four kernels that inline chain_step: k_chain, k_chain<true>
("chain_max_chains"), k_chain_long (a cap of one seed a read, "chain_long_seeds") and k_chain_long<true>."""
import pytest

from tests.test_chain_many_gpu import device_round   # (first: it brings torch up before the library)

import rawalign_amd as ra
from tests import chain_lattice_cases as cl
from tests.test_device_chain import compare

pytestmark = pytest.mark.gpu
CONFIGS = {"k_chain": (False, False), "k_chain_many": (True, False), "k_chain_long": (False, True), "k_chain_long_many": (True, True)}
ROUNDS = cl.rounds()


@pytest.fixture(scope="module", params=list(CONFIGS))
def eng(request):
    many, long_path = CONFIGS[request.param]
    with pytest.MonkeyPatch.context() as mp:
        if long_path:
            mp.setenv("RAWDTW_CHAIN_MAX_SEEDS", "1")   # (read when the context is created)
        e = ra.Engine(0)
    if long_path:
        e.set_option("chain_long_seeds", 4096)
    if many:
        e.set_option("chain_max_chains", 512)
    e.long_path = long_path
    yield e
    e.close()


@pytest.mark.parametrize("k", range(len(ROUNDS)), ids=[name.replace(" ", "_").replace(",", "") for name, _, _ in ROUNDS])
def test_round_equals_the_host(eng, k):
    name, copt, probes = ROUNDS[k]
    per_read = [p["seeds"] for p in probes]
    before = eng.chain_round_stats()
    out = device_round(eng, copt, per_read, n_keys=2)
    assert out[0] == 0, eng.lib.rawdtw_last_error(eng._ctx)
    # read by read, so that a failure names every case family it is in (compare's last check holds at every read's end)
    st, chain_off, anchor_off, recs, anchors = out[:5]
    bad = []
    for r, p in enumerate(probes):
        try:
            compare(eng.lib, copt, [p["seeds"]], (st, chain_off[r:r + 2], anchor_off, recs, anchors, None, None, None))
        except AssertionError:
            bad.append((p["family"], p["name"]))
    assert not bad, (name, len(bad), sorted({f for f, _ in bad}), [n for _, n in bad[:12]])
    after = eng.chain_round_stats()
    # no silent reroute: with the cap at one seed every read of two or more went through k_chain_long, otherwise none did
    want_long = sum(len(s) > 1 for s in per_read) if eng.long_path else 0
    assert (after["rounds"] - before["rounds"], after["long_reads"] - before["long_reads"]) == (1, want_long), name
