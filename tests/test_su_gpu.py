"""--sequence-until (and --output-chains) through the library's mapper on the device: a seven-sequence reference, the chaining
on the host and on the device, one read group and two, costs carried and not.  The lines, the stop point and su_state equal the
same mapper scored through the oracle hook (rawdtw_mapper_set_scorer); with sequence-until off the device writes today's lines,
and the sequence-until lines are exactly those, walked in mini-batches through mapping.SequenceUntil and gated (rmap.cpp:960)."""
import itertools

import pytest

import rawalign_amd as ra
from rawalign_amd import mapper, synth
from rawalign_amd.mapping import SequenceUntil, StopOpt
from tests.test_mapper_cpu import _oracle_scorer

N, BATCH = 60, 10
SU_KW = dict(t_threshold=1.5, tn_samples=2, ttest_freq=3, tmin_reads=8)


def _gate(line):
    f = line.split("\t")
    return "\t".join([f[0], f[1]] + ["*"] * 9 + [f[11]] + f[12:])


def _restate(lines_off, n_seq):
    """today's lines walked in mini-batches (records from the mapped lines, in order), gated at the stop, nothing after it"""
    su = SequenceUntil(n_seq, **SU_KW)
    out = [""] * len(lines_off)
    for b0 in range(0, len(lines_off), BATCH):
        f = [x.split("\t") for x in lines_off[b0:b0 + BATCH]]
        for k, x in enumerate(f):
            if x[2] != "*" and su.add_mapped_read(int(x[5][3:]), int(x[10]), k):
                break
        for k, line in enumerate(lines_off[b0:b0 + BATCH]):
            out[b0 + k] = _gate(line) if su.stop and k >= su.stop and f[k][2] != "*" else line
        if su.stop:
            return out, b0 // BATCH, su
    return out, None, su


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [0x2, 0x2 | 0x4, 0x2 | 0x20])
def test_device_mapper_sequence_until_equals_the_oracle_hook(oracle, flag):
    ref = synth.make_reference([20000, 35000, 12000, 8000, 26000, 15000, 30000], seed=20231005 + 9)
    seeds = mapper.SyntheticSeeds(ref, N, seed=13, max_chunks=4)
    names, lens = [f"seq{s}" for s in range(ref.n_seq)], [len(x) for x in ref.forward]
    slot = max(rd["n_ev"] for rd in seeds.reads) + 8
    ids = list(range(N))
    base = ra.MapOpt(flag=flag & ~0x20)
    oc = bool(flag & 0x20)
    stop = StopOpt()

    def make(eng, **kw):
        return mapper.CMapper(eng, base, stop, names, lens, slot_events=slot, max_reads=N, output_chains=oc, **kw)

    # the oracle hook: the same mapper, its rounds scored by the oracle (the CIGAR traceback of 0x4 still on the device)
    eng = ra.Engine(0)
    eng.upload_reference(ref.forward, ref.reverse)
    hook = make(eng, threads=4, sequence_until=SU_KW)
    hook.set_scorer(_oracle_scorer(oracle, ref, base))
    want, _ = mapper.map_reads_c(seeds, ids, hook, batch_size=BATCH)
    want_state = hook.su_state()
    hook.close()
    # sequence-until off: today's map_reads_c on the device
    off_cm = make(eng, threads=4, carry=True)
    off, _ = mapper.map_reads_c(seeds, ids, off_cm)
    off_cm.close()
    eng.close()
    restated, stop_batch, su = _restate(off, ref.n_seq)
    assert stop_batch in (1, 2, 3) and want == restated and want_state == (True, su.nreads)
    if oc:
        assert all("\tanchors:s:(" in line for line in off if line.split("\t")[2] != "*")
    if flag & 0x4:
        assert any("\taln:s:(" in line and line.split("\t")[3] == "*" for line in want), "a gated line keeps aln:s:"
    for dev, groups, carry in itertools.product((0, 1), (1, 2), (True, False)):
        eng = ra.Engine(0)
        eng.upload_reference(ref.forward, ref.reverse)
        cm = make(eng, threads=4, groups=groups, carry=carry, device_chain=bool(dev), sequence_until=SU_KW)
        got, _ = mapper.map_reads_c(seeds, ids, cm, batch_size=BATCH)
        assert got == want, (dev, groups, carry)
        assert cm.su_state() == want_state
        cm.close()
        eng.close()
