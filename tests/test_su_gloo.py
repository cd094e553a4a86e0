"""--sequence-until across two gloo ranks through the library's mapper: each rank maps its shard_reads block of every mini-batch
with a CMapper of its own (the oracle as the scorer, no device), hands the block's records (CMapper.batch_records) to
shard.sequence_until_round with a CSequenceUntil, and applies the decision to its block (CMapper.su_apply).  The ranks' lines put
together, the stop point and the counters equal one process closing the same mini-batches with su_batch."""
import multiprocessing as mp
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_READS, BATCH = 48, 12
SU_KW = dict(t_threshold=1.5, tn_samples=2, ttest_freq=2, tmin_reads=12)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup():
    from rawalign_amd import mapper, synth

    ref = synth.make_reference([24000, 15000, 9000], seed=20231005 + 31)
    seeds = mapper.SyntheticSeeds(ref, N_READS, seed=41, max_chunks=4)
    return ref, seeds


def _cmapper(ref, seeds, n):
    import rawalign_amd as ra
    from oracle.loader import Oracle
    from rawalign_amd import mapper
    from rawalign_amd.mapping import StopOpt
    from tests.test_mapper_cpu import _oracle_scorer

    opt = ra.MapOpt()
    cm = mapper.CMapper(None, opt, StopOpt(), [f"seq{s}" for s in range(ref.n_seq)], [len(x) for x in ref.forward],
                        slot_events=max(rd["n_ev"] for rd in seeds.reads) + 8, max_reads=n, threads=2, sequence_until=SU_KW)
    cm.set_scorer(_oracle_scorer(Oracle(), ref, opt))
    return cm


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from rawalign_amd.mapper import CSequenceUntil
    from rawalign_amd.shard import sequence_until_round, shard_reads

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ref, seeds = _setup()
        cm = _cmapper(ref, seeds, N_READS)
        su = CSequenceUntil(ref.n_seq, **SU_KW)
        lines, stops = {}, []
        for b0 in range(0, N_READS, BATCH):
            batch = list(range(b0, min(N_READS, b0 + BATCH)))
            lo, hi = shard_reads(len(batch), rank, world)
            mine = batch[lo:hi]
            ids = [cm.add_read(seeds.read_job(r).name, seeds.read_job(r).qlen, seeds.read_job(r).n_chunks_available) for r in mine]
            while True:
                act = [(i, r) for i, r in zip(ids, mine) if not cm.state(i)[0]]
                if not act:
                    break
                cm.round([i for i, _ in act], [seeds.chunk(r, cm.state(i)[1]) for i, r in act])
            mapped, ref_id, frag = cm.batch_records(ids)
            s = sequence_until_round(dist, su, mapped, ref_id, frag, len(batch))
            cm.su_apply(ids, None if s == 0 else min(max(s - lo, 0), hi - lo))
            stops.append(s)
            for i, r in zip(ids, mine):
                lines[r] = i
            if s:
                break
        assert cm.finish() == 0
        out = {r: cm.paf(i) for r, i in lines.items()}
        q.put((rank, out, stops, su.nreads, su.c_estimations.tolist(), cm.su_state()))
        cm.close()
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_sequence_until_across_two_ranks_equals_one_process(oracle):
    from rawalign_amd import mapper
    from rawalign_amd.shard import sequence_until_round

    ref, seeds = _setup()
    one = _cmapper(ref, seeds, N_READS)
    want, _ = mapper.map_reads_c(seeds, list(range(N_READS)), one, batch_size=BATCH)
    stopped, n_mapped = one.su_state()
    assert stopped and 0 < n_mapped
    # the one process's stop point and counters, replayed from its lines: a normal mapped line carries the record (genome in
    # field 5, fragment length in field 10); gated lines only follow the stop, and unmapped ones never count
    stop_batch = max(r for r in range(N_READS) if want[r]) // BATCH
    want_su, want_stops = mapper.CSequenceUntil(ref.n_seq, **SU_KW), []
    for bi in range(stop_batch + 1):
        f = [want[r].split("\t") for r in range(bi * BATCH, min(N_READS, (bi + 1) * BATCH))]
        m = [x[2] != "*" for x in f]
        want_stops.append(sequence_until_round(None, want_su, m, [int(x[5][3:]) if y else 0 for x, y in zip(f, m)],
                                               [int(x[10]) if y else 0 for x, y in zip(f, m)], len(f)))
    assert want_stops[-1] > 0 and not any(want_stops[:-1]) and want_su.nreads == n_mapped
    assert stop_batch in (1, 2)

    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
    got.sort(key=lambda x: x[0])
    lines = {}
    for _, out, _, _, _, _ in got:
        assert not set(out) & set(lines)
        lines.update(out)
    assert [lines.get(r, "") for r in range(N_READS)] == want
    (_, _, stops0, nr0, ce0, st0), (_, _, stops1, nr1, ce1, st1) = got
    assert stops0 == stops1 == want_stops
    assert nr0 == nr1 == n_mapped and ce0 == ce1 == want_su.c_estimations.tolist()
    assert st0[0] and st1[0] and st0[1] + st1[1] == n_mapped
    one.close()
