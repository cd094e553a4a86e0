#!/usr/bin/env python3
"""The HIP calls behind the mapper's round entries, for refactors of rawdtw_mapper*.cpp that must not move them.  The nine whole reads of
tests/golden/map_ref_reads.npz (up to four chunks a read, three sequences) through every round entry, each flow between two markers (a pair
of hipDeviceSynchronize, which the library never calls) on an engine and a mapper of its own:
    rawdtw_mapper_round               chains on the host with carry and --dtw-output-cigar (a rawdtw_mapper_finish that uploads the host's copies);
                                      on the device with two read groups; on the device with "device_round_end", and with
                                      "chain_decline_reads" under a cap of 110 seeds a read (reads declined alone in a plain round)
    rawdtw_mapper_round_seeded        device chaining
    rawdtw_mapper_round_seeded_resident   nothing on; "device_round_end" + "resident_chains"; those under a cap of 270 seeds with the stop rule
                                      that never fires -- round 3 falls back as a whole; and with "chain_decline_reads" too -- it declines one read
    rawdtw_mapper_round_signal_resident   every opt-in on
    rawdtw_mapper_round_raw_resident  "signal_cigar" on, --dtw-output-cigar (a rawdtw_mapper_finish that reads the arena)
The caps are the tests' (tests/chain_decline_cases.py), lowered as they lower them: RAWDTW_CHAIN_MAX_SEEDS around rawdtw_create.
Per flow the PAF lines, the log, the six stats entries and rawdtw_mapper_timing's slots 5-7 go to a JSON file.

    RAWDTW_LIBRARY=<library> rocprofv3 --hip-trace --output-format csv -d <dir> -o <name> -- python scripts/mapper_calls_probe.py <results.json>
    python scripts/mapper_calls_probe.py compare <parent>_hip_api_trace.csv <new>_hip_api_trace.csv <parent results> <new results> [out.json]
`compare`: the ordered lists of HIP API names from the first marker to the last and the two result files, side by side."""
import ctypes as C
import difflib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.batch_calls_probe import calls_between_markers  # noqa: E402


def compare(parent, new, parent_results, new_results, out=None):
    (a, ma), (b, mb) = calls_between_markers(parent), calls_between_markers(new)
    # what differs, as the calls the parent made and this tree does not (and the other way round), by name
    gone, came = {}, {}
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
        if tag != "equal":
            for x in a[i1:i2]:
                gone[x] = gone.get(x, 0) + 1
            for x in b[j1:j2]:
                came[x] = came.get(x, 0) + 1
    ra_, rb_ = json.load(open(parent_results)), json.load(open(new_results))
    same = {k: ra_[k] == rb_.get(k) for k in ra_}
    res = {"probe": "mapper_calls_probe", "what": "HIP API names in order between the script's first and last marker, and per flow the PAF lines, the log, the "
           "six stats entries and timing slots 5-7: parent's library and this tree's",
           "markers": {"parent": ma, "new": mb}, "calls": {"parent": len(a), "new": len(b)}, "only_in_parent": gone, "only_in_new": came,
           "flows": list(ra_), "results_equal": same,
           "verdict": ("equal" if a == b else "calls differ") + (", results equal" if all(same.values()) and list(ra_) == list(rb_) else ", RESULTS DIFFER")}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return all(same.values()) and not came


def main(out_path):
    try:  # PyTorch bundles its own HIP runtime: when both live in one process, torch has to come up first
        import torch  # noqa: F401
    except Exception:  # noqa: BLE001
        pass
    import rawalign_amd as ra
    from rawalign_amd import mapper
    from rawalign_amd.mapping import StopOpt
    from rawalign_amd.seeding import SeedIndex
    from tests import chain_decline_cases as dc
    from tests import map_ref_cases as mc
    from tests import optins_cases as oc
    from tests.test_signal_cigar_gpu import _DacSignal
    from tests.test_signal_round_gpu import _Signal

    hip = C.CDLL("libamdhip64.so")

    def mark():
        hip.hipDeviceSynchronize()
        hip.hipDeviceSynchronize()

    ref = mc.make_reference()
    six = SeedIndex.from_signals(ref.forward, ref.reverse, threads=4)
    wr = mc.WholeReads(0, ref=ref)
    raws = mc.make_raw_reads()
    names, lens, reads = ["seq%d" % s for s in range(len(wr.lens))], [int(x) for x in wr.lens], list(range(wr.n_reads))
    results = {}

    def flow(name, src, opts="default", options=None, cap=None, stop=None, **how):
        """one engine (created under `cap`), one mapper, map_reads_c to the end; mapper.CMapper's and map_reads_c's keywords in `how`"""
        if cap is not None:   # (read at rawdtw_create: the engine's context, and a second read group's inside rawdtw_mapper_create)
            os.environ["RAWDTW_CHAIN_MAX_SEEDS"] = str(cap)
        e = ra.Engine(0)
        e.upload_reference(ref.forward, ref.reverse)
        for k, v in (options or {}).items():
            e.set_option(k, v)
        opt, copt = mc.whole_project_opts(opts, 0)
        made = {k: how.pop(k) for k in ("carry", "groups", "device_chain") if k in how}
        mark()
        cm = mapper.CMapper(e, opt, stop or StopOpt(), names, lens, slot_events=4096, max_reads=wr.n_reads, chain_opt=copt, output_chains=True, threads=3,
                            **dict(dict(carry=False, groups=1, device_chain=True), **made))
        lines, rounds = mapper.map_reads_c(src, reads, cm, **how)
        tm = cm.timing()
        results[name] = dict(lines=lines, rounds=rounds, log=cm.log(), stats=cm.stats(), resident=cm.resident_stats(), signal=cm.signal_stats(),
                             round_end=cm.round_end_stats(), kept=cm.kept_stats(), decline=cm.decline_stats(),
                             bytes=[tm["anchor_bytes"], tm["event_bytes"], tm["other_bytes"]])
        cm.close()
        mark()
        e.close()
        os.environ.pop("RAWDTW_CHAIN_MAX_SEEDS", None)
        print(name, rounds, "rounds", results[name]["resident"], results[name]["decline"], flush=True)

    kept_on = dict(device_round_end=1, resident_chains=4096)
    fb = dc.MAPPER_CASES["whole_fb"]
    flow("round_host_carry_cigar", wr, opts="cigar", carry=True, device_chain=False)
    flow("round_device_two_groups", wr, groups=2)
    flow("round_device_round_end", wr, options=dict(device_round_end=1))
    flow("round_device_declines", wr, options=dict(device_round_end=1, chain_decline_reads=1), cap=dc.WHOLE_CAP, groups=2)
    flow("seeded", wr, seed_index=six)
    flow("resident_plain", wr, seed_index=six, resident=True)
    flow("resident_kept", wr, options=kept_on, seed_index=six, resident=True)
    flow("resident_falls_back", wr, options=kept_on, cap=fb["cap"], stop=oc.never(), seed_index=six, resident=True)
    flow("resident_declines_one", wr, options=dict(kept_on, chain_decline_reads=1), cap=fb["cap"], stop=oc.never(), seed_index=six, resident=True)
    flow("signal_all_on", _Signal(wr, raws), options=dict(kept_on, chain_decline_reads=1), seed_index=six, signal=True, event_opt=ra.EventOptions(contracted=False))
    flow("raw_signal_cigar", _DacSignal(wr, raws), opts="cigar", options=dict(signal_cigar=1), seed_index=six, signal=True, event_opt=ra.EventOptions(contracted=False))
    assert results["resident_falls_back"]["resident"]["fallback_rounds"] == 1 and results["resident_declines_one"]["resident"]["fallback_rounds"] == 0
    assert results["resident_declines_one"]["decline"]["reads_declined_seeds"] == 1 and results["round_device_declines"]["decline"]["rounds_with_declines"] > 0
    assert results["signal_all_on"]["signal"]["rounds"] > 0 and results["raw_signal_cigar"]["signal"]["rounds"] > 0
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("mapper_calls_probe: %d flows done" % len(results))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "compare":
        sys.exit(0 if compare(*sys.argv[2:7]) else 1)
    main(sys.argv[1] if len(sys.argv) > 1 else os.devnull)
